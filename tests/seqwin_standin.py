"""TEST INFRASTRUCTURE: a stand-in `checkm` package for the drop-in tests of the plot hooks, written to a directory: the modules
dropin.install() touches with the top-level classes the reference defines (tests/golden/reference_module_classes.json), and four plot
modules of this project's own.  They are NOT the reference's plot classes and share no text with them: each is a thin class over one
generic walker (`checkm/plot/_walk.py` below) that visits window k of every sequence for k in range((len - 1) // w) and asks the names
its module imported -- `readFasta`, `baseCount(text[k*w:(k+1)*w])`, `baseCount(text)`, `codingBases(name, k*w, (k+1)*w)`,
`seqSignature`, `distance` -- which are exactly the names dropin.install() rebinds.  So the default run of the drop-in tests covers the
hook PROTOCOL only; the reference's unmodified classes are exercised when tests/seqwin_dropin_driver.py is given a CheckM source tree."""
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SEQ_UTILS = '''
import re


def readFasta(fastaFile, trimHeader=True):
    records = re.split(r"^>", open(fastaFile).read(), flags=re.M)[1:]
    return {r.split(None, 1)[0]: "".join(r.split("\\n")[1:]) for r in records}


def baseCount(seq):
    up = seq.upper()
    return tuple(sum(up.count(ch) for ch in group) for group in ("A", "C", "G", "TU"))
'''

WALK = '''
def windows(bin_, w):
    """(name, text, k) for every window k of every sequence of {name: text}: k w .. (k + 1) w, while a base is left behind it."""
    for name, text in bin_.items():
        for k in range((len(text) - 1) // w if len(text) else 0):
            yield name, text, k


def lengths(bin_):
    return [len(text) for text in bin_.values()]
'''

GC_PLOTS = '''
from checkm.util.seqUtils import readFasta, baseCount
from checkm.plot._walk import lengths, windows


class GcPlots(object):
    def __init__(self, options):
        self.w = options.gc_window_size

    def plotOnAxes(self, fastaFile, distributionsToPlot, axesHist, axesDeltaGC):
        bin_ = readFasta(fastaFile)
        counts = [baseCount(text[k * self.w:(k + 1) * self.w]) for _name, text, k in windows(bin_, self.w)]
        fractions = [float(n[2] + n[1]) / sum(n) for n in counts if sum(n)]
        if fractions:
            axesHist.hist(fractions)
            axesDeltaGC.scatter(None, lengths(bin_))
'''

GC_BIAS_PLOTS = '''
from checkm.util.seqUtils import readFasta, baseCount
from checkm.plot._walk import windows


def fraction(n):
    return float(n[2] + n[1]) / sum(n)


class GcBiasPlot(object):
    def __init__(self, options):
        self.w = options.window_size

    def plotOnAxes(self, binFile, coverageProfile, windowAxes, seqAxes):
        bin_ = readFasta(binFile)
        per_window, per_seq = [], []
        for name, text in bin_.items():
            per_window += [fraction(baseCount(t[k * self.w:(k + 1) * self.w])) for _n, t, k in windows({name: text}, self.w)]
            per_seq.append(fraction(baseCount(text)))
        windowAxes.scatter(per_window, None)
        seqAxes.scatter(per_seq, None)
'''

CD_PLOTS = '''
import os

from checkm.prodigal import ProdigalGeneFeatureParser
from checkm.util.seqUtils import readFasta, baseCount
from checkm.plot._walk import lengths, windows


class CodingDensityPlots(object):
    def __init__(self, options):
        self.w, self.out = options.cd_window_size, options.results_dir

    def plotOnAxes(self, fastaFile, distributionsToPlot, axesHist, axesDeltaCD):
        gff = os.path.join(self.out, "bins", os.path.basename(fastaFile).rsplit(".", 1)[0], "genes.gff")
        if not os.path.isfile(gff):
            raise SystemExit(1)
        genes = ProdigalGeneFeatureParser(gff)
        bin_ = readFasta(fastaFile)
        density = []
        for name, text, k in windows(bin_, self.w):
            lo, hi = k * self.w, (k + 1) * self.w
            density.append(float(genes.codingBases(name, lo, hi)) / sum(baseCount(text[lo:hi])))
        if density:
            axesHist.hist(density)
            axesDeltaCD.scatter(None, lengths(bin_))
'''

TD_PLOTS = '''
import functools
import operator

from checkm.util.seqUtils import readFasta
from checkm.genomicSignatures import GenomicSignatures
from checkm.plot._walk import lengths, windows


class TetraDistPlots(object):
    def __init__(self, options):
        self.w = options.td_window_size

    def plotOnAxes(self, fastaFile, tetraSigs, distributionsToPlot, axesHist, axesDeltaTD):
        bin_ = readFasta(fastaFile)
        total = sum(lengths(bin_))
        centre = functools.reduce(operator.iadd, (tetraSigs[name] * (float(len(text)) / total) for name, text in bin_.items()))
        gs = GenomicSignatures(K=4, threads=1)
        per_window = [gs.distance(gs.seqSignature(text[k * self.w:(k + 1) * self.w]), centre) for _name, text, k in windows(bin_, self.w)]
        if per_window:
            axesHist.hist(per_window)
            axesDeltaTD.scatter([gs.distance(tetraSigs[name], centre) for name in bin_], lengths(bin_))
'''


def write_package(d):
    """Writes <d>/checkm and returns d (to be put in front of sys.path)."""
    pkg = os.path.join(str(d), "checkm")
    os.makedirs(os.path.join(pkg, "util"))
    os.makedirs(os.path.join(pkg, "plot"))
    for sub in ("", "util", "plot"):
        open(os.path.join(pkg, sub, "__init__.py"), "w").close()
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_module_classes.json")))["classes"]
    for mod, classes in gold.items():
        open(os.path.join(pkg, mod.split(".")[1] + ".py"), "w").write("".join("class %s(object):\n    pass\n\n\n" % c for c in classes))
    open(os.path.join(pkg, "genomicSignatures.py"), "w").write("class GenomicSignatures(object):\n    pass\n")
    open(os.path.join(pkg, "util", "seqUtils.py"), "w").write(SEQ_UTILS)
    for name, text in (("_walk", WALK), ("gcPlots", GC_PLOTS), ("gcBiasPlots", GC_BIAS_PLOTS), ("codingDensityPlots", CD_PLOTS), ("tetraDistPlots", TD_PLOTS)):
        open(os.path.join(pkg, "plot", name + ".py"), "w").write(text)
    return str(d)
