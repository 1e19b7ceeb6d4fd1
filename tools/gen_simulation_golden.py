#!/usr/bin/env python
"""Goldens of the marker-set simulation: the reference's own MarkerSetBuilder (scripts/genometreeworkflow/markerSetBuilder.py: uniformity,
sampleGenome, sampleGenomeScaffolds*, containedMarkerGenes), the worker and writer bodies of scripts/simulation.py, and
checkm.markerSets.MarkerSet / BinMarkerSets, over small hand-made genomes.  Both scripts are Python 2 and do not compile as they stand;
their text is loaded in memory after the substitutions listed below (each checked to hit) and never written to disk.  The script's
surroundings -- its authors' files, the tree, the queues, the two output paths under /tmp -- are stand-ins handed to the loaded functions,
not changes of their text.  Per case: the seed, the positions and the marker sets; every draw (trueComp, trueCont, the starts);
containedMarkerGenes per marker set; both genomeCheck results as float.hex(); the tuples the worker put on its queue; the writer's two
texts.  Runs only where a CheckM source tree is at hand; the tests read the JSON.
usage: CHECKM_SOURCE=<checkm source> python tools/gen_simulation_golden.py                (writes tests/golden/simulation_cases.json)
       CHECKM_SOURCE=<checkm source> python tools/gen_simulation_golden.py --time --mb N
                                      (times the reference's containedMarkerGenes + genomeCheck loop on one core over the synthetic
                                       genome of tools/simulation_bench.py, writes profiles/r18_simulation_reference_cpu.json)"""
import contextlib
import gzip
import io
import json
import os
import random
import re
import sys
import tempfile
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.gen_markerset_golden import SUBSTITUTIONS as KNOWN_FOUR, EXPECTED_HITS as KNOWN_HITS      # noqa: E402

# (what, pattern, replacement): Python 2 -> 3, nothing else
BUILDER_SUBSTITUTIONS = KNOWN_FOUR + [("integer division in sampleGenome", r"contigsInGenome = genomeLen / contigLen", "contigsInGenome = genomeLen // contigLen"),
                                      ("keys() as a list for numpy's choice", r"choice\(seqLens\.keys\(\)", "choice(list(seqLens.keys())")]
BUILDER_HITS = dict(KNOWN_HITS, **{"integer division in sampleGenome": 1, "keys() as a list for numpy's choice": 2})
SIMULATION_SUBSTITUTIONS = [("xrange", r"\bxrange\(", "range("),
                            ("print statements of the worker", r"(?m)^(\s*)print (.*?)\s*$", r"\1print(\2)"),
                            ("gzip file of str opened as text", r"(gzip\.open\('[^']*', )'wb'\)", r"\1'wt')")]
SIMULATION_HITS = {"xrange": 1, "print statements of the worker": 5, "gzip file of str opened as text": 2}      # one of the two is commented out in the script


def translate(text, substitutions, hits):
    for what, pattern, repl in substitutions:
        text, n = re.subn(pattern, repl, text)
        if n < 1 or n != hits.get(what, n):
            raise SystemExit("substitution '%s' hit %d times" % (what, n))
    return text


def load_builder(source):
    """The reference's MarkerSetBuilder class, compiled from the translated text in memory."""
    text = translate(open(os.path.join(source, "scripts", "genometreeworkflow", "markerSetBuilder.py")).read(), BUILDER_SUBSTITUTIONS, BUILDER_HITS)
    ns = {"__name__": "reference_markerSetBuilder"}
    exec(compile(text, "<markerSetBuilder.py, translated in memory>", "exec"), ns)
    return ns["MarkerSetBuilder"]


def load_worker_and_writer(source, read_fasta_bases, open_file, gzip_module):
    """(__workerThread, __writerThread) of the reference's Simulation as plain functions of (self, ...): the text between the two `def`s
    and `def run`, dedented, translated and compiled in memory.  The module's imports (dendropy, its authors' lib package) are not run: the
    names the two bodies use are given here."""
    text = open(os.path.join(source, "scripts", "simulation.py")).read()
    m = re.search(r"(?ms)^    def __workerThread\(.*?(?=^    def run\()", text)
    if not m:
        raise SystemExit("worker and writer bodies not found")
    body = translate(re.sub(r"(?m)^    ", "", m.group(0)), SIMULATION_SUBSTITUTIONS, SIMULATION_HITS)
    from collections import defaultdict
    from numpy import abs, mean, std
    ns = dict(os=os, sys=sys, defaultdict=defaultdict, gzip=gzip_module, mean=mean, std=std, abs=abs, readFastaBases=read_fasta_bases, open=open_file)
    exec(compile(body, "<simulation.py worker and writer, translated in memory>", "exec"), ns)
    return ns["__workerThread"], ns["__writerThread"]


# ---- the cases --------------------------------------------------------------------------------------------------------------------------------
def marker_set(uid, lineage, genomes, sets):
    return dict(UID=uid, lineageStr=lineage, numGenomes=genomes, sets=[sorted(s) for s in sets])


def cases():
    c = []
    # 10 whole contigs of 1000 (and 3 of 3000) in 10500 bases.  Copies exactly at a contig's start, its last base, the next contig's start
    # and the base before (M_start .. M_before around 3000 / 4000); a copy beyond the last whole contig (M_tail); markers with 0 (a key
    # with an empty list), 1, 2 and 5 copies; M_absent has no key; M_two sits in two co-located sets of one marker set; with completeness
    # 1.0 every contamination contig repeats a completeness contig.  Two sets of the chain share a lineageStr, and the refined chain
    # lacks it.
    pos = {"M_start": [[3000, 3900]], "M_last": [[3999, 4100]], "M_next": [[4000, 4100]], "M_before": [[2999, 3100]], "M_tail": [[10200, 10400]], "M_zero": [],
           "M_one": [[500, 700]], "M_two": [[1500, 1600], [7200, 7300]], "M_five": [[100, 200], [1100, 1200], [5100, 5200], [8100, 8200], [9100, 9200]]}
    chain = [marker_set("UID1", "k__Bacteria;p__X", 40, [["M_start", "M_last"], ["M_next", "M_before", "M_two"], ["M_two", "M_five", "M_absent"], ["M_tail"], ["M_zero", "M_one"]]),
             marker_set("UID2", "k__Bacteria", 200, [["M_one", "M_two", "M_five"], ["M_start"]]),
             marker_set("UID3", "k__Bacteria", 900, [["M_five"], ["M_one", "M_absent", "M_last"]])]
    refined = [marker_set("UID1", "k__Bacteria;p__X", 40, [["M_start", "M_last"], ["M_two", "M_five"], ["M_one"]])]
    explicit = [([3000], 1000), ([2000, 2000, 3000, 3000, 3000], 1000), ([], 1000), ([0, 1000, 1000, 5000, 9000], 1000), ([2999], 2), ([100, 1100, 7000], 300), ([0], 2**31 - 1)]
    c.append(dict(name="edges", seed=5, genomeId="G1", taxonomy=["Bacteria", "X", "Y"], genomeSize=10500, numReplicates=3, contigLens=[1000, 3000], percentComps=[0.5, 1.0],
                  percentConts=[0.0, 0.2], positions=pos, chain=chain, refined=refined, explicit=explicit))
    # co-located sets of three and of seven markers, 72 of them: the quotients do not sum exactly, and the order of the sum shows
    rng = random.Random(11)
    sizes = [3, 7] * 36
    names = ["pfam%05d" % k for k in range(sum(sizes))]
    pos = {}
    for m in names:
        pos[m] = [[s, s + 600] for s in sorted(rng.randrange(0, 200000) for _ in range(rng.choice([0, 1, 1, 1, 1, 1, 2, 3])))]
    sets, at = [], 0
    for n in sizes:
        sets.append(names[at:at + n]); at += n
    shuffled = names[:]
    rng.shuffle(shuffled)
    other = [shuffled[k:k + 3] for k in range(0, 210, 3)]
    chain = [marker_set("UID10", "k__Bacteria;p__Thirds", 55, sets), marker_set("UID11", "k__Bacteria", 3000, other)]
    refined = [marker_set("UID10", "k__Bacteria;p__Thirds", 55, sets[:65]), marker_set("UID11", "k__Bacteria", 3000, other[:10] + [names[300:307]])]
    c.append(dict(name="thirds_and_sevenths", seed=12, genomeId="G2", taxonomy=["Bacteria", "Thirds"], genomeSize=200000, numReplicates=1, contigLens=[5000], percentComps=[0.7, 0.9],
                  percentConts=[0.0, 0.1], positions=pos, chain=chain, refined=refined, explicit=[([0, 5000, 5000, 100000], 5000)]))
    return c


def scaffold_cases():
    lens = {"s%02d" % k: n for k, n in enumerate([120000, 45000, 45000, 30000, 9000, 5000, 2500, 1200, 800, 500])}
    return [dict(seed=21, targetPer=t, seqLens=lens, genomeSize=sum(lens.values())) for t in (0.1, 0.5, 0.95, 1.0)]


class Stand(object):
    """An object with the attributes it is given: the script's surroundings."""
    def __init__(self, **k):
        self.__dict__.update(k)


class Queue(object):
    def __init__(self, items=()):
        self.items = list(items)

    def get(self, block=True, timeout=None):
        return self.items.pop(0)

    def put(self, item):
        self.items.append(item)


def bin_marker_sets(MarkerSet, BinMarkerSets, binId, sets):
    b = BinMarkerSets(binId, BinMarkerSets.TREE_MARKER_SET)
    for s in sets:
        b.addMarkerSet(MarkerSet(s["UID"], s["lineageStr"], s["numGenomes"], [set(x) for x in s["sets"]]))
    return b


def plain(x):
    """A queue tuple as JSON holds it: dicts for defaultdicts, Python numbers for numpy's."""
    if isinstance(x, dict):
        return {k: plain(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [plain(v) for v in x]
    return x.item() if isinstance(x, np.generic) else x


def run_case(Builder, MarkerSet, BinMarkerSets, source, c):
    d = tempfile.mkdtemp(prefix="ckm_sim_golden_")
    chain, refined = bin_marker_sets(MarkerSet, BinMarkerSets, c["genomeId"], c["chain"]), bin_marker_sets(MarkerSet, BinMarkerSets, c["genomeId"], c["refined"])
    b = object.__new__(Builder)                     # the reference's __init__ reads files of its authors' machine
    b.buildBinMarkerSet = lambda *a, **k: (chain, refined)
    img = Stand(genomeDir=d, geneDistTable=lambda ids, markers, spacingBetweenContigs: {c["genomeId"]: {m: p for m, p in c["positions"].items() if m in markers}})
    sim = Stand(markerSetBuilder=b, img=img, contigLens=c["contigLens"], percentComps=c["percentComps"], percentConts=c["percentConts"])
    redirect = lambda path: os.path.join(d, os.path.basename(path))
    worker, writer = load_worker_and_writer(source, lambda path: c["genomeSize"], lambda path, mode: open(redirect(path), mode),
                                            Stand(open=lambda path, mode: gzip.open(redirect(path), mode)))
    tree = Stand(find_node_with_taxon_label=lambda label: Stand(parent_node=None))
    out = Queue()
    random.seed(c["seed"]); np.random.seed(c["seed"])
    with contextlib.redirect_stdout(io.StringIO()):
        worker(sim, tree, {c["genomeId"]: dict(taxonomy=c["taxonomy"])}, 0.97, 0.97, c["numReplicates"], Queue([c["genomeId"], None]), out)
    tuples = list(out.items)
    recorded = plain(tuples)                          # as they leave the worker: the writer's lookups add keys to the defaultdicts it is handed
    with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        writer(sim, 1, Queue(tuples + [(None,) * 20]))
    summary = open(os.path.join(d, "simulation.summary.testing.tsv")).read()
    replicates = gzip.open(os.path.join(d, "simulation.testing.tsv.gz"), "rt").read()
    # the same draws again, each scored the way the worker scores it
    random.seed(c["seed"]); np.random.seed(c["seed"])
    draws = []
    for contigLen in c["contigLens"]:
        for percentComp in c["percentComps"]:
            for percentCont in c["percentConts"]:
                for _ in range(c["numReplicates"]):
                    trueComp, trueCont, starts = b.sampleGenome(c["genomeSize"], percentComp, percentCont, contigLen)
                    draws.append(dict(contigLen=contigLen, percentComp=percentComp, percentCont=percentCont, trueComp=trueComp, trueCont=trueCont, starts=plain(starts)))
    assert [x["trueComp"] for x in draws] == [v for t in tuples for v in t[8]]
    for starts, contigLen in c["explicit"]:
        draws.append(dict(contigLen=contigLen, starts=starts, explicit=True))
    for x in draws:
        x["contained"], x["checks"] = [], []
        for ms in list(chain.markerSetIter()) + list(refined.markerSetIter()):
            contained = b.containedMarkerGenes(ms.getMarkerGenes(), c["positions"], x["starts"], x["contigLen"])
            x["contained"].append({m: plain(v) for m, v in sorted(contained.items())})
            x["checks"].append([v.hex() for v in ms.genomeCheck(contained, bIndividualMarkers=True) + ms.genomeCheck(contained, bIndividualMarkers=False)])
    return dict(c, draws=draws, tuples=recorded, summary=summary, replicates=replicates)


def run_scaffolds(Builder, c):
    b = object.__new__(Builder)
    out = dict(c)
    np.random.seed(c["seed"])
    ids, per = b.sampleGenomeScaffoldsInvLength(c["targetPer"], c["seqLens"], c["genomeSize"])
    out["inv_length"] = [[str(x) for x in ids], per.hex()]
    ids, per = b.sampleGenomeScaffoldsWithoutReplacement(c["targetPer"], c["seqLens"], c["genomeSize"])
    out["without_replacement"] = [[str(x) for x in ids], per.hex()]
    rng = random.Random(c["seed"])
    pts = [rng.randrange(0, c["genomeSize"]) for _ in range(9)]
    out["uniformity"] = [[pts, b.uniformity(c["genomeSize"], pts).hex()], [[0, 10, 20, 30], b.uniformity(40, [0, 10, 20, 30]).hex()],
                         [[5, 5, 7], b.uniformity(100, [5, 5, 7]).hex()]]
    return out


def main():
    source = os.environ.get("CHECKM_SOURCE", "")
    os.environ["CHECKM_DATA_PATH"] = tempfile.mkdtemp(prefix="ckm_sim_data_")      # the reference's import otherwise creates ~/.checkm
    sys.path.insert(0, source)
    from checkm.markerSets import BinMarkerSets, MarkerSet
    Builder = load_builder(source)
    if "--time" in sys.argv:
        return time_reference(Builder, MarkerSet)
    head = dict(generator="tools/gen_simulation_golden.py: the class of scripts/genometreeworkflow/markerSetBuilder.py, the worker and writer bodies of scripts/simulation.py "
                          "and checkm.markerSets of the reference, the scripts loaded in memory after the substitutions the tool lists",
                substitutions=dict(markerSetBuilder=[s[0] for s in BUILDER_SUBSTITUTIONS], simulation=[s[0] for s in SIMULATION_SUBSTITUTIONS]),
                scaffolds=[run_scaffolds(Builder, c) for c in scaffold_cases()])
    done = [run_case(Builder, MarkerSet, BinMarkerSets, source, c) for c in cases()]
    path = os.path.join(ROOT, "tests", "golden", "simulation_cases.json")
    lines = ",\n".join(json.dumps(c, sort_keys=True, separators=(",", ":")) for c in done)          # a case per line
    open(path, "w").write(json.dumps(head, sort_keys=True)[:-1] + ', "cases": [\n' + lines + "\n]}\n")
    for c in done:
        print(c["name"], len(c["draws"]), "draws", len(c["tuples"]), "tuples", len(c["summary"]), len(c["replicates"]), "bytes of text")
    print(os.path.getsize(path), "bytes")


def time_reference(Builder, MarkerSet):
    from tools.simulation_bench import synth_genome
    arg = lambda name, default: int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
    mb, markers, calls = arg("--mb", 5), arg("--markers", 1500), arg("--calls", 3)
    positions, chain, _refined, genomeSize = synth_genome(mb, markers, 1, seed=18)
    ms = MarkerSet(chain[0].UID, chain[0].lineageStr, chain[0].numGenomes, [set(s) for s in chain[0].markerSet])
    b = object.__new__(Builder)
    random.seed(18); np.random.seed(18)
    wall, starts_seen = 0.0, 0
    for _ in range(calls):
        _c, _t, starts = b.sampleGenome(genomeSize, 1.0, 0.2, 1000)
        t0 = time.perf_counter()
        contained = b.containedMarkerGenes(ms.getMarkerGenes(), positions, starts, 1000)
        ms.genomeCheck(contained, bIndividualMarkers=True)
        ms.genomeCheck(contained, bIndividualMarkers=False)
        wall += time.perf_counter() - t0
        starts_seen += len(starts)
    out = dict(what="reference containedMarkerGenes + both genomeCheck modes (translated in memory), one core, one marker set per call, the synthetic genome of "
                    "tools/simulation_bench.py, 1 kb contigs at completeness 1.0 and contamination 0.2", mb=mb, markers=markers, calls=calls, starts_per_call=starts_seen / calls,
               seconds=wall, seconds_per_replicate_set_check=wall / calls, replicate_set_checks_per_second=calls / wall)
    open(os.path.join(ROOT, "profiles", "r18_simulation_reference_cpu.json"), "w").write(json.dumps(out) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
