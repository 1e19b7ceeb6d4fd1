#!/usr/bin/env python
"""Goldens of `checkm coverage` and `checkm profile` produced by the REFERENCE's own Coverage and Profile (checkm/coverage.py,
checkm/profile.py imported read-only from a CheckM source tree named by CHECKM_SOURCE).  Here only.

pysam is not installed: the reference's Coverage runs on tests/shim/pysam.py (a plain-Python BAM reader whose pysam semantics are from
memory -- DESIGN section 15, [pysam-ext]); this script binds `checkm.coverage.pysam` to it, because the reference imports pysam inside
__init__ and uses the name as a global.  The reference runs with threads = 1 and with its multiprocessing replaced by an in-process
stand-in (queues from `queue`, a Process that runs its target when joined), so that the printed read summary and a worker's exception
can be recorded.  Profile, parseCoverage and binProfiles need no shim: their goldens come straight from the reference.
Only data is recorded: the cases as record lists, the expected file text, read summaries and failures.

usage: CHECKM_SOURCE=<checkm source> python tools/gen_coverage_golden.py > tests/golden/coverage_cases.json"""
import contextlib
import io
import json
import logging
import os
import queue
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DATA = tempfile.mkdtemp(prefix="ckm_data_")          # the reference wants a data root at import time
os.makedirs(os.path.join(DATA, "pfam"))
open(os.path.join(DATA, "pfam", "Pfam-A.hmm.dat"), "w").close()
os.environ["CHECKM_DATA_PATH"] = DATA
sys.dont_write_bytecode = True

from tests import coverage_reference as cr  # noqa: E402
from tests.shim import pysam as shim  # noqa: E402

U, DUP, SEC, SUP, QCF, PP = 0x4, 0x400, 0x100, 0x800, 0x200, 0x2


class InProcess(object):
    """multiprocessing as checkm/coverage.py uses it, in this process."""
    failures = []
    Queue = queue.Queue

    class Process(object):
        def __init__(self, target, args):
            self.target, self.args = target, args

        def start(self):
            pass

        def join(self):
            try:
                self.target(*self.args)
            except Exception as e:
                if self.target.__name__.endswith("workerThread"):      # (the writer's own failure on zero reads is the reference's, and is not ours)
                    InProcess.failures.append(e)
                raise

        def terminate(self):
            pass

    class _Manager(object):
        dict = dict

    @staticmethod
    def Manager():
        return InProcess._Manager()


def rec(ref, flag=PP | 1, mapq=30, l_seq=100, cigar=None, nm=0, nm_type="C", name="read", tags=None):
    cigar = [["M", l_seq]] if cigar is None else cigar
    tags = ([["NM", nm_type, nm]] if nm is not None else []) if tags is None else tags
    return dict(ref=ref, flag=flag, mapq=mapq, l_seq=l_seq, cigar=cigar, name=name, tags=tags)


def chain_records():
    """Every class, reads of two classes, NM in every integer type behind Z / H / B fields, clips, l_seq == 0, names of 1 to 9."""
    z, h, b = ["RG", "Z", "group"], ["XH", "H", "1AE301"], ["XB", "B", ["s", [-3, 2, 9]]]
    out = [rec(0, name="a"), rec(0, name="ab", nm=1), rec(0, flag=U | 1, name="abc"),                  # a placed unmapped read
           rec(0, flag=DUP | PP | 1, name="abcd", nm=None),                                           # duplicate without NM: no error
           rec(0, flag=U | DUP | 1, name="abcde"), rec(0, flag=DUP | SEC | 1, name="abcdef"),           # two classes: the first wins
           rec(0, flag=SEC | PP | 1, name="abcdefg"), rec(0, flag=SUP | PP | 1, name="abcdefgh"),
           rec(0, flag=QCF | PP | 1, name="abcdefghi"), rec(0, mapq=14), rec(0, mapq=15),
           rec(0, flag=QCF | 1, mapq=3, cigar=[["S", 90], ["M", 10]], nm=None),                       # QC, short, no NM, unpaired: QC wins
           rec(1, cigar=[["H", 5], ["S", 10], ["M", 80], ["S", 10], ["H", 5]]),                       # 80 of 100: fails 0.98
           rec(1, cigar=[["H", 5], ["S", 1], ["M", 98], ["S", 1], ["H", 5]]),                         # 98 of 100: passes
           rec(1, cigar=[["S", 1], ["M", 97], ["D", 4], ["I", 1], ["S", 1]]),
           rec(1, nm=2), rec(1, nm=3), rec(1, flag=1, nm=3), rec(1, flag=1), rec(1, flag=0),
           rec(1, l_seq=0, cigar=[["S", 5], ["M", 40], ["I", 2], ["=", 3], ["X", 1], ["S", 4]], nm=0),  # no bases: length from the CIGAR
           rec(1, l_seq=0, cigar=[["M", 50]], nm=1),                                                  # 1 > 0.02 * 0
           rec(1, l_seq=0, cigar=[], flag=U | 1, nm=None)]
    for k, t in enumerate("cCsSiI"):
        out.append(rec(3, nm=k % 3, nm_type=t, name="t" * (k + 1), tags=[z, h, b][:k % 4] + [["AS", "i", -k]] + [["NM", t, k % 3]] + [["XS", "f", 1.5], ["XA", "A", "q"]]))
    out.append(rec(3, tags=[z, ["NM", "s", 300]], l_seq=250, cigar=[["M", 250]]))
    out += [rec(-1, flag=U | 1, name="nowhere"), rec(-1, flag=U | 1, name="n2", nm=None)]
    return out


def record_lists():
    return dict(chain=chain_records(), second=[rec(0, name="x%d" % k, nm=k % 4) for k in range(7)] + [rec(2, l_seq=150, cigar=[["M", 150]], nm=1)])


def cases():
    refs = [["c1", 1000], ["c2", 2000], ["c_empty", 500], ["c_free", 800]]
    bins = [dict(file="bin_a.fna", seqs=[["c2", 1990], ["c1", 1000], ["only_in_bin", 321]]), dict(file="bin_b.fa", seqs=[["c_empty", 500], ["seq_x", 7]])]
    chain, second = "chain", "second"                     # stored once (record_lists), named by the cases
    std = dict(bAllReads=False, minAlignPer=0.98, maxEditDistPer=0.02, minQC=15)
    out = [dict(name="chain", bins=bins, bams=[dict(file="sample1.bam", refs=refs, records=chain)], params=std),
           dict(name="chain_all_reads", bins=bins, bams=[dict(file="sample1.bam", refs=refs, records=chain)], params=dict(std, bAllReads=True)),
           dict(name="two_bams", bins=bins, bams=[dict(file="sample1.bam", refs=refs, records=chain),
                                                  dict(file="other.sorted.bam", refs=[["c1", 1000], ["c_other", 4000], ["c_empty", 512]], records=second)], params=std),
           # the coverage file the qa golden reads: the bin ids of the QA table, one of its two bins without a sequence here
           dict(name="qa_chain", bins=[dict(file="binA.fna", seqs=[["c1", 1000], ["c2", 2000]])],
                bams=[dict(file="sample1.bam", refs=refs, records=chain), dict(file="other.sorted.bam", refs=[["c1", 1000], ["c_other", 4000], ["c_empty", 512]], records=second)], params=std),
           dict(name="no_bins", bins=[], bams=[dict(file="sample1.bam", refs=refs, records=chain)], params=dict(std, minQC=0))]
    assert 0.29 * 100 == 28.999999999999996 and 0.07 * 100 == 7.000000000000001 and 0.57 * 100 == 56.99999999999999 and 0.98 * 150 == 147.0
    clip = lambda n, a: [["S", n - a], ["M", a]]
    out.append(dict(name="ties_029_007", bins=bins[:1], bams=[dict(file="t.bam", refs=refs[:2], records=[
        rec(0, cigar=clip(100, 29)), rec(0, cigar=clip(100, 28)), rec(1, nm=7), rec(1, nm=8)])], params=dict(bAllReads=False, minAlignPer=0.29, maxEditDistPer=0.07, minQC=15)))
    out.append(dict(name="ties_098_057", bins=bins[:1], bams=[dict(file="t.bam", refs=refs[:2], records=[
        rec(0, l_seq=150, cigar=clip(150, 146)), rec(0, l_seq=150, cigar=clip(150, 147)), rec(1, nm=57), rec(1, nm=56)])],
        params=dict(bAllReads=False, minAlignPer=0.98, maxEditDistPer=0.57, minQC=15)))
    out.append(dict(name="nm_missing", bins=bins[:1], bams=[dict(file="t.bam", refs=refs[:2], records=[rec(0), rec(1, name="lacks_nm", tags=[["RG", "Z", "g"]]), rec(1)])], params=std))
    out.append(dict(name="no_reads", bins=bins[:1], bams=[dict(file="t.bam", refs=refs[:2], records=[])], params=std))
    out.append(dict(name="only_unplaced", bins=bins[:1], bams=[dict(file="t.bam", refs=refs[:2], records=[rec(-1, flag=U | 1)])], params=std))
    out.append(dict(name="zero_length_reference", bins=[], bams=[dict(file="t.bam", refs=[["c1", 1000], ["c0", 0]], records=[rec(0)])], params=std))
    out.append(dict(name="no_index", bins=bins[:1], bams=[dict(file="t.bam", refs=refs[:2], records=[rec(0)], index=False)], params=std))
    return out


COVERAGE_FILES = dict(
    one_bam=("Sequence Id\tBin Id\tSequence length (bp)\tBam Id\tCoverage\tMapped reads\n"
             "s1\tbin_a\t1000\tsample1\t12.500000\t130\ns2\tbin_a\t3000\tsample1\t7.250000\t220\ns3\tbin_b\t500\tsample1\t0.000000\t0\n"
             "s4\tunbinned\t700\tsample1\t3.141593\t25\ns5\tbin_c\t1234567\tsample1\t101.100000\t999999\n"),
    three_bams=("Sequence Id\tBin Id\tSequence length (bp)" + "\tBam Id\tCoverage\tMapped reads" * 3 + "\n"
                "s1\tbin_a\t1000\tzeta\t12.500000\t130\talpha\t0.000000\t0\tmid\t1.000000\t10\n"
                "s2\tbin_a\t3000\tzeta\t7.250000\t220\talpha\t0.000000\t0\tmid\t2.000000\t20\n"
                "s2b\tbin_a\t10\tzeta\t0.100000\t1\talpha\t0.000000\t0\tmid\t0.333333\t3\n"
                "s3\tbin_single\t500\tzeta\t9.000000\t45\talpha\t0.000000\t0\tmid\t0.000000\t0\n"
                "s4\tunbinned\t700\tzeta\t3.141593\t25\talpha\t2.000000\t14\tmid\t0.500000\t4\n"),
    no_unbinned=("Sequence Id\tBin Id\tSequence length (bp)\tBam Id\tCoverage\tMapped reads\n"
                 "s1\tb2\t1500\tx\t1.333333\t20\ns2\tb10\t2500\tx\t2.666667\t60\ns3\tb2\t100\tx\t0.010000\t1\n"))


def expand(case, lists):
    """The case with its record lists put in place of their names."""
    return dict(case, bams=[dict(b, records=lists[b["records"]] if isinstance(b["records"], str) else b["records"]) for b in case["bams"]])


def reference_qa(coverage_text):
    """Format 2 of the reference's own ResultsParser.printSummary, tab and framed, with the coverage file: a bin the file holds and one it
    does not.  Only binProfiles runs, which needs no pysam; the import inside Coverage.__init__ gets an empty module."""
    import types
    import checkm.defaultValues
    import checkm.hmmerModelParser
    import checkm.markerSets
    import checkm.resultsParser
    sys.modules["pysam"] = types.ModuleType("pysam")
    ns = types.SimpleNamespace(HmmModel=checkm.hmmerModelParser.HmmModel, MarkerSet=checkm.markerSets.MarkerSet, BinMarkerSets=checkm.markerSets.BinMarkerSets,
                               ResultsManager=checkm.resultsParser.ResultsManager, ResultsParser=checkm.resultsParser.ResultsParser, DefaultValues=checkm.defaultValues.DefaultValues)
    rcase = json.load(open(os.path.join(ROOT, "tests", "golden", "reduce_cases.json")))["cases"][QA_REDUCE_CASE]
    with open(ns.DefaultValues.PFAM_CLAN_FILE, "w") as f:
        f.write(rcase["pfam_dat"])
    work = tempfile.mkdtemp(prefix="ckm_cov_qa_")
    rp, bms = cr.qa_parser(ns, rcase, work)
    cov = os.path.join(work, "coverage.tsv")
    with open(cov, "w") as f:
        f.write(coverage_text)

    class FakeAAI(object):
        aaiMeanBinHetero = {"binA": 12.5}
    out = {}
    for tab in (True, False):
        of = os.path.join(work, "qa_%d.txt" % tab)
        rp.printSummary(2, FakeAAI(), bms, False, cov, tab, of, work)
        out["tab" if tab else "framed"] = open(of).read()
    return dict(reduce_case=QA_REDUCE_CASE, coverage_case="qa_chain", outputs=out)


QA_REDUCE_CASE = 0


def run_coverage(case):
    import checkm.coverage as ref
    sys.modules["pysam"] = shim          # for the import inside Coverage.__init__
    ref.pysam = shim                     # for the global name _processBam and the workers use
    ref.mp = InProcess
    d = tempfile.mkdtemp(prefix="ckm_cov_gold_")
    binFiles, bamFiles, _ = cr.materialise(case, d)
    out = os.path.join(d, "coverage.tsv")
    del InProcess.failures[:]
    buf, err = io.StringIO(), io.StringIO()
    try:
        with contextlib.redirect_stdout(buf), contextlib.redirect_stderr(err):
            ref.Coverage(1).run(binFiles, bamFiles, out, *cr.params_of(case))
    except SystemExit as e:
        return dict(error=dict(type="SystemExit", code=e.code))
    if InProcess.failures:
        e = InProcess.failures[0]
        return dict(error=dict(type=type(e).__name__, args=[str(a) for a in e.args]))
    # the summaries, one per BAM file, as the writer printed them (none where it died on zero reads, after it had stored the results)
    printed = buf.getvalue()
    parts = [("\n    # total reads" + p) for p in printed.split("\n    # total reads")[1:] if not p.startswith(": 0\n")]
    sums, k = [], 0
    for path in bamFiles:
        n = sum(1 for r in shim.Samfile(path)._reads if r.reference_id >= 0)
        if n:
            text = parts[k]; k += 1
            sums.append(text[:text.rindex("%)\n") + 3] + "\n")
        else:
            sums.append(None)
    assert k == len(parts), (k, parts)
    return dict(output=open(out, encoding="utf-8").read(), summaries=sums)


def golden():
    sys.path.insert(0, os.environ.get("CHECKM_SOURCE", ""))
    logging.getLogger("timestamp").setLevel(logging.INFO)
    logging.getLogger("timestamp").addHandler(logging.NullHandler())
    lists = record_lists()
    named = cases()
    cs = [expand(c, lists) for c in named]
    for c in cs:
        c["expected"] = run_coverage(c)
        # the plain restatement must agree before anything is written
        if "output" in c["expected"]:
            d = tempfile.mkdtemp(prefix="ckm_cov_gold_")
            _b, bams, seqs = cr.materialise(c, d)
            text, sums = cr.run(seqs, bams, cr.params_of(c))
            assert text == c["expected"]["output"] and sums == c["expected"]["summaries"], c["name"]
    want = dict(nm_missing="KeyError", zero_length_reference="ZeroDivisionError", no_index="SystemExit")
    for c in cs:
        assert c["expected"].get("error", {}).get("type") == want.get(c["name"]), (c["name"], c["expected"])
    chain = next(c for c in cs if c["name"] == "chain")
    classes = []
    d = tempfile.mkdtemp(prefix="ckm_cov_gold_")
    cr.counters(cr.materialise(chain, d)[1][0], *cr.params_of(chain), classes=classes)
    assert set(classes) == set(range(8)), sorted(set(classes))
    from checkm.coverage import Coverage
    from checkm.profile import Profile
    import types
    sys.modules["pysam"] = types.ModuleType("pysam")          # (nothing below reads a BAM: only the import inside Coverage.__init__ must succeed)
    files = []
    for name, text in COVERAGE_FILES.items():
        d = tempfile.mkdtemp(prefix="ckm_cov_gold_")
        path = os.path.join(d, name + ".tsv")
        with open(path, "w") as f:
            f.write(text)
        cov = Coverage(1)
        g = dict(name=name, text=text, parseCoverage=cov.parseCoverage(path),
                 binProfiles={b: {m: [float(v[0]), float(v[1])] for m, v in p.items()} for b, p in cov.binProfiles(path).items()},
                 binProfiles_order={b: list(p.keys()) for b, p in cov.binProfiles(path).items()})
        for tab in (True, False):
            out = os.path.join(d, "profile_%d.txt" % tab)
            Profile().run(path, out, tab)
            g["profile_tab" if tab else "profile_pretty"] = open(out).read()
        files.append(g)
    # the chain: the reference's Profile and qa table on the coverage file of case qa_chain (straight from the reference, given the file)
    chain_out = next(c for c in cs if c["name"] == "qa_chain")["expected"]["output"]
    d = tempfile.mkdtemp(prefix="ckm_cov_gold_")
    path = os.path.join(d, "qa_chain.tsv")
    with open(path, "w") as f:
        f.write(chain_out)
    qa = reference_qa(chain_out)
    for tab in (True, False):
        out = os.path.join(d, "profile_%d.txt" % tab)
        Profile().run(path, out, tab)
        qa["profile_tab" if tab else "profile_framed"] = open(out).read()
    assert "\t0.00\t0.00\t0.00\t0.00\n" in qa["outputs"]["tab"] and "Coverage std (other.sorted)" in qa["outputs"]["framed"]
    for c, n in zip(cs, named):
        c["bams"] = n["bams"]
    w = sys.stdout.write
    w('{"generator": "tools/gen_coverage_golden.py", "reference": "checkm/coverage.py, checkm/profile.py, checkm/resultsParser.py", "shim": "tests/shim/pysam.py",\n')
    w('"record_lists": {\n' + ",\n".join('%s: [\n%s]' % (json.dumps(k), ",\n".join(json.dumps(r) for r in v)) for k, v in lists.items()) + '},\n')
    w('"cases": [\n' + ",\n".join(json.dumps(c) for c in cs) + '],\n')
    w('"coverage_files": [\n' + ",\n".join(json.dumps(g) for g in files) + '],\n')
    w('"qa": ' + json.dumps(qa) + '}\n')


if __name__ == "__main__":
    golden()
