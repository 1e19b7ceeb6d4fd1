#!/usr/bin/env python
"""Goldens of AminoAcidIdentity: the reference's own checkm.aminoAcidIdentity.AminoAcidIdentity().run over small hand-made output
directories.  Per case the files of the directory, aaiRawScores, aaiHetero, aaiMeanBinHetero, the alignment report as it lies after the
call, the records of the 'timestamp' logger and a failure by type and message.  os.listdir is made to return sorted names while the
reference runs (the tests do the same), so that the traversal does not depend on the file system.  Runs only where a CheckM source
tree is at hand; the tests read the JSON.
usage: CHECKM_SOURCE=<checkm source> python tools/gen_aai_golden.py                         (writes tests/golden/aai_cases.json)
       CHECKM_SOURCE=<checkm source> python tools/gen_aai_golden.py --time --bins N --copies K [--markers M] [--big B]
                                      (times the reference's run on one core over the tree of tools/aai_bench.py, writes
                                       profiles/r16_aai_reference_cpu.json)"""
import json
import logging
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

Q = "storage/aai_qa/"


def case(name, bins, files, threshold=0.9, report=True):
    return dict(name=name, bins=bins, files=files, threshold=threshold, report=report)


def fa(*recs):
    return "".join(">%s\n%s\n" % r for r in recs)


def cases():
    c = []
    c.append(case("empty_tree", [], {}))
    # a bin without a folder, a bin folder without a .masked.faa, a file with one sequence
    c.append(case("nothing_to_compare", ["b0", "b1", "b2"], {Q + "b1/notes.txt": "x\n", Q + "b1/PF1.faa": fa(("b1&&g1", "AC"), ("b1&&g2", "AC")),
                                                             Q + "b2/PF00001.1.masked.faa": fa(("b2&&g1 [e-value=1e-5,score=10.0]", "ACDEF"))}))
    # three copies, gap runs at both ends, a both-gap column and a residue against a gap inside, stats behind the ids, a blank line; two bins
    c.append(case("basic", ["b1", "b2"], {
        Q + "b1/PF00318.15.masked.faa": fa(("b1&&g1 [e-value=1e-30,score=99.1]", "--ACDEFGHIK-LMN--"), ("b1&&g2 [e-value=1e-20,score=80.0]", "-MACDEF-HIK-LMNP-"), ("b1&&g3", "---CDEWGHIKALMN-Q")),
        Q + "b1/TIGR00001.masked.faa": fa(("b1&&g7", "MKV"), ("b1&&g8", "MKV")) + "\n",
        Q + "b2/PF00318.15.masked.faa": fa(("b2&&h1", "ACDEFGHIKL"), ("b2&&h2", "ACDEFGHIKV"))}, threshold=0.8))
    # the scan for the end never looks at column 0; rows without a compared column; rows of one column and of none
    c.append(case("column_zero", ["b1"], {
        Q + "b1/A.masked.faa": fa(("b1&&g1", "A----"), ("b1&&g2", "A----"), ("b1&&g3", "C----")),
        Q + "b1/B.masked.faa": fa(("b1&&g1", "-ACD"), ("b1&&g2", "-ACD"), ("b1&&g3", "----")),
        Q + "b1/C.masked.faa": fa(("b1&&g1", "-"), ("b1&&g2", "A"), ("b1&&g3", "A")),
        Q + "b1/D.masked.faa": fa(("b1&&g1", ""), ("b1&&g2", "")),
        Q + "b1/E.masked.faa": fa(("b1&&g1", "-----"), ("b1&&g2", "-----")),
        Q + "b1/F.masked.faa": fa(("b1&&g1", "-C---"), ("b1&&g2", "AC---"), ("b1&&g3", "A-C--"))}, threshold=0.5))
    # a repeated id keeps its place and takes the later record; an id without '&&' is cut one character short (find() == -1)
    c.append(case("ids", ["b1", "solo"], {
        Q + "b1/PF1.masked.faa": fa(("b1&&g1", "ACDEF"), ("b1&&g2", "ACDEW"), ("b1&&g1", "AC-EW"), ("b1&&g3", "WWWWW")),
        Q + "solo/PF2.masked.faa": fa(("solox", "ACDEF"), ("soloy", "ACDEF"), ("soloz", "ACDQF"))}))
    # marker names with two dots fall on one marker; lower case differs from upper case; a sequence on two lines
    c.append(case("names_and_case", ["b1"], {
        Q + "b1/PF00318.15.masked.faa": fa(("b1&&g1", "ACDEF"), ("b1&&g2", "ACDEF")),
        Q + "b1/PF00318.2.masked.faa": fa(("b1&&g3", "acdef"), ("b1&&g4", "ACDEF"), ("b1&&g5", "ACdEF")),
        Q + "b1/TIGR1.x.y.masked.faa": ">b1&&g6\nACD\nEFG\n>b1&&g7\nACDEFG\n"}, threshold=0.95))
    # rows of unequal length in the second of three groups: the assertion, after the report of the first group and of one pair
    c.append(case("unequal", ["b1", "b2"], {
        Q + "b1/A.masked.faa": fa(("b1&&g1", "ACDEF"), ("b1&&g2", "ACDEW")),
        Q + "b1/B.masked.faa": fa(("b1&&g1", "ACDEF"), ("b1&&g2", "ACDEF"), ("b1&&g3", "ACDE")),
        Q + "b2/A.masked.faa": fa(("b2&&g1", "ACDEF"), ("b2&&g2", "ACDEF"))}))
    # owners that differ: the log line and the exit, after the pairs in front
    c.append(case("owners", ["b1", "b2"], {
        Q + "b1/A.masked.faa": fa(("b1&&g1", "ACDEF"), ("b1&&g2", "AC-EW")),
        Q + "b1/B.masked.faa": fa(("b1&&g1", "ACDEF"), ("b1&&g2", "ACDEF"), ("b9&&g3", "ACDEF")),
        Q + "b2/A.masked.faa": fa(("b2&&g1", "ACDEF"), ("b2&&g2", "ACDEF"))}))
    # a non-ASCII row between two plain groups; no report
    c.append(case("non_ascii", ["b1"], {
        Q + "b1/A.masked.faa": fa(("b1&&g1", "ACDEF"), ("b1&&g2", "ACDEW")),
        Q + "b1/B.masked.faa": fa(("b1&&g1", "ACDéF"), ("b1&&g2", "ACDEF"), ("b1&&g3", "ACDéF")),
        Q + "b1/C.masked.faa": fa(("b1&&g1", "-CDEF"), ("b1&&g2", "ACDE-"))}))
    c.append(case("no_report", ["b1"], {Q + "b1/A.masked.faa": fa(("b1&&g1", "ACDEF"), ("b1&&g2", "ACDEW"), ("b1&&g3", "ACWEW"))}, report=False))
    return c


def write_tree(d, c):
    """The output directory of a case under d."""
    os.makedirs(os.path.join(d, "bins"))
    for b in c["bins"]:
        os.makedirs(os.path.join(d, "bins", b))
    for rel, text in c["files"].items():
        p = os.path.join(d, *rel.split("/"))
        os.makedirs(os.path.dirname(p), exist_ok=True)
        open(p, "wb").write(text.encode("utf-8"))
    return d


class Records(logging.Handler):
    def __init__(self):
        logging.Handler.__init__(self)
        self.out = []

    def emit(self, record):
        self.out.append([record.levelname, record.getMessage()])


def run_case(AminoAcidIdentity, c):
    d = write_tree(tempfile.mkdtemp(prefix="ckm_aai_golden_"), c)
    path = os.path.join(d, "alignments.txt") if c["report"] else None
    logger, h = logging.getLogger("timestamp"), Records()
    logger.addHandler(h)
    logger.setLevel(logging.INFO)
    listdir, error = os.listdir, None
    os.listdir = lambda p: sorted(listdir(p))
    a = AminoAcidIdentity()
    try:
        a.run(c["threshold"], d, path)
    except (Exception, SystemExit) as e:
        error = dict(type=type(e).__name__, message=str(e))
        del e
    finally:
        os.listdir = listdir
        logger.removeHandler(h)
    import gc
    gc.collect()                                                 # the failed call's frame is gone: its report is closed as at interpreter exit
    plain = lambda x: {k: (plain(v) if isinstance(v, dict) else v) for k, v in x.items()}
    return dict(c, raw=plain(a.aaiRawScores), hetero=plain(a.aaiHetero), mean=plain(a.aaiMeanBinHetero),
                report_text=open(path, "rb").read().decode("utf-8") if path and os.path.exists(path) else None, log=h.out, error=error)


def main():
    sys.path.insert(0, os.environ.get("CHECKM_SOURCE", ""))
    from checkm.aminoAcidIdentity import AminoAcidIdentity
    if "--time" in sys.argv:
        return time_reference(AminoAcidIdentity)
    out = dict(generator="tools/gen_aai_golden.py: checkm.aminoAcidIdentity.AminoAcidIdentity().run of the reference, os.listdir returning sorted names",
               cases=[run_case(AminoAcidIdentity, c) for c in cases()])
    open(os.path.join(ROOT, "tests", "golden", "aai_cases.json"), "w").write(json.dumps(out, indent=1, sort_keys=True) + "\n")
    for c in out["cases"]:
        print(c["name"], c["error"], sum(len(v) for m in c["raw"].values() for v in m.values()), len(c["log"]))


def time_reference(AminoAcidIdentity):
    from tools.aai_bench import synth_tree
    arg = lambda name, default: int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
    bins, copies, markers, big = arg("--bins", 64), arg("--copies", 12), arg("--markers", 20), arg("--big", 300)
    d = synth_tree(tempfile.mkdtemp(prefix="ckm_aai_time_"), bins, markers, copies, big)
    a = AminoAcidIdentity()
    t0 = time.perf_counter()
    a.run(0.9, d, os.path.join(d, "alignments.txt"))
    wall = time.perf_counter() - t0
    pairs = sum(len(v) for m in a.aaiRawScores.values() for v in m.values())
    out = dict(what="reference AminoAcidIdentity.run, one core, the tree of tools/aai_bench.py, with the alignment report", bins=bins, markers=markers, copies=copies,
               big=big, pairs=pairs, seconds=wall)
    open(os.path.join(ROOT, "profiles", "r16_aai_reference_cpu.json"), "w").write(json.dumps(out) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
