#!/usr/bin/env python
"""Goldens of CoverageWindows (`checkm gc_bias_plot`) produced by the REFERENCE's own class (checkm/coverageWindows.py imported
read-only from a CheckM source tree named by CHECKM_SOURCE).  Here only.

pysam is not installed, and the reference as shipped cannot run at all: it imports pysam inside ReadLoader.__init__ only and uses the
name as a global in _processBam.  This script binds both `sys.modules['pysam']` and `checkm.coverageWindows.pysam` to
tests/shim/pysam_legacy.py (a plain-Python BAM reader whose pysam semantics are from memory -- DESIGN section 16, [pysam-ext]).  The
reference runs with threads = 1 and with its multiprocessing replaced by the in-process stand-in of tools/gen_coverage_golden.py, so
that the printed read summary and a worker's exception can be recorded.
Only data is recorded: the cases as record lists, the returned dict with every float as float.hex(), the read summaries, and the
failures by type and arguments.

usage: CHECKM_SOURCE=<checkm source> python tools/gen_covwin_golden.py > tests/golden/covwin_cases.json"""
import contextlib
import io
import json
import logging
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from tests import covwin_reference as wr  # noqa: E402
from tests.shim import pysam_legacy as shim  # noqa: E402
from tools.gen_coverage_golden import InProcess  # noqa: E402

U, DUP, SEC, SUP, QCF, PP = 0x4, 0x400, 0x100, 0x800, 0x200, 0x2


def rec(ref, pos=0, flag=PP | 1, mapq=30, l_seq=100, cigar=None, nm=0, nm_type="C", name="read", tags=None):
    cigar = [["M", l_seq]] if cigar is None else cigar
    tags = ([["NM", nm_type, nm]] if nm is not None else []) if tags is None else tags
    return dict(ref=ref, pos=pos, flag=flag, mapq=mapq, l_seq=l_seq, cigar=cigar, name=name, tags=tags)


def chain_records():
    """Every class, reads of two classes, a supplementary read and a read of mapping quality 0 that end up mapped, a duplicate
    without NM, CIGARs with D, N, I, S, H, = and X, l_seq == 0, reads nowhere."""
    z = ["RG", "Z", "group"]
    return [rec(0, 10, name="a"), rec(0, 20, name="ab", nm=1), rec(0, 30, flag=U | 1, name="abc"),
            rec(0, 40, flag=DUP | PP | 1, name="abcd", nm=None),                                       # duplicate without NM: no error
            rec(0, 50, flag=U | DUP | 1, name="abcde"), rec(0, 60, flag=DUP | SEC | 1, name="abcdef"),  # two classes: the first wins
            rec(0, 70, flag=SEC | PP | 1, name="abcdefg"), rec(0, 80, flag=SUP | PP | 1, name="abcdefgh"),   # supplementary: mapped
            rec(0, 90, flag=QCF | PP | 1, name="abcdefghi"), rec(0, 95, mapq=0), rec(0, 99, mapq=14),   # no mapping-quality test
            rec(0, 100, flag=QCF | 1, mapq=3, cigar=[["S", 90], ["M", 10]], nm=None),                  # QC, short, no NM, unpaired: QC wins
            rec(0, 950, name="over_the_end"),
            rec(1, 5, cigar=[["H", 5], ["S", 10], ["M", 80], ["S", 10], ["H", 5]]),                    # 80 of 100: fails 0.98
            rec(1, 15, cigar=[["H", 5], ["S", 1], ["M", 98], ["S", 1], ["H", 5]]),                     # 98 of 100: passes
            rec(1, 25, cigar=[["S", 1], ["M", 90], ["D", 4], ["I", 8], ["S", 1]]),                     # 94: fails; I does not count
            rec(1, 35, cigar=[["S", 1], ["M", 90], ["D", 9], ["I", 8], ["S", 1]]),                     # 99: passes; D counts
            rec(1, 45, cigar=[["=", 40], ["N", 450], ["X", 2], ["M", 58]], tags=[z, ["NM", "s", 2]]),  # spans windows through N
            rec(1, 300, nm=2), rec(1, 310, nm=3), rec(1, 320, flag=1, nm=3), rec(1, 330, flag=1), rec(1, 340, flag=0),
            rec(1, 400, l_seq=0, cigar=[["S", 5], ["M", 40], ["I", 2], ["=", 3], ["X", 1], ["D", 7], ["S", 4]], nm=0),   # no bases: rlen 0
            rec(1, 410, l_seq=0, cigar=[["M", 50]], nm=1),                                             # 1 > 0.02 * 0
            rec(1, 420, l_seq=0, cigar=[], flag=U | 1, nm=None),
            rec(3, 0, tags=[z, ["XB", "B", ["s", [-3, 2, 9]]], ["NM", "i", 1]], name="t"),
            rec(3, 700, tags=[z, ["NM", "S", 300]], l_seq=250, cigar=[["M", 250]]),
            rec(-1, -1, flag=U | 1, name="nowhere"), rec(-1, -1, flag=U | 1, name="n2", nm=None)]


def mapped(ref, pos, alen, name, cigar=None, l_seq=None):
    return rec(ref, pos, l_seq=alen if l_seq is None else l_seq, cigar=cigar, name=name)


def geometry(w):
    """References of length w, w + 1, 2 w, 2 w + 1 and 6 w + 3 with the same reads on each, as far as they fit: inside one window, ending
    exactly on a boundary, starting on one, crossing one, clipped by L, starting at L; on the long one a read that spans five windows
    and more through an N."""
    refs = [["L_w", w], ["L_w1", w + 1], ["L_2w", 2 * w], ["L_2w1", 2 * w + 1], ["L_long", 6 * w + 3]]
    half = max(1, w // 2)
    out = []
    for k, (_n, L) in enumerate(refs):
        out += [mapped(k, 0, half, "inside"), mapped(k, w - half, half, "ends_on_boundary")]
        if L > w:
            out += [mapped(k, w - 1, 2, "crosses_one"), mapped(k, w, 1, "starts_on_boundary")]
        if k == 4:
            out.append(mapped(k, w // 2, 0, "five_windows", cigar=[["M", 1], ["N", 4 * w], ["M", 1]], l_seq=2))
        out += [mapped(k, L - 1, 3, "clipped_by_L"), mapped(k, L, 4, "starts_at_L"), mapped(k, L + 2, 4, "starts_past_L")]
    return refs, out


def cases():
    refs = [["c1", 1000], ["c2", 2000], ["c_empty", 500], ["c_free", 800]]
    std = dict(bAllReads=False, minAlignPer=0.98, maxEditDistPer=0.02)
    out = [dict(name="chain", file="sample1.bam", refs=refs, records="chain", params=std, windowSize=100),
           dict(name="chain_all_reads", file="sample1.bam", refs=refs, records="chain", params=dict(std, bAllReads=True), windowSize=100),
           dict(name="chain_w333", file="sample1.bam", refs=refs, records="chain", params=std, windowSize=333)]
    assert 0.29 * 100 == 28.999999999999996 and 0.07 * 100 == 7.000000000000001 and 0.57 * 100 == 56.99999999999999 and 0.98 * 150 == 147.0
    clip = lambda n, a: [["S", n - a], ["M", a]]
    out.append(dict(name="ties_029_007", file="t.bam", refs=refs[:2], windowSize=50, params=dict(bAllReads=False, minAlignPer=0.29, maxEditDistPer=0.07), records=[
        rec(0, 10, cigar=clip(100, 29)), rec(0, 20, cigar=clip(100, 28)), rec(1, 30, nm=7), rec(1, 40, nm=8)]))
    out.append(dict(name="ties_098_057", file="t.bam", refs=refs[:2], windowSize=50, params=dict(bAllReads=False, minAlignPer=0.98, maxEditDistPer=0.57), records=[
        rec(0, 10, l_seq=150, cigar=clip(150, 146)), rec(0, 20, l_seq=150, cigar=clip(150, 147)), rec(1, 30, nm=57), rec(1, 40, nm=56)]))
    for w in (1, 7, 5000):
        g_refs, g_recs = geometry(w)
        out.append(dict(name="geometry_w%d" % w, file="g.bam", refs=g_refs, records=g_recs, params=std, windowSize=w))
    out.append(dict(name="alen_zero", file="t.bam", refs=refs[:2], windowSize=100, params=dict(std, minAlignPer=0.0), records=[
        rec(0, 10), rec(0, 150, cigar=[["S", 50], ["I", 50]], name="covers_nothing"), rec(1, 1999, cigar=[["I", 100]])]))
    out.append(dict(name="nm_missing", file="t.bam", refs=refs[:2], windowSize=100, params=std, records=[rec(0), rec(1, 5, name="lacks_nm", tags=[["RG", "Z", "g"]]), rec(1, 9)]))
    out.append(dict(name="no_cigar", file="t.bam", refs=refs[:2], windowSize=100, params=std, records=[rec(0), rec(0, 3, flag=U | 1, cigar=[], name="unmapped_without"),
                                                                                                      rec(1, 5, cigar=[], name="lacks_cigar"), rec(1, 9)]))
    out.append(dict(name="no_reads", file="t.bam", refs=refs[:2], windowSize=100, params=std, records=[]))
    out.append(dict(name="only_unplaced", file="t.bam", refs=refs[:2], windowSize=100, params=std, records=[rec(-1, -1, flag=U | 1)]))
    out.append(dict(name="zero_length_reference", file="t.bam", refs=[["c1", 1000], ["c0", 0]], windowSize=100, params=std, records=[rec(0)]))
    out.append(dict(name="no_index", file="t.bam", refs=refs[:2], windowSize=100, params=std, records=[rec(0)], index=False))
    return out


def run_reference(case):
    import checkm.coverageWindows as ref
    sys.modules["pysam"] = shim          # for the import inside ReadLoader.__init__
    ref.pysam = shim                     # for the global name _processBam and the workers use
    ref.mp = InProcess
    d = tempfile.mkdtemp(prefix="ckm_cw_gold_")
    path = wr.materialise(case, d)
    del InProcess.failures[:]
    buf, err = io.StringIO(), io.StringIO()
    try:
        with contextlib.redirect_stdout(buf), contextlib.redirect_stderr(err):
            info = ref.CoverageWindows(1).run([], path, *(wr.params_of(case) + (case["windowSize"],)))
    except SystemExit as e:
        return dict(error=dict(type="SystemExit", code=e.code))
    if InProcess.failures:
        e = InProcess.failures[0]
        return dict(error=dict(type=type(e).__name__, args=[str(a) for a in e.args]))
    printed = buf.getvalue()
    summary = None
    if "# total reads: 0\n" not in printed:          # (the writer dies there dividing by zero, after it has stored the results)
        summary = printed[:printed.rindex("%)\n") + 3] + "\n"
        assert printed == summary and summary.startswith("\n    # total reads: "), printed
    assert list(info.keys()) == [n for n, _l in case["refs"]]
    return dict(result={k: [float(v[0]).hex(), [float(x).hex() for x in v[1]]] for k, v in info.items()}, summary=summary)


def golden():
    sys.path.insert(0, os.environ.get("CHECKM_SOURCE", ""))
    logging.getLogger("timestamp").setLevel(logging.INFO)
    logging.getLogger("timestamp").addHandler(logging.NullHandler())
    lists = dict(chain=chain_records())
    named = cases()
    cs = [dict(c, records=lists[c["records"]] if isinstance(c["records"], str) else c["records"]) for c in named]
    want = dict(nm_missing="KeyError", no_cigar="TypeError", zero_length_reference="ZeroDivisionError", no_index="SystemExit")
    for c in cs:
        c["expected"] = run_reference(c)
        assert c["expected"].get("error", {}).get("type") == want.get(c["name"]), (c["name"], c["expected"])
        if "result" in c["expected"]:          # the plain restatement must agree before anything is written
            d = tempfile.mkdtemp(prefix="ckm_cw_gold_")
            info, _cnt = wr.run(wr.materialise(c, d), wr.params_of(c), c["windowSize"])
            assert wr.hexed(info) == c["expected"]["result"], c["name"]
    classes = []
    d = tempfile.mkdtemp(prefix="ckm_cw_gold_")
    wr.depth(wr.materialise(cs[0], d), *wr.params_of(cs[0]), classes=classes)
    assert set(classes) == set(range(8)), sorted(set(classes))
    for c, n in zip(cs, named):
        c["records"] = n["records"]
    w = sys.stdout.write
    w('{"generator": "tools/gen_covwin_golden.py", "reference": "checkm/coverageWindows.py", "shim": "tests/shim/pysam_legacy.py",\n')
    w('"record_lists": {\n' + ",\n".join('%s: [\n%s]' % (json.dumps(k), ",\n".join(json.dumps(r) for r in v)) for k, v in lists.items()) + '},\n')
    w('"cases": [\n' + ",\n".join(json.dumps(c) for c in cs) + ']}\n')


if __name__ == "__main__":
    golden()
