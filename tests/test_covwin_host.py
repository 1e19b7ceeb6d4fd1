"""CoverageWindows (`checkm gc_bias_plot`) without a device: the host executor of the device pass (tests/emu/covwin_emu.cpp: the
library's BAM reader, covwin_dev.h, the O(1) scatter into direct / diff and the scan) and the plain-Python restatement with its per-base
depth array (tests/covwin_reference.py) against what the reference's own CoverageWindows returned on the pysam stand-in
(tests/golden/covwin_cases.json).  Bar: == on every integer, and on every float as float.hex()."""
import logging
import os
import subprocess
import sys

import numpy as np
import pytest

from checkm_amd import _lib
from checkm_amd import coverageWindows as cwin
from synthdata import bam as sbam
from tests import covwin_reference as wr
from tests.emu import covwin as emu

GOLD = wr.load_golden()
CASES = {c["name"]: c for c in GOLD["cases"]}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class EmuCoverageWindows(cwin.CoverageWindows):
    """CoverageWindows.run with the device pass replaced by the host executor: everything else is the product's code."""
    budget = 0

    def _pass(self, bamFile, bAllReads, minAlignPer, maxEditDistPer, windowSize):
        bam = _lib.Bam(bamFile)
        names, lengths = bam.references, bam.lengths
        bam.close()
        try:
            out, first, sums, _info = emu.windows(bamFile, bAllReads, minAlignPer, maxEditDistPer, windowSize, budget=self.budget)
        except emu.RecordError as e:
            raise _lib.CoverageRecordError(-1, str(e), e.reason, e.record, e.read)
        return names, lengths, out[:len(names)], first[:len(names) + 1], sums, {}


def check_golden_case(make, case, tmp_path, capsys, caplog, **bgzf):
    """One golden case through `make(threads).run`: the dict, the printed summary, the failures."""
    exp = case["expected"]
    path = wr.materialise(case, str(tmp_path), **bgzf)
    args = ([], path) + wr.params_of(case) + (case["windowSize"],)
    with caplog.at_level(logging.INFO, logger="timestamp"):
        if "error" in exp:
            with pytest.raises(BaseException) as e:
                make(1).run(*args)
            assert type(e.value).__name__ == exp["error"]["type"]
            if exp["error"]["type"] == "SystemExit":
                assert e.value.code == exp["error"]["code"]
                assert "BAM file is not sorted: " + path + "\n" in [r.getMessage() for r in caplog.records if r.levelno >= logging.ERROR]
            else:
                assert str(e.value.args[0]) == exp["error"]["args"][0]
                assert case["name"] != "nm_missing" or "lacks_nm" in e.value.args[1]
                assert case["name"] != "no_cigar" or "lacks_cigar" in e.value.args[1]
            return None
        capsys.readouterr()
        c = make(3)
        info = c.run(*args)
    printed = capsys.readouterr().out
    assert type(info) is dict and list(info.keys()) == [n for n, _l in case["refs"]]
    assert all(type(v[0]) is float and type(v[1]) is list for v in info.values())
    assert wr.hexed(info) == exp["result"]
    assert printed == (exp["summary"] or "")
    if exp["summary"] is None:
        assert any("no read summary" in r.getMessage() for r in caplog.records if r.levelno == logging.WARNING)
    assert "Calculating coverage of windows." in [r.getMessage() for r in caplog.records]
    return c


def check_slots(case, path, got, first, sums):
    """Counters and depth sums against the restatement's per-base array; a reference's numerator is the sum of its slots, tail included."""
    _refs, _lens, want, cov = wr.depth(path, *wr.params_of(case))
    wfirst, wsums = wr.slots(cov, case["windowSize"])
    n = len(want)
    assert (got[:n] == want).all() and (first[:n + 1] == wfirst).all() and len(sums) == len(wsums) and (sums == wsums).all()
    for k in range(n):
        assert int(sums[first[k]:first[k + 1]].sum()) == int(got[k, 8])


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_executor_and_restatement_match_the_reference(name, tmp_path, capsys, caplog):
    case = CASES[name]
    c = check_golden_case(EmuCoverageWindows, case, tmp_path, capsys, caplog, block_bytes=997, empty_every=3)
    path = os.path.join(str(tmp_path), case["file"])
    if c is None:
        if case["expected"]["error"]["type"] in ("KeyError", "TypeError"):
            with pytest.raises(BaseException) as e:
                wr.run(path, wr.params_of(case), case["windowSize"])
            assert type(e.value).__name__ == case["expected"]["error"]["type"]
        return
    assert set(c.last_timing) >= {"s_pass", "s_python", "s_total"}
    info, _cnt = wr.run(path, wr.params_of(case), case["windowSize"])
    assert wr.hexed(info) == case["expected"]["result"]
    for budget in (0, 1, 300):
        got, first, sums, meta = emu.windows(path, *wr.params_of(case), case["windowSize"], budget=budget)
        check_slots(case, path, got, first, sums)
        assert (budget != 0 or meta["batches"] == min(1, meta["records"])) and (budget != 1 or meta["batches"] == meta["records"])


def test_silent_above_info(tmp_path, capsys, caplog):
    case = CASES["chain"]
    path = wr.materialise(case, str(tmp_path))
    with caplog.at_level(logging.WARNING, logger="timestamp"):
        info = EmuCoverageWindows(1).run([], path, *wr.params_of(case), case["windowSize"])
    out = capsys.readouterr()
    assert out.out == "" and out.err == "" and wr.hexed(info) == case["expected"]["result"]


def test_chain_case_holds_every_class_and_the_other_chain_differs(tmp_path):
    from tests import coverage_reference as cr
    classes = []
    path = wr.materialise(CASES["chain"], str(tmp_path))
    _r, _l, want, _cov = wr.depth(path, *wr.PARAMS, classes=classes)
    assert set(classes) == set(range(8))
    assert (cr.counters(path, False, 0.98, 0.02, 15)[2][:, :8] != want[:, :8]).any()          # supplementary, mapq, alen: not the chain of `checkm coverage`


def test_argument_refusals(tmp_path):
    _lib.coverage_windows_check(False, 0.98, 0.02, 5000)
    _lib.coverage_windows_check(True, 0.0, 1.0, 1)
    _lib.coverage_windows_check(True, 0.0, 1.0, 2 ** 31 - 1)
    for bad in ((float("nan"), 0.02, 100), (0.98, float("nan"), 100), (0.98, 0.02, 0), (0.98, 0.02, -3), (0.98, 0.02, 2 ** 31), (0.98, 0.02, 2 ** 70)):
        with pytest.raises(_lib.CkmError) as e:
            _lib.coverage_windows_check(False, *bad)
        assert e.value.code == -1
    path = sbam.write_bam(str(tmp_path / "a.bam"), [("c1", 1000), ("c0", 0), ("c2", 1001), ("c3", 1)], [])
    for w in (0, -1, 2 ** 31):
        with pytest.raises(ValueError):
            emu.windows(path, *wr.PARAMS, w)
        with pytest.raises(ValueError):
            EmuCoverageWindows(1).run([], path, *wr.PARAMS, w)
    with pytest.raises(ValueError):
        EmuCoverageWindows(1).run([], path, *wr.PARAMS, 2.5)
    b = _lib.Bam(path)
    try:
        assert _lib.coverage_windows_layout(b, 100).tolist() == [0, 10, 10, 21, 22] and _lib.coverage_windows_layout(b, 1).tolist() == [0, 1000, 1000, 2001, 2002]
        assert _lib.coverage_windows_layout(b, 1000).tolist() == [0, 1, 1, 3, 4]
        with pytest.raises(_lib.CkmError):
            _lib.coverage_windows_layout(b, 0)
    finally:
        b.close()
    # more than 2^31 - 1 slots in total: refused with a message, by the library and by the executor
    many = sbam.write_bam(str(tmp_path / "many.bam"), [("g%d" % k, 2 ** 31 - 1) for k in range(3)], [])
    b = _lib.Bam(many)
    try:
        assert _lib.coverage_windows_layout(b, 4).tolist()[-1] == 3 * ((2 ** 31 - 2) // 4 + 1)
        with pytest.raises(_lib.CkmError) as e:
            _lib.coverage_windows_layout(b, 1)
        assert "2^31 - 1 windows" in str(e.value) and "many.bam" in str(e.value)
    finally:
        b.close()
    with pytest.raises(emu.Refused):
        emu.windows(many, *wr.PARAMS, 1)


def test_record_errors_name_the_first_record(tmp_path):
    refs = [("c1", 1000)]
    base = dict(ref=0, pos=5, flag=3, mapq=30, l_seq=50, cigar=[("M", 50)], name="walker")
    ok = dict(base, tags=[("NM", "C", 0)], name="fine")
    path = str(tmp_path / "aux.bam")
    for bad, reason in ((dict(base, tags=[("RG", "Z", "g")], raw_tail=b"XZZabc"), 1), (dict(base, tags=[]), 2), (dict(base, tags=[("NM", "f", 1.0)]), 3),
                        (dict(base, tags=[], raw_tail=b"XQ?1"), 4), (dict(base, cigar=[], tags=[("NM", "C", 0)]), 5), (dict(base, pos=-1, tags=[("NM", "C", 0)]), 6)):
        sbam.write_bam(path, refs, [ok] * 70 + [bad, dict(base, tags=[])] + [ok] * 3)
        with pytest.raises(emu.RecordError) as e:
            emu.windows(path, *wr.PARAMS, 100)
        assert (e.value.record, e.value.reason, e.value.read) == (70, reason, "walker")
    # the chain stops before the CIGAR, NM and pos are looked at
    early = [dict(base, flag=0x403, pos=-1, cigar=[], tags=[]), dict(base, flag=0x7, pos=-1, cigar=[], tags=[]), dict(base, flag=0x1, pos=-1, tags=[("NM", "C", 0)])]
    sbam.write_bam(path, refs, [ok] + early)
    got, first, sums, _ = emu.windows(path, *wr.PARAMS, 100)
    assert got[0].tolist() == [4, 1, 0, 0, 0, 0, 1, 1, 50] and sums.tolist() == [50] + [0] * 9


@pytest.mark.parametrize("nrec", [1, 63, 64, 65, 129])
def test_structure_small_counts(nrec, tmp_path):
    refs, recs = wr.synthetic(nrec, min(nrec, 3), seed=nrec)
    path = sbam.write_bam(str(tmp_path / "s.bam"), refs, recs)
    case = dict(params=dict(bAllReads=False, minAlignPer=0.98, maxEditDistPer=0.02), windowSize=100)
    for budget in (0, 1, 2000):
        got, first, sums, _ = emu.windows(path, *wr.PARAMS, 100, budget=budget)
        check_slots(case, path, got, first, sums)


def test_structure_runs_boundaries_and_order(tmp_path):
    """Runs of equal refID and of equal slot that end on a wavefront boundary, one record past it and across a batch boundary; the same
    records interleaved give the same sums with more atomic adds; any batch size gives the same sums."""
    runs = [64, 65, 63, 1, 128, 1, 190, 2, 62, 300]
    refs, recs = wr.synthetic(sum(runs), len(runs), seed=3, run_lengths=runs)
    for x in recs:                                               # one window per reference holds most reads: the slot runs are the refID runs
        if x["ref"] % 2:
            x["pos"] = 200 + x["pos"] % 50
    recs.sort(key=lambda x: (x["ref"], x["pos"]))
    by = [[x for x in recs if x["ref"] == r] for r in range(len(runs))]
    mixed = [lst[k] for k in range(max(runs)) for lst in by if k < len(lst)]
    path, mpath = sbam.write_bam(str(tmp_path / "sorted.bam"), refs, recs), sbam.write_bam(str(tmp_path / "mixed.bam"), refs, mixed)
    case = dict(params=dict(bAllReads=False, minAlignPer=0.98, maxEditDistPer=0.02), windowSize=500)
    one, first, sums1, info1 = emu.windows(path, *wr.PARAMS, 500)
    assert one[:len(runs), 0].tolist() == runs
    check_slots(case, path, one, first, sums1)
    many, _f, sums2, info2 = emu.windows(path, *wr.PARAMS, 500, budget=70 * len(sbam.record_bytes(recs[0])))
    mix, _f, sums3, info3 = emu.windows(mpath, *wr.PARAMS, 500)
    assert (many == one).all() and (mix == one).all() and (sums2 == sums1).all() and (sums3 == sums1).all()
    assert info1["batches"] == 1 and info2["batches"] >= 10 and info3["atomics"] > 3 * info1["atomics"]


def _blocks_case():
    """References whose slot counts are 1, 2, 63, 64, 65, SCAN_BLOCK, SCAN_BLOCK + 1 and 2 * SCAN_BLOCK + 1 at w = 3, zero-window
    references (length 0 and length <= w) between them, and reads that span many windows across the scan's workgroup boundaries."""
    import random
    blk, w = _lib.COVWIN_SCAN_BLOCK, 3
    counts = [1, 0, 2, 63, 1, 64, 0, 65, blk, 1, blk + 1, 0, 2 * blk + 1, 1]
    refs = [("b%02d" % k, 0 if n == 0 else (n - 1) * w + 1 + (k % w if n > 1 else k % w)) for k, n in enumerate(counts)]
    r, recs = random.Random(9), []
    for k, (_n, L) in enumerate(refs):
        for _ in range(0 if L == 0 else 12):
            pos = r.randrange(L)
            span = r.choice((1, 2, w, w + 1, 5 * w, 200 * w, 3000 * w))
            recs.append(dict(ref=k, pos=pos, flag=3, mapq=30, l_seq=2, cigar=[("M", 1), ("N", span), ("M", 1)], name="n", tags=[("NM", "C", 0)]))
    recs.sort(key=lambda x: (x["ref"], x["pos"]))
    return refs, recs, w, counts


def test_scan_across_workgroups_and_zero_window_references(tmp_path):
    refs, recs, w, counts = _blocks_case()
    path = sbam.write_bam(str(tmp_path / "blocks.bam"), refs, recs)
    case = dict(params=dict(bAllReads=False, minAlignPer=0.98, maxEditDistPer=0.02), windowSize=w)
    got, first, sums, info = emu.windows(path, *wr.PARAMS, w)
    assert np.diff(first[:len(refs) + 1]).tolist() == counts
    check_slots(case, path, got, first, sums)
    # w = 1 on a 300-base reference
    one = dict(case, windowSize=1)
    p1 = sbam.write_bam(str(tmp_path / "w1.bam"), [("c300", 300)], [dict(x, ref=0, pos=x["pos"] % 300) for x in recs[:200]])
    got, first, sums, info = emu.windows(p1, *wr.PARAMS, 1)
    assert info["slots"] == 300
    check_slots(one, p1, got, first, sums)


def test_dropin_binds_coverage_windows(tmp_path):
    """dropin.install() in a subprocess with a stand-in `checkm` package (the modules dropin.py touches, each with the top-level classes
    the reference defines): CoverageWindows and CoverageStruct are rebound, ReadLoader stays, no name is added."""
    import json
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_module_classes.json")))["classes"]
    gold = dict(gold, **{"checkm.coverageWindows": ["ReadLoader", "CoverageStruct", "CoverageWindows"]})
    pkg = tmp_path / "stand_in" / "checkm"
    pkg.mkdir(parents=True)
    (pkg / "__init__.py").write_text("")
    for mod, classes in gold.items():
        (pkg / (mod.split(".")[1] + ".py")).write_text("".join("class %s(object):\n    pass\n\n\n" % c for c in classes))
    code = ("import checkm.coverageWindows as w\n"
            "before = sorted(n for n in vars(w) if not n.startswith('_'))\n"
            "old = w.ReadLoader\n"
            "import checkm_amd.dropin as d; d.install()\n"
            "assert sorted(n for n in vars(w) if not n.startswith('_')) == before\n"
            "assert w.CoverageWindows.__module__ == 'checkm_amd.coverageWindows' and w.CoverageStruct.__module__.startswith('checkm_amd.') and w.ReadLoader is old\n"
            "import inspect\n"
            "assert list(inspect.signature(w.CoverageWindows.run).parameters) == ['self', 'binFiles', 'bamFile', 'bAllReads', 'minAlignPer', 'maxEditDistPer', 'windowSize']\n"
            "assert list(inspect.signature(w.CoverageWindows.__init__).parameters) == ['self', 'threads']\n"
            "print('ok')\n")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([str(tmp_path / "stand_in"), ROOT]))
    out = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr
    # a CheckM package without the module keeps what it has
    (pkg / "coverageWindows.py").unlink()
    out = subprocess.run([sys.executable, "-c", "import checkm_amd.dropin as d; d.install(); print('ok')"], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr
