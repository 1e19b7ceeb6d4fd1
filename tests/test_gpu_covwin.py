"""GPU parity of CoverageWindows (`checkm gc_bias_plot`): CoverageWindows.run against what the reference's own class returned on the
pysam stand-in (tests/golden/covwin_cases.json), and the device pass (ckm_coverage_windows_run: counters, scatter, scan) against the
plain-Python restatement with its per-base depth array (tests/covwin_reference.py) over record counts, run boundaries, slot counts
around the scan's workgroup, record order and batch sizes.  Bar: == on every integer and on every float as float.hex()."""
import numpy as np
import pytest

from checkm_amd import _lib
from synthdata import bam as sbam
from tests import covwin_reference as wr
from tests import test_covwin_host as host

pytestmark = pytest.mark.gpu

GOLD = wr.load_golden()
CASES = {c["name"]: c for c in GOLD["cases"]}
LARGE = dict(nrec=20000, nref=300, seed=11, w=100)


def _case(w):
    return dict(params=dict(bAllReads=False, minAlignPer=0.98, maxEditDistPer=0.02), windowSize=w)


def _device(gpu_ctx, path, w, params=wr.PARAMS, budget=0):
    b = _lib.Bam(path)
    try:
        return _lib.coverage_windows(gpu_ctx, b, *params, w, budget_bytes=budget)
    finally:
        b.close()


@pytest.fixture(scope="module")
def large(tmp_path_factory):
    """The large case, written once: (path, references, records, the restatement's counters, first slots, slot sums, classes, mapped reads)."""
    refs, recs = wr.synthetic(LARGE["nrec"], LARGE["nref"], LARGE["seed"], w=LARGE["w"])
    path = sbam.write_bam(str(tmp_path_factory.mktemp("covwin") / "large.bam"), refs, recs)
    classes, mapped = [], []
    _r, _l, want, cov = wr.depth(path, *wr.PARAMS, classes=classes, mapped=mapped)
    first, sums = wr.slots(cov, LARGE["w"])
    return path, refs, recs, want, first, sums, classes, mapped


@pytest.mark.parametrize("name", sorted(CASES))
def test_coverage_windows_run_matches_reference_goldens(gpu_ctx, name, tmp_path, capsys, caplog):
    from checkm_amd.coverageWindows import CoverageWindows
    case = CASES[name]
    c = host.check_golden_case(CoverageWindows, case, tmp_path, capsys, caplog)
    if c is not None:
        assert all(k in c.last_timing for k in ("ms_inflate", "ms_offsets", "ms_upload", "ms_kernel", "ms_scan", "ms_download", "slots", "s_python"))
        path = str(tmp_path / case["file"])
        got, first, sums, _t = _device(gpu_ctx, path, case["windowSize"], wr.params_of(case))
        host.check_slots(case, path, got, first, sums)


def test_large_case_covers_classes_wavefronts_and_window_geometry(large):
    """The coverage condition, on the restatement alone: every class has at least 1 % of the records; at least 10 % of the wavefronts
    hold two or more references; of the mapped reads at least 10 % cross a window boundary, at least 1 % span three or more windows and
    at least 1 % are clipped by the reference's end."""
    _path, refs, recs, _want, _first, _sums, classes, mapped = large
    share = np.bincount(classes, minlength=8) / float(len(classes))
    assert len(classes) == LARGE["nrec"] and (share >= 0.01).all(), share
    assert wr.waves_with_two_refs(recs) >= 0.10
    cross, three, clipped = wr.geometry(mapped, [n for _n, n in refs], LARGE["w"])
    assert cross >= 0.10 and three >= 0.01 and clipped >= 0.01, (cross, three, clipped)


def test_large_case_under_any_budget_and_twice(gpu_ctx, large):
    """One batch, about twelve, and one batch again on the same context: the same counters and sums (the accumulators are cleared)."""
    path, _refs, recs, want, wfirst, wsums, _c, _m = large
    size = sum(len(sbam.record_bytes(r)) for r in recs)
    for budget, nb in ((0, 1), (size // 12, 12), (0, 1)):
        got, first, sums, t = _device(gpu_ctx, path, LARGE["w"], budget=budget)
        assert (got == want).all() and (first == wfirst).all() and (sums == wsums).all()
        assert t["records"] == LARGE["nrec"] and nb <= t["batches"] <= nb + 2 and t["slots"] == len(wsums)


def test_interleaved_records_give_the_same_sums(gpu_ctx, large, tmp_path):
    _path, _refs, _recs, want, _first, wsums, _c, _m = large
    mixed = sbam.write_bam(str(tmp_path / "mixed.bam"), *wr.synthetic(LARGE["nrec"], LARGE["nref"], LARGE["seed"], w=LARGE["w"], interleave=True))
    got, _f, sums, _t = _device(gpu_ctx, mixed, LARGE["w"])
    assert (got == want).all() and (sums == wsums).all()


@pytest.mark.parametrize("nrec", [1, 63, 64, 65, 129])
def test_small_record_counts(gpu_ctx, nrec, tmp_path):
    refs, recs = wr.synthetic(nrec, min(nrec, 3), seed=nrec)
    path = sbam.write_bam(str(tmp_path / "s.bam"), refs, recs)
    for budget in (0, 1):
        got, first, sums, t = _device(gpu_ctx, path, 100, budget=budget)
        host.check_slots(_case(100), path, got, first, sums)
        assert t["batches"] == (1 if budget == 0 else nrec)


def test_runs_on_wavefront_and_batch_boundaries(gpu_ctx, tmp_path):
    """Runs of equal refID and of equal slot of 64, 65, 63, 1, 128 ... records, in one batch and in batches of 70 records."""
    runs = [64, 65, 63, 1, 128, 1, 190, 2, 62, 300]
    refs, recs = wr.synthetic(sum(runs), len(runs), seed=3, run_lengths=runs)
    for x in recs:                                               # one window per odd reference holds its reads: the slot runs are the refID runs
        if x["ref"] % 2:
            x["pos"] = 200 + x["pos"] % 50
    recs.sort(key=lambda x: (x["ref"], x["pos"]))
    path = sbam.write_bam(str(tmp_path / "runs.bam"), refs, recs)
    for budget in (0, 70 * len(sbam.record_bytes(recs[0]))):
        got, first, sums, _t = _device(gpu_ctx, path, 500, budget=budget)
        assert got[:, 0].tolist() == runs
        host.check_slots(_case(500), path, got, first, sums)


def test_slot_counts_around_the_scan_workgroup(gpu_ctx, tmp_path):
    """Slot counts per reference of 1, 2, 63, 64, 65, SCAN_BLOCK, SCAN_BLOCK + 1 and 2 * SCAN_BLOCK + 1 with zero-window references
    between them; w = 1 on a 300-base reference; and more slots than one tile of the pass over the workgroup totals holds."""
    refs, recs, w, counts = host._blocks_case()
    path = sbam.write_bam(str(tmp_path / "blocks.bam"), refs, recs)
    got, first, sums, _t = _device(gpu_ctx, path, w)
    assert np.diff(first).tolist() == counts
    host.check_slots(_case(w), path, got, first, sums)
    p1 = sbam.write_bam(str(tmp_path / "w1.bam"), [("c300", 300)], [dict(x, ref=0, pos=x["pos"] % 300) for x in recs[:200]])
    got, first, sums, t = _device(gpu_ctx, p1, 1)
    assert t["slots"] == 300
    host.check_slots(_case(1), p1, got, first, sums)
    n = 256 * _lib.COVWIN_SCAN_BLOCK + 2 * _lib.COVWIN_SCAN_BLOCK + 5          # more workgroup totals than one tile of their scan
    far = [dict(x, ref=k % 2, pos=(x["pos"] * 7919 + 1000 * k) % n) for k, x in enumerate(recs[:300])]
    far.sort(key=lambda x: (x["ref"], x["pos"]))
    p2 = sbam.write_bam(str(tmp_path / "tiles.bam"), [("a", n), ("b", n // 3)], far)
    got, first, sums, t = _device(gpu_ctx, p2, 1)
    assert t["slots"] == n + n // 3
    host.check_slots(_case(1), p2, got, first, sums)


def test_error_slot_names_the_first_record(gpu_ctx, tmp_path):
    base = dict(ref=0, pos=5, flag=3, mapq=30, l_seq=50, cigar=[("M", 50)], name="walker")
    ok = dict(base, tags=[("NM", "C", 0)], name="fine")
    path = str(tmp_path / "aux.bam")
    for bad, reason in ((dict(base, tags=[("RG", "Z", "g")], raw_tail=b"XZZabc"), 1), (dict(base, cigar=[], tags=[("NM", "C", 0)]), 5), (dict(base, pos=-1, tags=[("NM", "C", 0)]), 6)):
        sbam.write_bam(path, [("c1", 1000)], [ok] * 70 + [bad, dict(base, tags=[])] + [ok] * 3)
        with pytest.raises(_lib.CoverageRecordError) as e:
            _device(gpu_ctx, path, 100)
        assert (e.value.record, e.value.reason, e.value.read) == (70, reason, "walker") and "aux.bam" in str(e.value)
