"""GPU parity of `checkm coverage`: Coverage.run against the files the reference's own Coverage wrote on the pysam shim
(tests/golden/coverage_cases.json), and the device pass (ckm_coverage_run) against the plain-Python restatement
(tests/coverage_reference.py) over record counts, run boundaries, record order and batch sizes.
Bar: == on every counter and on the file bytes."""
import hashlib
import json
import logging
import os

import numpy as np
import pytest

from checkm_amd import _lib
from synthdata import bam as sbam
from tests import coverage_reference as cr

pytestmark = pytest.mark.gpu

GOLD = cr.load_golden()
CASES = {c["name"]: c for c in GOLD["cases"]}
LARGE = dict(nrec=20000, nref=300, seed=11)


@pytest.fixture(scope="module")
def large(tmp_path_factory):
    """The large case, written once: (path, references, records, the restatement's counters, the class of every record)."""
    refs, recs = cr.synthetic(LARGE["nrec"], LARGE["nref"], LARGE["seed"])
    path = str(tmp_path_factory.mktemp("cov") / "large.bam")
    sbam.write_bam(path, refs, recs)
    classes = []
    _r, _l, want = cr.counters(path, *cr.PARAMS, classes=classes)
    return path, refs, recs, want, classes


def _device(gpu_ctx, path, params=cr.PARAMS, budget=0):
    b = _lib.Bam(path)
    try:
        return _lib.coverage_counters(gpu_ctx, b, *params, budget_bytes=budget)
    finally:
        b.close()


@pytest.mark.parametrize("name", sorted(CASES))
def test_coverage_run_matches_reference_goldens(gpu_ctx, name, tmp_path, capsys, caplog):
    from checkm_amd.coverage import Coverage
    case, exp = CASES[name], CASES[name]["expected"]
    binFiles, bamFiles, _ = cr.materialise(case, str(tmp_path))
    out = str(tmp_path / "coverage.tsv")
    with caplog.at_level(logging.INFO, logger="timestamp"):
        if "error" in exp:
            with pytest.raises(BaseException) as e:
                Coverage(1).run(binFiles, bamFiles, out, *cr.params_of(case))
            assert type(e.value).__name__ == exp["error"]["type"]
            if exp["error"]["type"] == "SystemExit":
                assert e.value.code == exp["error"]["code"]
                assert "BAM file is either unsorted or not indexed: " + bamFiles[0] + "\n" in [r.getMessage() for r in caplog.records if r.levelno >= logging.ERROR]
            else:
                assert str(e.value.args[0]) == exp["error"]["args"][0]
                assert name != "nm_missing" or "lacks_nm" in e.value.args[1]
            return
        capsys.readouterr()
        c = Coverage(2)
        c.run(binFiles, bamFiles, out, *cr.params_of(case))
    assert open(out, encoding="utf-8").read() == exp["output"]
    assert capsys.readouterr().out == "".join(s for s in exp["summaries"] if s)
    assert all(k in c.last_timing for k in ("s_bins", "ms_inflate", "ms_offsets", "ms_upload", "ms_kernel", "ms_download", "s_write"))
    for path in bamFiles:
        _r, _l, want = cr.counters(path, *cr.params_of(case))
        got, _t = _device(gpu_ctx, path, cr.params_of(case))
        assert (got == want).all()


def test_large_case_covers_the_classes_and_mixed_wavefronts(large):
    """The coverage condition, on the restatement alone: every class has at least 1 % of the records, at least 10 % of the wavefronts hold
    two or more references."""
    _path, _refs, recs, _want, classes = large
    share = np.bincount(classes, minlength=8) / float(len(classes))
    assert len(classes) == LARGE["nrec"] and (share >= 0.01).all(), share
    assert cr.waves_with_two_refs(recs) >= 0.10


def _sha(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def test_batch_size_and_repeats_do_not_change_the_file(gpu_ctx, tmp_path, capsys):
    """Coverage.run on 40 000 records (13 MB inflated) with CKM_COVERAGE_BATCH_MB unset (one batch) and set to 1 (a dozen), and twice in
    a row: the same SHA-256 of the coverage file, which is the restatement's text."""
    from checkm_amd.coverage import Coverage
    refs, recs = cr.synthetic(40000, 300, seed=12)
    path = str(tmp_path / "batches.bam")
    sbam.write_bam(path, refs, recs)
    fa = str(tmp_path / "bin_1.fna")
    with open(fa, "w") as f:
        for name, n in refs[:100]:
            f.write(">%s\n%s\n" % (name, "ACGT" * (n // 4)))
    want, _sums = cr.run([(fa, [(name, n // 4 * 4) for name, n in refs[:100]])], [path], cr.PARAMS)
    digests, batches = [], []
    old = os.environ.pop("CKM_COVERAGE_BATCH_MB", None)
    try:
        for k, mb in enumerate((None, "1", None)):
            if mb is not None:
                os.environ["CKM_COVERAGE_BATCH_MB"] = mb
            out = str(tmp_path / ("coverage_%d.tsv" % k))
            c = Coverage(1)
            c.run([fa], [path], out, *cr.PARAMS)
            os.environ.pop("CKM_COVERAGE_BATCH_MB", None)
            t = c.last_timing
            print("coverage %d records, CKM_COVERAGE_BATCH_MB=%s: %d batches, inflate %.3f ms, offsets %.3f ms, upload %.3f ms, kernel %.3f ms, download %.3f ms" %
                  (t["records"], mb, t["batches"], t["ms_inflate"], t["ms_offsets"], t["ms_upload"], t["ms_kernel"], t["ms_download"]))
            digests.append(_sha(out)); batches.append(int(t["batches"]))
    finally:
        if old is not None:
            os.environ["CKM_COVERAGE_BATCH_MB"] = old
    assert batches[0] == 1 and batches[2] == 1 and 12 <= batches[1] <= 14, batches
    assert len(set(digests)) == 1 and digests[0] == hashlib.sha256(want.encode()).hexdigest()


def test_large_case_counters_under_any_budget(gpu_ctx, large):
    path, _refs, recs, want, _classes = large
    size = sum(len(sbam.record_bytes(r)) for r in recs)
    for budget, nb in ((0, 1), (size // 12, 12)):
        got, t = _device(gpu_ctx, path, budget=budget)
        assert (got == want).all() and t["records"] == LARGE["nrec"] and nb <= t["batches"] <= nb + 2


def test_interleaved_records_give_the_same_counters(gpu_ctx, large, tmp_path):
    _path, _refs, _recs, want, _classes = large
    mixed = str(tmp_path / "mixed.bam")
    sbam.write_bam(mixed, *cr.synthetic(LARGE["nrec"], LARGE["nref"], LARGE["seed"], interleave=True))
    got, _t = _device(gpu_ctx, mixed)
    assert (got == want).all()


@pytest.mark.parametrize("nrec", [1, 63, 64, 65, 129])
def test_small_record_counts(gpu_ctx, nrec, tmp_path):
    refs, recs = cr.synthetic(nrec, min(nrec, 3), seed=nrec)
    path = str(tmp_path / "s.bam")
    sbam.write_bam(path, refs, recs)
    _r, _l, want = cr.counters(path, *cr.PARAMS)
    for budget in (0, 1):
        got, t = _device(gpu_ctx, path, budget=budget)
        assert (got == want).all() and t["batches"] == (1 if budget == 0 else nrec)


def test_runs_on_wavefront_and_batch_boundaries(gpu_ctx, tmp_path):
    runs = [64, 65, 63, 1, 128, 1, 190, 2, 62, 300]
    refs, recs = cr.synthetic(sum(runs), len(runs), seed=3, run_lengths=runs)
    path = str(tmp_path / "runs.bam")
    sbam.write_bam(path, refs, recs)
    _r, _l, want = cr.counters(path, *cr.PARAMS)
    assert want[:, 0].tolist() == runs
    for budget in (0, 70 * len(sbam.record_bytes(recs[0]))):
        got, _t = _device(gpu_ctx, path, budget=budget)
        assert (got == want).all()


def test_error_slot_names_the_first_record(gpu_ctx, tmp_path):
    base = dict(ref=0, flag=3, mapq=30, l_seq=50, cigar=[("M", 50)], name="walker")
    ok = dict(base, tags=[("NM", "C", 0)], name="fine")
    path = str(tmp_path / "aux.bam")
    sbam.write_bam(path, [("c1", 1000)], [ok] * 70 + [dict(base, tags=[("RG", "Z", "g")], raw_tail=b"XZZabc"), dict(base, tags=[])] + [ok] * 3)
    with pytest.raises(_lib.CoverageRecordError) as e:
        _device(gpu_ctx, path)
    assert (e.value.record, e.value.reason, e.value.read) == (70, 1, "walker") and "aux.bam" in str(e.value)


def test_record_refusal_through_the_library(gpu_ctx, tmp_path):
    import struct
    good = dict(ref=0, flag=3, mapq=30, l_seq=50, cigar=[("M", 50)], name="ok", tags=[("NM", "C", 0)])
    bad = bytearray(sbam.record_bytes(good)); bad[4:8] = struct.pack("<i", 7)
    path = str(tmp_path / "refid.bam")
    with open(path, "wb") as f:
        f.write(sbam.bgzf(sbam.header_bytes([("c1", 1000)]) + sbam.record_bytes(good) * 3 + bytes(bad)))
    with pytest.raises(_lib.CkmError) as e:
        _device(gpu_ctx, path)
    assert e.value.code == -1 and "refid.bam: record 3: refID 7 out of range" in str(e.value)


def test_coverage_then_profile_and_qa(gpu_ctx, tmp_path):
    """The chain on synthetic bins and BAM files: Coverage.run writes the coverage file of case qa_chain; Profile.run on that file and
    ResultsParser.printSummary (format 2, tab and framed) with that file print what the reference's own Profile and ResultsParser printed
    for it: a bin the file holds (binA) and one it does not (binB: 0 / 0), two BAM columns."""
    import types
    from checkm_amd import defaultValues, hmmerModelParser, markerSets, resultsParser
    from checkm_amd.coverage import Coverage
    from checkm_amd.profile import Profile
    qa, case = GOLD["qa"], CASES[GOLD["qa"]["coverage_case"]]
    d = tmp_path / "chain"
    d.mkdir()
    binFiles, bamFiles, _ = cr.materialise(case, str(d))
    cov = str(tmp_path / "coverage.tsv")
    Coverage(1).run(binFiles, bamFiles, cov, *cr.params_of(case))
    assert open(cov).read() == case["expected"]["output"]
    for tab, key in ((True, "profile_tab"), (False, "profile_framed")):
        out = str(tmp_path / key)
        Profile().run(cov, out, tab)
        assert open(out).read() == qa[key]
    rcase = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reduce_cases.json")))["cases"][qa["reduce_case"]]
    root = tmp_path / "data"
    (root / "pfam").mkdir(parents=True)
    defaultValues.DefaultValues.set_data_root(str(root))
    (root / "pfam" / "Pfam-A.hmm.dat").write_text(rcase["pfam_dat"])
    ns = types.SimpleNamespace(HmmModel=hmmerModelParser.HmmModel, MarkerSet=markerSets.MarkerSet, BinMarkerSets=markerSets.BinMarkerSets,
                               ResultsManager=resultsParser.ResultsManager, ResultsParser=resultsParser.ResultsParser, DefaultValues=defaultValues.DefaultValues)
    work = tmp_path / "qa"
    work.mkdir()
    rp, bms = cr.qa_parser(ns, rcase, str(work))

    class FakeAAI(object):
        aaiMeanBinHetero = {"binA": 12.5}
    for tab, key in ((True, "tab"), (False, "framed")):
        of = str(work / ("qa_%s.txt" % key))
        rp.printSummary(2, FakeAAI(), bms, False, cov, tab, of, str(work))
        assert open(of).read() == qa["outputs"][key], key
