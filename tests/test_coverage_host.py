"""`checkm coverage` / `checkm profile` without a device: the host executor of the device pass (tests/emu/coverage_emu.cpp: the library's
BAM reader plus coverage_dev.h) and the plain-Python restatement against the files the reference's own Coverage wrote on the pysam shim
(tests/golden/coverage_cases.json); the library's reader against the shim's reader; Profile, parseCoverage and binProfiles against the
reference's own output, byte for byte."""
import os
import struct

import numpy as np
import pytest

from checkm_amd import _lib
from checkm_amd import coverage as cov
from checkm_amd.profile import Profile
from synthdata import bam as sbam
from tests import coverage_reference as cr
from tests.emu import coverage as emu
from tests.shim import pysam as shim

GOLD = cr.load_golden()
CASES = {c["name"]: c for c in GOLD["cases"]}


class EmuCoverage(cov.Coverage):
    """Coverage.run with the device pass replaced by the host executor: everything else is the product's code."""
    budget = 0

    def _counters(self, bamFile, bAllReads, minAlignPer, maxEditDistPer, minQC):
        names, lengths, _off, _nb, _hb = emu.scan(bamFile)
        try:
            out, info = emu.counters(bamFile, bAllReads, minAlignPer, maxEditDistPer, minQC, budget=self.budget)
        except emu.RecordError as e:
            if e.reason == 2:
                raise KeyError("tag 'NM' not present", e.read)
            raise
        return names, lengths, out[:len(names)], {}


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_executor_and_restatement_match_the_reference(name, tmp_path, capsys, caplog):
    case = CASES[name]
    exp = case["expected"]
    binFiles, bamFiles, binSeqs = cr.materialise(case, str(tmp_path), block_bytes=997, empty_every=3)
    out = str(tmp_path / "coverage.tsv")
    import logging
    with caplog.at_level(logging.INFO, logger="timestamp"):
        if "error" in exp:
            with pytest.raises(BaseException) as e:
                EmuCoverage(1).run(binFiles, bamFiles, out, *cr.params_of(case))
            assert type(e.value).__name__ == exp["error"]["type"]
            if exp["error"]["type"] == "SystemExit":
                assert e.value.code == exp["error"]["code"] and "BAM file is either unsorted or not indexed: " + bamFiles[0] + "\n" in [r.getMessage() for r in caplog.records]
            else:
                assert str(e.value.args[0]) == exp["error"]["args"][0]
                if name == "nm_missing":
                    assert "lacks_nm" in e.value.args[1]
                    with pytest.raises(KeyError):
                        cr.run(binSeqs, bamFiles, cr.params_of(case))
            return
        capsys.readouterr()
        EmuCoverage(3).run(binFiles, bamFiles, out, *cr.params_of(case))
    printed = capsys.readouterr().out
    assert open(out, encoding="utf-8").read() == exp["output"]
    assert printed == "".join(s for s in exp["summaries"] if s)
    if None in exp["summaries"]:
        assert any("no read summary" in r.getMessage() for r in caplog.records if r.levelno == logging.WARNING)
    msgs = [r.getMessage() for r in caplog.records]
    assert msgs[0] == "Determining bin assignment of each sequence." and msgs[1] == "Processing %d file(s) with 3 threads.\n" % len(bamFiles)
    assert "Processing %s (1 of %d):" % (os.path.basename(bamFiles[0]), len(bamFiles)) in msgs and msgs[-1] == "Writing coverage information to file."
    # the restatement, and the counters themselves
    text, sums = cr.run(binSeqs, bamFiles, cr.params_of(case))
    assert text == exp["output"] and sums == exp["summaries"]
    for path in bamFiles:
        refs, lens, want = cr.counters(path, *cr.params_of(case))
        for budget in (0, 1, 300):
            got, info = emu.counters(path, *cr.params_of(case), budget=budget)
            assert (got[:len(refs)] == want).all() and not got[len(refs):].any(), (name, budget)
            assert (budget != 0 or info["batches"] == min(1, info["records"])) and (budget != 1 or info["batches"] == info["records"])


def test_chain_case_holds_every_class():
    import tempfile
    classes = []
    d = tempfile.mkdtemp()
    cr.counters(cr.materialise(CASES["chain"], d)[1][0], *cr.params_of(CASES["chain"]), classes=classes)
    assert set(classes) == set(range(8))


def _big(tmp_path, **kw):
    refs, recs = cr.synthetic(3000, 40, seed=5)
    path = str(tmp_path / "big.bam")
    sbam.write_bam(path, refs, recs, **kw)
    return path, refs, recs


def test_library_reader_against_the_shim(tmp_path):
    """Header, record count and offsets: a record spanning two BGZF blocks (blocks of 100 bytes: every record does), empty blocks, the EOF
    block present and absent, batches of 64 KB and of one record; the header through the library (ckm_bam_open), the records through the
    same reader inside the host executor."""
    for kw in (dict(block_bytes=100, empty_every=2), dict(block_bytes=0xff00), dict(block_bytes=4096, eof=False)):
        path, refs, recs = _big(tmp_path, **kw)
        f = shim.Samfile(path)
        want = np.array([r.offset for r in f._reads], dtype=np.uint64)
        assert len(want) == len(recs)
        for budget, nb in ((0, 1), (1 << 16, None), (1, len(recs))):
            b = _lib.Bam(path)
            assert b.references == list(f.references) == [n for n, _ in refs] and b.lengths == list(f.lengths) and b.header_bytes == f.header_bytes
            b.close()
            names, lengths, off, batches, hb = emu.scan(path, budget)
            assert names == list(f.references) and lengths == list(f.lengths) and (off == want).all() and hb == f.header_bytes
            assert (nb is None or batches == nb) and (budget != 1 << 16 or batches > 3)


def _refusal(path, header=False):
    """The reader's message; a refusal in the first blocks or the header must come from ckm_bam_open too, with CKM_EINVAL."""
    with pytest.raises(emu.Refused) as e:
        emu.counters(path, *cr.PARAMS)
    assert os.path.basename(path) in str(e.value)
    if header:
        with pytest.raises(_lib.CkmError) as le:
            _lib.Bam(path)
        assert le.value.code == -1 and str(e.value) in str(le.value)
    else:
        _lib.Bam(path).close()
    return str(e.value)


def test_library_reader_refusals(tmp_path):
    refs = [("c1", 1000), ("c2", 500)]
    good = [dict(ref=0, flag=3, mapq=30, l_seq=50, cigar=[("M", 50)], name="ok", tags=[("NM", "C", 0)]) for _ in range(5)]
    head, body = sbam.header_bytes(refs), [sbam.record_bytes(r) for r in good]

    def write(name, data, **kw):
        p = str(tmp_path / name)
        with open(p, "wb") as f:
            f.write(data if kw.pop("raw", False) else sbam.bgzf(data, **kw))
        return p
    whole = sbam.bgzf(head + b"".join(body))
    assert "bad magic" in _refusal(write("magic.bam", b"BAX\1" + head[4:] + b"".join(body)), header=True)
    assert "bad magic" in _refusal(write("gzip.bam", b"\x1f\x8b\x08\x00" + whole[4:], raw=True), header=True)
    assert "truncated" in _refusal(write("cut.bam", whole[:len(whole) - 28 - 9], raw=True), header=True)
    spoiled = bytearray(whole); spoiled[30] ^= 0x55
    assert "block" in _refusal(write("inflate.bam", bytes(spoiled), raw=True), header=True)
    short = struct.pack("<i", 20) + body[2][4:24]
    assert "record 2: block_size 20" in _refusal(write("short.bam", head + body[0] + body[1] + short))
    assert "record 5: the record runs past the end" in _refusal(write("past.bam", head + b"".join(body) + body[0][:30]))
    assert "n_ref" in _refusal(write("nref.bam", head[:8 + struct.unpack_from("<i", head, 4)[0]] + struct.pack("<i", -2)), header=True)
    bad_ref = bytearray(body[3]); bad_ref[4:8] = struct.pack("<i", 2)
    assert "record 3: refID 2 out of range" in _refusal(write("refid.bam", head + b"".join(body[:3]) + bytes(bad_ref)))
    fields = bytearray(body[1]); fields[20:24] = struct.pack("<i", 5000)
    assert "record 1: the fields run past block_size" in _refusal(write("fields.bam", head + body[0] + bytes(fields)))
    long_cigar = sbam.record_bytes(dict(good[0], cigar=[("S", 50), ("N", 70000)], tags=[("CG", "B", ("I", [50 << 4]))]))
    assert "record 1: the CIGAR is the placeholder of a long CIGAR" in _refusal(write("cg.bam", head + body[0] + long_cigar))


def test_auxiliary_walk_sets_the_error_slot(tmp_path):
    refs = [("c1", 1000)]
    base = dict(ref=0, flag=3, mapq=30, l_seq=50, cigar=[("M", 50)], name="walker")
    ok = dict(base, tags=[("NM", "C", 0)], name="fine")
    for tail, reason in ((b"XZZabc", 1), (b"XBBi\x10\0\0\0", 1), (b"NM", 1), (b"XQ?1", 4), (b"NMf\0\0\0\0", 3), (b"NMZ1\0", 3), (b"", 2)):
        path = str(tmp_path / "aux.bam")
        sbam.write_bam(path, refs, [ok] * 70 + [dict(base, tags=[("RG", "Z", "g")], raw_tail=tail), dict(base, tags=[], raw_tail=b"XZZabc")] + [ok] * 3)
        with pytest.raises(emu.RecordError) as e:
            emu.counters(path, *cr.PARAMS)
        assert (e.value.record, e.value.reason, e.value.read) == (70, reason, "walker"), tail
        dup = dict(base, flag=0x403, tags=[], raw_tail=tail)                   # the chain stops before NM: nothing is walked
        sbam.write_bam(path, refs, [ok, dup])
        got, _ = emu.counters(path, *cr.PARAMS)
        assert got[0].tolist() == [2, 1, 0, 0, 0, 0, 0, 1, 50]


@pytest.mark.parametrize("nrec", [1, 63, 64, 65, 129])
def test_structure_small_counts(nrec, tmp_path):
    refs, recs = cr.synthetic(nrec, min(nrec, 3), seed=nrec)
    path = str(tmp_path / "s.bam")
    sbam.write_bam(path, refs, recs)
    _r, _l, want = cr.counters(path, *cr.PARAMS)
    for budget in (0, 1, 2000):
        got, _ = emu.counters(path, *cr.PARAMS, budget=budget)
        assert (got[:len(refs)] == want).all()


def test_structure_runs_boundaries_and_order(tmp_path):
    """Runs that end on a wavefront boundary, one record past it and across a batch boundary; the same records interleaved give the same
    counters with more atomic adds; any batch size gives the same counters."""
    runs = [64, 65, 63, 1, 128, 1, 190, 2, 62, 300]
    refs, recs = cr.synthetic(sum(runs), len(runs), seed=3, run_lengths=runs)
    path, mixed = str(tmp_path / "sorted.bam"), str(tmp_path / "mixed.bam")
    sbam.write_bam(path, refs, recs)
    sbam.write_bam(mixed, *cr.synthetic(sum(runs), len(runs), seed=3, run_lengths=runs, interleave=True))
    _r, _l, want = cr.counters(path, *cr.PARAMS)
    assert want[:, 0].tolist() == runs and (cr.counters(mixed, *cr.PARAMS)[2] == want).all()
    one, info1 = emu.counters(path, *cr.PARAMS)
    rec_bytes = len(sbam.record_bytes(recs[0]))
    many, info2 = emu.counters(path, *cr.PARAMS, budget=70 * rec_bytes)
    mix, info3 = emu.counters(mixed, *cr.PARAMS)
    assert (one[:len(refs)] == want).all() and (many == one).all() and (mix == one).all()
    assert info1["batches"] == 1 and info2["batches"] >= 10 and info3["atomics"] > 5 * info1["atomics"]


def test_parameters_are_checked_without_a_device():
    _lib.coverage_check(False, 0.98, 0.02, 15)
    with pytest.raises(_lib.CkmError):
        _lib.coverage_check(False, float("nan"), 0.02, 15)


@pytest.mark.parametrize("g", GOLD["coverage_files"], ids=lambda g: g["name"])
def test_profile_parse_and_bin_profiles_match_the_reference(g, tmp_path):
    path = str(tmp_path / "coverage.tsv")
    with open(path, "w") as f:
        f.write(g["text"])
    c = cov.Coverage(1)
    assert c.parseCoverage(path) == g["parseCoverage"]
    prof = c.binProfiles(path)
    assert {b: {m: [float(v[0]), float(v[1])] for m, v in p.items()} for b, p in prof.items()} == g["binProfiles"]
    assert {b: list(p.keys()) for b, p in prof.items()} == g["binProfiles_order"]
    for tab, key in ((True, "profile_tab"), (False, "profile_pretty")):
        out = str(tmp_path / key)
        Profile().run(path, out, tab)
        assert open(out).read() == g[key]
    with pytest.raises(SystemExit):
        Profile().run(str(tmp_path / "missing.tsv"), "", True)


def test_goldens_hold_the_profile_branches():
    three = next(g for g in GOLD["coverage_files"] if g["name"] == "three_bams")
    assert "unbinned" in three["binProfiles"] and three["binProfiles"]["bin_single"]["zeta"][1] == 0.0          # one sequence: no variance
    rows = [ln.split("\t") for ln in three["profile_tab"].splitlines()]
    k = rows[0].index("alpha: % binned populations")
    assert all(r[k] in ("0.0", "NA") for r in rows[1:])                                                            # sumNormBinCoverage == 0
