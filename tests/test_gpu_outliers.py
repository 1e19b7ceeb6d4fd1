"""`checkm outliers` on the device: BinTools.identifyOutliers against the reference's files (tests/golden/outliers_cases.json), against
BinTools' numpy helpers on synthetic bins at real size (a bin of more than 10 000 short contigs and a one-contig bin among them),
run-to-run and batch-split identity, and the reference's failures."""
import ast
import hashlib
import logging
import os

import numpy as np
import pytest

from checkm_amd import _lib
from checkm_amd import binTools as bt
from checkm_amd import genomicSignatures as gs
from tests.test_bintools_host import CASES, GOLD, HEADER, data_root, fixture_dists, helper_columns, restated_outliers, same_bits, write_case  # noqa: F401
from tests.test_gpu_nucstats import synthetic_bins, write_fasta

pytestmark = pytest.mark.gpu


def device_profile(case, tmp):
    """The case's tetranucleotide profile written by GenomicSignatures.calculate on the device, plus the repeated ids; its SHA-256 is the
    reference file's."""
    fa, prof = str(tmp / "profile.fna"), str(tmp / "tetra.tsv")
    open(fa, "w").write(case["profile_fasta"])
    gs.GenomicSignatures(4, 1).calculate(fa, prof)
    rows = dict((ln.split("\t", 1)[0], ln.split("\t", 1)[1]) for ln in open(prof).read().splitlines(True)[1:])
    with open(prof, "a") as f:
        for seqId, src in case["repeat"]:
            f.write(seqId + "\t" + rows[src])
    assert hashlib.sha256(open(prof, "rb").read()).hexdigest() == case["profile_sha256"]
    return prof


def test_every_golden_run_writes_the_reference_file(tmp_path, data_root):
    case = CASES["three_bins"]
    paths, out, _ = write_case(tmp_path, case)
    prof = device_profile(case, tmp_path)
    for r in case["runs"]:
        o = str(tmp_path / ("o_%d_%s.tsv" % (r["distribution"], r["reportType"])))
        bt.BinTools().identifyOutliers(out, paths, prof, r["distribution"], r["reportType"], o)
        assert open(o).read() == r["output"], (r["distribution"], r["reportType"])


def test_the_reference_failures(tmp_path, data_root, caplog):
    for name, exc in (("missing_gff", SystemExit), ("missing_id", KeyError), ("zero_division", ZeroDivisionError)):
        case = CASES[name]
        d = tmp_path / name
        d.mkdir()
        paths, out, _ = write_case(d, case)
        prof = device_profile(case, d)
        want = case["runs"][0]["error"]
        with caplog.at_level(logging.ERROR, logger="timestamp"), pytest.raises(exc) as e:
            bt.BinTools().identifyOutliers(out, paths, prof, 95, "any", str(d / "o.tsv"))
        if exc is SystemExit:
            assert e.value.code == want["code"] and caplog.records[-1].getMessage() == want["log"][0]
        else:
            assert [str(a) for a in e.value.args] == want["args"]


def test_library_reports_the_division_by_zero_itself(tmp_path, gpu_ctx):
    """ckm_outliers_run is the backstop of the check BinTools makes first: a sequence without A, C, G, T, U is refused, not computed."""
    p = tmp_path / "z.fna"
    p.write_text(">a\nACGTACGT\n>z\nNNNNNN\n")
    seqs = _lib.NucSeqs([str(p)])
    r = _lib.nucstats(gpu_ctx, seqs)
    with pytest.raises(ZeroDivisionError):
        _lib.outliers(gpu_ctx, seqs, r["count"], np.zeros((2, 136)), np.zeros(2, dtype=np.int64), [0, 1], [100.0], [0.0], [0.0], [0], [0], 0)
    with pytest.raises(_lib.CkmError):                       # a table index outside the tables
        _lib.outliers(gpu_ctx, seqs, r["count"], np.zeros((2, 136)), np.zeros(2, dtype=np.int64), [0, 1], [100.0], [0.0], [0.0], [3], [0], 0)
    seqs.close()


def synthetic_workload(tmp, n_bins=64, seed=77):
    """Bins of the shape tests/test_gpu_nucstats.py uses, a bin of 10 500 short contigs and a one-contig bin; one contig in twelve has a
    skewed composition, one in sixteen has no genes.  Returns (bin paths, out dir, FASTA of all contigs)."""
    rng = np.random.default_rng(seed)
    bins = synthetic_bins(n_bins, seed)
    many = []
    for c in range(10500):
        many.append(("many_c%d" % c, rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=int(rng.integers(200, 600))).tobytes()))
    bins.append(many)
    bins.append([("single_c0", rng.choice(np.frombuffer(b"ACGTN", dtype=np.uint8), size=150000, p=[.2, .3, .29, .2, .01]).tobytes())])
    out = tmp / "out"
    paths = []
    with open(str(tmp / "assembly.fna"), "wb") as asm:
        for b, contigs in enumerate(bins):
            name = "sbin%03d" % b
            gff = ["##gff-version  3\n"]
            for k, (cid, s) in enumerate(contigs):
                if (k + b) % 12 == 5:                                        # skewed composition: GC (and often TD) outliers
                    s = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=len(s), p=[.15, .35, .35, .15]).tobytes()
                    contigs[k] = (cid, s)
                if (k + b) % 16 == 3:                                        # no genes: CD outliers
                    continue
                pos, n = 1, len(s)
                cover = float(rng.uniform(0.8, 0.95))
                while pos + 60 < n:
                    z = min(n, pos + int(rng.integers(300, 3000)))
                    gff.append("%s\tx\tCDS\t%d\t%d\t1.0\t+\t0\tID=g\n" % (cid, pos, z))
                    pos = z - 20 if rng.random() < 0.2 else z + 1 + int((z - pos) * (1 - cover) / cover)
            paths.append(write_fasta(tmp / (name + ".fna"), contigs))
            asm.write(open(paths[-1], "rb").read())
            d = out / "bins" / name
            d.mkdir(parents=True)
            (d / "genes.gff").write_text("".join(gff))
    return paths, str(out), str(tmp / "assembly.fna")


def test_synthetic_bins_at_real_size(tmp_path, data_root, monkeypatch):
    paths, out, asm = synthetic_workload(tmp_path)
    prof = str(tmp_path / "tetra.tsv")
    gs.GenomicSignatures(4, 8).calculate(asm, prof)
    seen = []
    real = _lib.outliers

    def spy(*a, **k):
        seen.append((a, real(*a, **k)))
        return seen[-1][1]
    monkeypatch.setattr(_lib, "outliers", spy)
    tools = bt.BinTools()
    f1 = str(tmp_path / "o1.tsv")
    tools.identifyOutliers(out, paths, prof, 95, "any", f1)
    monkeypatch.setattr(_lib, "outliers", real)
    text = open(f1).read()
    t = tools.last_timing
    assert t["bins"] == len(paths) == 66 and t["sequences"] > 10500
    # thresholds that flag nothing or everything cannot pass
    assert 0.01 * t["sequences"] <= t["flagged"] <= 0.5 * t["sequences"], (t["flagged"], t["sequences"])
    assert text.count("\n") - 1 == t["flagged"]
    # the file against the plain-Python statement of the writer
    with np.errstate(invalid="ignore"):
        assert text == restated_outliers(out, paths, prof, 95, "any", fixture_dists())
    # the device columns against the numpy helpers, bit for bit
    assert len(seen) == 1
    (ctx, seqs, count, sig, coding, tab_off, key, lo, hi, gct, cdt, tdt), o = seen[0]
    sigs = gs.GenomicSignatures(4, 1).read(prof)
    bins = []
    first = [0]
    k = 0
    for p in paths:
        s = bt._read_fasta(p)
        bins.append((s, {i: int(coding[k + j]) for j, i in enumerate(s)}, {i: sigs[i] for i in s}))
        k += len(s)
        first.append(k)
    want = helper_columns(bins, (tab_off, key, lo, hi), gct, cdt, tdt)
    for name in ("gc", "delta_gc", "cd", "delta_cd", "td", "mean_gc", "mean_cd", "bin_sig"):
        assert same_bits(o[name], want[name]), name
    assert np.array_equal(o["flags"], want["flags"])
    for bit in (1, 2, 4):
        assert int((o["flags"] & bit != 0).sum()) > 0, bit
    # a second run, and a run whose batches hold a megabyte of files each, write the same file
    f2, f3 = str(tmp_path / "o2.tsv"), str(tmp_path / "o3.tsv")
    bt.BinTools().identifyOutliers(out, paths, prof, 95, "any", f2)
    monkeypatch.setenv("CKM_NUCSTATS_BATCH_MB", "1")
    calls = []
    monkeypatch.setattr(_lib, "outliers", lambda *a, **k: calls.append(1) or real(*a, **k))
    bt.BinTools().identifyOutliers(out, paths, prof, 95, "any", f3)
    assert len(calls) > 3
    assert open(f2).read() == text and open(f3).read() == text
    for kname in ("upload", "seq", "binsig", "td", "flags"):
        assert t[kname] > 0.0, kname
