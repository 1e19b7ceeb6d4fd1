"""ReferenceDistributions on the device: kernels_refdist.hip against the plain-Python restatement (tests/refdist_reference.py) and against
the goldens made from the reference's own primitives (tests/golden/refdist_cases.json).  Everything is compared at ==, floats by
float.hex(); nothing is timed."""
import random

import numpy as np
import pytest

from checkm_amd import _lib, binTools as bt, common
from checkm_amd import genomicSignatures as gs
from checkm_amd import referenceDistributions as rdm
from checkm_amd.defaultValues import DefaultValues
from tests import refdist_reference as ref
from tests.test_bintools_host import restated_outliers
from tests.test_refdist_host import (BLOCKS, CASES, RUNS, expect, outcome, random_genome, restated_windows, run_windows, through_class, trim, window_shapes,
                                     write_case)

pytestmark = pytest.mark.gpu
STATS = ["gc", "cd", "td"]


@pytest.mark.parametrize("name,stat", RUNS)
def test_every_golden_case(gpu_ctx, tmp_path, name, stat):
    case = CASES[name]
    path, gff = write_case(tmp_path, case)
    R = rdm.ReferenceDistributions()
    assert trim(outcome(lambda: through_class(R, case, stat, path, gff))) == expect(case, stat)
    assert not R.last_timing or not R.last_timing["host"]


@pytest.mark.parametrize("stat", STATS)
@pytest.mark.parametrize("block", BLOCKS)
def test_blocks_and_window_shapes(gpu_ctx, tmp_path, stat, block):
    r = random.Random(100 + block)
    seqs = random_genome(r, [3000, 1, 2500, 64, 0, 1777, 2001])
    scaf = ref.scaffold(dict(enumerate(seqs)), stat)
    assert len(scaf) <= 10000
    st, sz = window_shapes(r, len(scaf), block)
    want = restated_windows(scaf, stat, st, sz)
    got, o = run_windows(_lib.refdist, gpu_ctx, tmp_path, seqs, stat, st, sz, block=block)
    assert got == want and o["blocks"] == -(-len(scaf) // block)
    small, _ = run_windows(_lib.refdist, gpu_ctx, tmp_path, seqs, stat, st, sz, block=block, budget_bytes=544 * 5)
    assert small == want


@pytest.mark.parametrize("stat", ["gc", "td"])
def test_same_bytes_for_every_block_size(gpu_ctx, tmp_path, stat):
    r = random.Random(5)
    seqs = random_genome(r, [4000, 3000])
    scaf = ref.scaffold(dict(enumerate(seqs)), stat)
    st, sz = window_shapes(r, len(scaf), 64)
    got = [run_windows(_lib.refdist, gpu_ctx, tmp_path, seqs, stat, st, sz, block=b)[0] for b in BLOCKS + [0, 128, 512]]
    assert all(g == got[0] for g in got) and got[0] == restated_windows(scaf, stat, st, sz)


@pytest.mark.parametrize("stat", ["gc", "td"])
@pytest.mark.parametrize("nwin", [1, 7, 8, 9, 65])
def test_ragged_groups_of_windows(gpu_ctx, tmp_path, stat, nwin):
    r = random.Random(nwin)
    seqs = random_genome(r, [1500, 900])
    scaf = ref.scaffold(dict(enumerate(seqs)), stat)
    sz = [r.choice([3, 4, 50, 256, 700, 2000]) for _ in range(nwin)]
    st = [r.randint(0, len(scaf) - w) for w in sz]
    assert run_windows(_lib.refdist, gpu_ctx, tmp_path, seqs, stat, st, sz)[0] == restated_windows(scaf, stat, st, sz)


@pytest.mark.parametrize("stat", ["gc", "td"])
@pytest.mark.parametrize("nblocks", [1, 63, 64, 65])
def test_scan_seams(gpu_ctx, tmp_path, stat, nblocks):
    r = random.Random(nblocks)
    sep = rdm.SEP_LEN[stat]
    L = nblocks * 16 - (5 if nblocks > 1 else 0)
    seqs = random_genome(r, [L - L // 2 - sep, L // 2], dirty=False)
    scaf = ref.scaffold(dict(enumerate(seqs)), stat)
    assert len(scaf) == L
    st, sz = window_shapes(r, L, 16)
    for w in (L // 2, L - 17, 62 * 16, 63 * 16 + 1, 64 * 16):
        if 0 < w <= L:
            st += [0, L - w, (L - w) // 2]
            sz += [w] * 3
    got, o = run_windows(_lib.refdist, gpu_ctx, tmp_path, seqs, stat, st, sz, block=16)
    assert got == restated_windows(scaf, stat, st, sz) and o["blocks"] == nblocks


def gene_text(genomeId, L, r):
    rows, pos = [], 1
    while pos + 400 < L:
        a = pos + r.randint(0, 120)
        z = a + r.randint(150, 380)
        rows.append("%s\tProdigal_v2.6.3\tCDS\t%d\t%d\t10.0\t+\t0\tID=1_%d;partial=00\n" % (genomeId, a, z, len(rows) + 1))
        pos = z - r.randint(0, 30)
    return "##gff-version  3\n" + "".join(rows)


def test_default_block_on_a_70_kb_genome(gpu_ctx, tmp_path):
    """One genome of 70 kb for all three statistics and every default size up to 50 000.  Its first contig is 56 kb without an ambiguous
    byte (lower case and U are bases after upper-casing), so a CD window of 50 000 is accepted at 6 000 of the 20 020 possible starts; the
    other two contigs carry N runs and IUPAC codes."""
    r = random.Random(70)
    first = list(random_genome(r, [56000], dirty=False)[0])
    for _ in range(2000):
        first[r.randrange(56000)] = r.choice("acgtUu")
    seqs = ["".join(first)] + random_genome(r, [9000, 5000])
    path, gffPath = str(tmp_path / "big.fna"), str(tmp_path / "big.gff")
    open(path, "w").write("".join(">c%d\n%s\n" % (i, s) for i, s in enumerate(seqs)))
    gff = gene_text("big", 70020, r)
    open(gffPath, "w").write(gff)
    R = rdm.ReferenceDistributions()
    sizes = [w for w in R.windowSizes() if w <= 50000]
    assert sizes[0] == 500 and sizes[-1] == 50000 and len(sizes) == 30
    d = dict(enumerate(seqs))
    for stat, got, want in (("gc", lambda: R.deltaGC(path, 200, sizes, 1), lambda: ref.delta_gc(d, "big", 200, sizes, 1)),
                            ("td", lambda: R.deltaTD(path, 200, sizes, 1), lambda: ref.delta_td_numpy(d, "big", 200, sizes, 1)),
                            ("cd", lambda: R.deltaCD(path, gffPath, 200, sizes, 1), lambda: ref.delta_cd(d, gff, "big", 200, sizes, 1))):
        g, w = outcome(got), outcome(want)
        assert w["error"] is None and sorted(w["dist"], key=int) == [str(x) for x in sizes] and all(len(v) == 200 for v in w["dist"].values())
        assert g == w, stat
        assert R.last_timing["prefix_blocks"] == -(-(70000 + 2 * rdm.SEP_LEN[stat]) // 256) and not R.last_timing["host"]


def test_tables_from_genomes_drive_identify_outliers(gpu_ctx, tmp_path):
    r = random.Random(6)
    genomes, gffs = [], []
    for k in range(6):
        p = 0.35 + 0.05 * k
        text = "".join(r.choice("GC") if r.random() < p else r.choice("AT") for _ in range(3000))
        path, gff = str(tmp_path / ("ref%d.fna" % k)), str(tmp_path / ("ref%d.gff" % k))
        open(path, "w").write(">a\n%s\n>b\n%s\n" % (text[:1800], text[1800:]))
        open(gff, "w").write(gene_text("ref%d" % k, 3010, r))
        genomes.append(path)
        gffs.append(gff)
    R = rdm.ReferenceDistributions()
    work = str(tmp_path / "work")
    R.run(genomes, work, gffFiles=gffs, numWindows=40, windowSizes=[500, 700, 1000], seed=3)
    root = tmp_path / "data"
    (root / "distributions").mkdir(parents=True)
    R.bounds(work + "/deltaGC", str(root / "distributions" / "gc_dist.txt"), minGenomes=1)
    R.bounds(work + "/deltaCD", str(root / "distributions" / "cd_dist.txt"), minGenomes=1)
    _, bad = R.boundsTD(work + "/deltaTD", str(root / "distributions" / "td_dist.txt"), seed=3)
    assert bad == []
    before = DefaultValues.CHECKM_DATA_DIR
    DefaultValues.set_data_root(str(root))
    try:
        dists = tuple(common.readDistribution(k) for k in ("gc_dist", "cd_dist", "td_dist"))
        assert all(len(d) > 0 for d in dists)
        out = tmp_path / "out"
        (out / "bins" / "binA").mkdir(parents=True)
        contigs = [("k0", "".join(r.choice("ACGT") for _ in range(900))), ("k1", "".join(r.choice("GGGC") for _ in range(600))), ("k2", "".join(r.choice("ACGT") for _ in range(1200))),
                   ("k3", "".join(r.choice("AATT") for _ in range(500)))]
        binFile, prof, o = str(tmp_path / "binA.fna"), str(tmp_path / "tetra.tsv"), str(tmp_path / "outliers.tsv")
        open(binFile, "w").write("".join(">%s\n%s\n" % kv for kv in contigs))
        (out / "bins" / "binA" / "genes.gff").write_text("##gff-version  3\n" + "".join(gene_text(k, len(s), r).split("\n", 1)[1] for k, s in contigs))
        gs.GenomicSignatures(4, 1).calculate(binFile, prof)
        bt.BinTools().identifyOutliers(str(out), [binFile], prof, 95, "any", o)
        got = open(o).read()
        assert got == restated_outliers(str(out), [binFile], prof, 95, "any", dists) and got.count("\n") > 1
    finally:
        DefaultValues.set_data_root(before)
