"""GPU: every single-stream entry point owns its stream and events through one call scope (CallStream, ckm_host.h).  For each of them: a
valid call, a call the argument checks refuse (nothing launched, the scope never opened), the valid call again in the same process --
the same bytes both times, every timing finite and not negative -- and, where the entry point has one, a call without device work."""
import ctypes as C
import math

import numpy as np
import pytest

from checkm_amd import _lib
from checkm_amd.hmmerModelParser import read_nuc_models
from synthdata import bam as sbam
from tests import coverage_reference as cr
from tests import merger_common as mc
from tests import ssufinder_synth as syn
from tests import test_placement_host as place_host
from tests import test_selection_host as select_host
from tests import test_simscaffolds_host as simscaf_host
from tests import test_simulation_host as sim_host
from tests.test_gpu_nucstats import write_fasta
from tests.test_gpu_placement import TREES, tables as place_tables
from tests.test_markerset_host import synthetic_table

pytestmark = pytest.mark.gpu

EINVAL = -1
LOOSE = [-1000.0, 1000.0, -1000.0, 1000.0]


def timings_ok(r):
    ms = {k: v for k, v in r.items() if k.startswith("ms_")}
    assert "ms_total" in ms and ms["ms_total"] > 0, ms
    assert all(math.isfinite(v) and v >= 0 for v in ms.values()), ms


def same_outputs(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if k.startswith("ms_"):
            continue
        if isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k
        elif isinstance(a[k], list):      # arrays of unequal shapes: select_run's rows, one array per genome
            assert len(a[k]) == len(b[k]) and all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a[k], b[k])), k
        else:
            assert a[k] == b[k], k


def twice_around_a_refusal(valid, refused):
    """valid() -> dict of outputs and timings; refused() makes the call that the argument checks turn down."""
    first = valid()
    with pytest.raises(_lib.CkmError) as e:
        refused()
    assert e.value.code == EINVAL
    second = valid()
    same_outputs(first, second)
    timings_ok(first)
    timings_ok(second)
    return first


@pytest.fixture(scope="module")
def seqs(tmp_path_factory):
    """Two files, three sequences: a run of twelve N (the fill pass of nucstats runs), a length that is no multiple of 16, lower case."""
    rng = np.random.default_rng(5)
    def dna(n):
        return rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n).tobytes()
    d = tmp_path_factory.mktemp("scope")
    paths = [write_fasta(d / "a.fna", [("a1", dna(700) + b"N" * 12 + dna(333)), ("a2", dna(65).lower())]), write_fasta(d / "b.fna", [("b1", dna(1500))])]
    s = _lib.NucSeqs(paths)
    yield s
    s.close()


def test_nucstats(gpu_ctx, seqs):
    r = twice_around_a_refusal(lambda: _lib.nucstats(gpu_ctx, seqs, tetra=True), lambda: _lib.nucstats(gpu_ctx, seqs, tetra=True, tile_bytes=24))
    assert r["run_starts"] == 1 and r["ms_fill"] > 0 and int(r["count"][:, 6].sum()) == 700 + 12 + 333 + 65 + 1500


def test_seq_windows(gpu_ctx, seqs):
    sig = np.full((2, 136), 1.0 / 136)
    r = twice_around_a_refusal(lambda: _lib.seq_windows(gpu_ctx, seqs, 100, bin_sig=sig, want_tetra=True, piece_bytes=64),
                               lambda: _lib.seq_windows(gpu_ctx, seqs, 100, bin_sig=sig, want_tetra=True, piece_bytes=8))
    assert r["windows"] == 10 + 0 + 14 and r["batches"] >= 1


@pytest.mark.parametrize("stat", ["gc", "td"])
def test_refdist(gpu_ctx, seqs, stat):
    starts, sizes = [0, 5, 990, 2400], [100, 700, 40, 210]                      # the scaffold: 1045 + 65 + 1500 bytes, no separator
    r = twice_around_a_refusal(lambda: _lib.refdist(gpu_ctx, seqs, stat, 0, starts, sizes, block=64),
                               lambda: _lib.refdist(gpu_ctx, seqs, stat, 0, starts, [100, 700, 40, 211], block=64))
    assert r["windows"] == 4 and r["bytes"] == 2610


def test_unbinned(gpu_ctx, seqs):
    keep = np.array([1, 0, 1], dtype=np.uint8)
    r = twice_around_a_refusal(lambda: _lib.unbinned_count(gpu_ctx, seqs, keep), lambda: _lib.unbinned_count(gpu_ctx, seqs, keep, tile_bytes=1000))
    assert r["kept"] == 2 and r["counts"][:, 4].tolist() == [1045, 0, 1500]
    nothing = _lib.unbinned_count(gpu_ctx, seqs, np.zeros(3, dtype=np.uint8))    # nothing kept: the scope is never opened
    assert not nothing["counts"].any() and nothing["batches"] == 0 and nothing["ms_upload"] == 0
    timings_ok(nothing)
    same_outputs(r, _lib.unbinned_count(gpu_ctx, seqs, keep))


def test_outliers(gpu_ctx, seqs):
    ns = _lib.nucstats(gpu_ctx, seqs, tetra=True)
    sig = ns["tetra"] / ns["tetra"].sum(axis=1, keepdims=True)
    coding = np.array([500, 30, 900], dtype=np.int64)
    def run(td_tab):
        return _lib.outliers(gpu_ctx, seqs, ns["count"], sig, coding, [0, 2], [100.0, 2000.0], [-0.01, -0.02], [0.01, 0.02], [0, 0], [0, 0], td_tab)
    r = twice_around_a_refusal(lambda: run(0), lambda: run(1))
    assert len(r["td"]) == 3 and r["bin_sig"].shape == (2, 136)


def test_merge(gpu_ctx):
    member, hit_sum, n_markers = mc.synthetic(70, 104, seed=3)
    bits = mc.pack(member)
    bad = n_markers.copy(); bad[69] = 0
    r = twice_around_a_refusal(lambda: _lib.merge_pairs(gpu_ctx, bits, hit_sum, n_markers, 104, LOOSE), lambda: _lib.merge_pairs(gpu_ctx, bits, hit_sum, bad, 104, LOOSE))
    assert r["npairs"] == 70 * 69 // 2
    one = _lib.merge_pairs(gpu_ctx, bits[:1], hit_sum[:1], n_markers[:1], 104, LOOSE)      # one bin: no pair, the scope is never opened
    assert one["npairs"] == 0 and one["ms_upload"] == 0
    timings_ok(one)
    same_outputs(r, _lib.merge_pairs(gpu_ctx, bits, hit_sum, n_markers, 104, LOOSE))


def test_aai(gpu_ctx):
    groups = [[b"ACDEFGHIKL", b"ACDEFGHIKM", b"ACDEFGHIKL"], [b"MK" * 600, b"MR" * 600]]
    r = twice_around_a_refusal(lambda: _lib.aai_pairs(gpu_ctx, groups), lambda: _lib.aai_pairs(gpu_ctx, [[b"ACD", b"AC"]]))
    assert r["npairs"] == 4 and r["mismatches"].tolist() == [1, 0, 1, 600]
    none = _lib.aai_pairs(gpu_ctx, [[], [b"ACD"], []])                           # zero pairs: the scope is never opened
    assert none["npairs"] == 0 and none["nbatches"] == 0 and none["ms_upload"] == 0
    timings_ok(none)
    same_outputs(r, _lib.aai_pairs(gpu_ctx, groups))


def test_coverage(gpu_ctx, tmp_path):
    refs, recs = cr.synthetic(65, 3, seed=65)
    path = str(tmp_path / "s.bam")
    sbam.write_bam(path, refs, recs)
    def run(min_qc):
        b = _lib.Bam(path)
        try:
            params = list(cr.PARAMS)
            params[3] = min_qc
            counters, t = _lib.coverage_counters(gpu_ctx, b, *params, budget_bytes=1 if min_qc == cr.PARAMS[3] else 0)
            return dict(t, counters=counters)
        finally:
            b.close()
    r = twice_around_a_refusal(lambda: run(cr.PARAMS[3]), lambda: run(float("nan")))
    assert r["records"] == 65 and r["batches"] == 65 and (r["counters"] == cr.counters(path, *cr.PARAMS)[2]).all()


@pytest.fixture(scope="module")
def mset_table(gpu_ctx):
    """Six genomes, seventy families: two tile columns of marker pairs."""
    t = _lib.MsetTable(gpu_ctx, *synthetic_table(21, 6, 70))
    yield t
    t.close()


def test_mset_markers(gpu_ctx, mset_table):
    r = twice_around_a_refusal(lambda: _lib.mset_markers(gpu_ctx, mset_table, [[0, 1, 2], [5]], [2.0, 1.0], [1.0, 1.0], want_counts=True),
                               lambda: _lib.mset_markers(gpu_ctx, mset_table, [[6]], [1.0], [1.0]))
    assert r["flag"].shape == (2, 70) and r["counts"].shape == (2, 70, 3) and r["nbatches"] == 1


def test_mset_colocated(gpu_ctx, mset_table):
    markers = list(range(70))
    r = twice_around_a_refusal(lambda: _lib.mset_colocated(gpu_ctx, mset_table, [[0, 1, 2, 3]], [markers], genome_threshold=0.2),
                               lambda: _lib.mset_colocated(gpu_ctx, mset_table, [[0, 6]], [[0, 1]]))
    assert r["tests"] == 4 * (70 * 69 // 2) and r["npairs"] > 0 and r["nrounds"] == 1
    none = _lib.mset_colocated(gpu_ctx, mset_table, [[0, 1]], [[3]])            # one marker: no pair to test, the scope is never opened
    assert none["npairs"] == 0 and none["nrounds"] == 0 and none["ms_upload"] == 0
    timings_ok(none)


def test_sim_run(gpu_ctx):
    r = twice_around_a_refusal(lambda: _lib.sim_run(gpu_ctx, sim_host.small_tables()), lambda: _lib.sim_run(gpu_ctx, sim_host.small_tables(starts=[1000, 0, 5, 5, 2000])))
    assert r["out"].shape == (3, 2, 4) and r["nrounds"] == 1
    none = _lib.sim_run(gpu_ctx, sim_host.small_tables(rs_off=[0], starts=[], contig_len=[]))      # no replicate: the scope is never opened
    assert none["out"].shape == (0, 2, 4) and none["nrounds"] == 0 and none["ms_upload"] == 0
    timings_ok(none)
    same_outputs(r, _lib.sim_run(gpu_ctx, sim_host.small_tables()))


def test_simscaf_run(gpu_ctx):
    r = twice_around_a_refusal(lambda: _lib.simscaf_run(gpu_ctx, simscaf_host.small_tables()),
                               lambda: _lib.simscaf_run(gpu_ctx, simscaf_host.small_tables(cont=[2, _lib.SIMSCAF_NONE, 0])))
    assert r["out"].shape == (3, 2, 4) and r["out"][0, 0].tolist() == [100 * 2.0 / 3, 100 * 2.0 / 3, 50.0, 50.0] and r["nrounds"] == 1


def test_select_run(gpu_ctx):
    r = twice_around_a_refusal(lambda: _lib.select_run(gpu_ctx, select_host.small_tables(), with_rows=True),
                               lambda: _lib.select_run(gpu_ctx, select_host.small_tables(ms_off=[0, 2, 2])))
    assert r["truth"].shape == (2, 3, 2) and r["out"].shape == (2, 3, 2, 4) and r["nrounds"] == 1
    none = _lib.select_run(gpu_ctx, select_host.small_tables(R=0))              # no draw: the scope is never opened
    assert none["truth"].size == 0 and none["nrounds"] == 0 and none["ms_upload"] == 0
    timings_ok(none)
    same_outputs(r, _lib.select_run(gpu_ctx, select_host.small_tables(), with_rows=True))


@pytest.mark.parametrize("make", [place_host.small_tables, lambda **over: place_tables(2, TREES["two_leaves"], 10, 2)], ids=["trifurcating_root", "two_leaves"])
def test_place_run(gpu_ctx, make):
    def bad():
        t = make()
        t.length[0] = -1.0
        return _lib.place_run(gpu_ctx, t)
    r = twice_around_a_refusal(lambda: _lib.place_run(gpu_ctx, make()), bad)
    assert r["nchunks"] >= 1 and r["top_edge"].size > 0


def test_nhmm_run(gpu_ctx, tmp_path):
    p = str(tmp_path / "m10.hmm")
    cons = syn.write_model(p, "m10", 10, 5)
    m = read_nuc_models(p)[0]
    text, _ = syn.planted_contig(np.random.default_rng(6), 300, [(60, cons, False), (190, cons, True)])
    fna = str(tmp_path / "contig.fna")
    syn.write_fasta(fna, [("contig", text)])
    seqs = _lib.NucSeqs([fna])
    try:
        r = twice_around_a_refusal(lambda: _lib.nhmm_run(gpu_ctx, _lib.NhmmTables([(m.emis, m.trans)], [0], 64, 32, 3), seqs),
                                   lambda: _lib.nhmm_run(gpu_ctx, _lib.NhmmTables([(m.emis, m.trans)], [0], 64, 32, 0), seqs))
        assert len(r["row_pos"]) > 0 and r["launches"] == 1 and len(r["hit_from"]) >= 2
    finally:
        seqs.close()


def test_gtree_run(gpu_ctx):
    rng = np.random.default_rng(8)
    text = rng.choice(np.frombuffer(b"ACDEFGHIKL-", dtype=np.uint8), size=4 * 16)
    cols = rng.integers(0, 16, size=(2, 16))
    def refused():      # gtree_run itself asks ckm_gtree_check first: the entry point's own refusal is reached through the library
        bad = _lib.GtreeTables(text=text, nrows=4, ncols=16, cols=cols, model=7)
        a, o, info = bad.args(), _lib.GtreeOut(None, None, None, None, None), _lib.GtreeInfo()
        _lib._chk(_lib.load().ckm_gtree_run(gpu_ctx.h, C.byref(a), 0, C.byref(o), C.byref(info)))
    r = twice_around_a_refusal(lambda: _lib.gtree_run(gpu_ctx, _lib.GtreeTables(text=text, nrows=4, ncols=16, cols=cols, model="poisson"), counts=True, dist=True), refused)
    assert r["ntrees"] == 3 and r["merge_ij"].shape == (3, 3, 2) and r["compared"].shape == (4, 4)
