"""The marker-set selection's draws on the device (kernels_select.hip) against the host executor of the same header (tests/emu/selection),
at == on the bits of the true values, the four results per marker set and every multiplicity row: the smallest shapes at which the
kernel takes another path -- contigs around the wavefront and the block, the LDS limit, every degenerate count of draws, markers around
the staged counts, co-located sets around the wavefront, the round cuts -- and MarkerSetSelection in both modes of drawing."""
import os
import re

import numpy as np
import pytest

from checkm_amd import _lib
from tests.emu import selection as emu
from tests.test_selection_host import ERANGE, GOLDEN, ROOT, make_tables, random_keys, random_sets, same, selection_of, synthetic_tables, wanted_tuples
from tests.test_selection_host import TIE_CONTIGS, TIE_RANK, tied_tables

pytestmark = pytest.mark.gpu

_DEV_H = open(os.path.join(ROOT, "checkm_amd", "csrc", "select_dev.h")).read()
MAX_CONTIGS = int(re.search(r"MAX_CONTIGS = (\d+);", _DEV_H).group(1))
STAGE_COUNTS = int(re.search(r"STAGE_COUNTS = (\d+);", open(os.path.join(ROOT, "checkm_amd", "csrc", "sim_dev.h")).read()).group(1))
LEN = 10                                                            # bases of a contig in the shape tests


def both(gpu_ctx, tables, budget_bytes=0):
    want, got = emu.select_run(None, tables, budget_bytes, with_rows=True), _lib.select_run(gpu_ctx, tables, budget_bytes, with_rows=True)
    assert same(got, want) and got["nrounds"] == want["nrounds"] and got["truth"].shape == want["truth"].shape and got["out"].shape == want["out"].shape
    plain = _lib.select_run(gpu_ctx, tables, budget_bytes)             # without the rows: the same numbers
    assert plain["rows"] is None and same(dict(plain, rows=[]), dict(want, rows=[]))
    return got


def shape_tables(C, comp, cont, seed, U=9, R=2, tail=7):
    """One genome of C contigs and a partial tail; markers with 0 to 5 copies at 0, in the tail, at genome_len, beyond it and at 2^31 - 1."""
    rng = np.random.RandomState(seed)
    n = C * LEN + tail
    keys = random_keys(rng, [n], U, LEN)
    keys[0][0] = [0, n - 1, n, 2**31 - 1, C * LEN - 1]
    if U > 1:
        keys[0][1] = []
    return make_tables([n], keys, random_sets(rng, U, 3), R, LEN, comp, cont, seed)


@pytest.mark.parametrize("C", [1, 63, 64, 65, 255, 256, 257, MAX_CONTIGS])
def test_contigs_and_degenerate_counts(gpu_ctx, C):
    assert MAX_CONTIGS >= 16384
    frac = lambda k: (k / C, k / C)
    many = int(C * 2.5 + 0.5)
    for comp, cont, holds in (((0.5, 1.0), (0.0, 0.2), lambda row: C // 2 <= row.sum() <= C + C // 5 + 1),
                              (frac(0), frac(0), lambda row: row.sum() == 0),                                    # nComp = 0, nCont = 0
                              (frac(1), frac(0), lambda row: row.sum() == 1),                                    # nComp = 1
                              (frac(0), frac(1), lambda row: row.sum() == 1),                                    # nCont = 1
                              (frac(C - 1), (2.5, 2.5), lambda row: row.sum() == C - 1 + many and many > C),     # nComp = C - 1, nCont > C (C = 1: all on one contig)
                              (frac(C), (0.0, 2.5), lambda row: row.min() >= 1),                                 # nComp = C
                              ((0.0, 1.0), frac(0), lambda row: row.max() <= 1)):
        got = both(gpu_ctx, shape_tables(C, comp, cont, 100 + C))
        assert all(holds(row.astype(np.int64)) for row in got["rows"][0]), (comp, cont)


def test_one_contig_more_is_refused_before_any_launch(gpu_ctx):
    t = shape_tables(MAX_CONTIGS + 1, (0.5, 1.0), (0.0, 0.2), 3)
    with pytest.raises(_lib.CkmError) as e:
        _lib.select_run(gpu_ctx, t)
    assert e.value.code == ERANGE and str(MAX_CONTIGS) in str(e.value)


@pytest.mark.parametrize("U", [1, 63, 64, 65, STAGE_COUNTS, STAGE_COUNTS + 1])
def test_markers(gpu_ctx, U):
    got = both(gpu_ctx, shape_tables(300, (0.5, 1.0), (0.0, 0.5), 200 + U, U=U, R=3))
    assert (got["out"] > 0).any()


@pytest.mark.parametrize("members", [1, 64, 65])
def test_colocated_sets_with_repeats_and_more_sets_than_wavefronts(gpu_ctx, members):
    rng = np.random.RandomState(members)
    U, n = 80, 500 * LEN + 3
    sets = [[[int(m) for m in rng.randint(0, U, size=members)] for _ in range(k)] for k in (1, 64, 65, 2, 3, 1, 5, 7, 2)]       # nine marker sets, four wavefronts
    sets[1][0][-1] = sets[1][0][0]
    both(gpu_ctx, make_tables([n], random_keys(rng, [n], U, LEN), sets, 3, LEN, seed=members))


@pytest.mark.parametrize("G,R", [(1, 1), (3, 1), (1, 3), (100, 100)])
def test_genomes_and_replicates(gpu_ctx, G, R):
    rng = np.random.RandomState(G * 1000 + R)
    lens = [int(x) for x in rng.randint(LEN, 700 * LEN, size=G)]            # genomes of different lengths in one call
    got = both(gpu_ctx, make_tables(lens, random_keys(rng, lens, 30, LEN), random_sets(rng, 30, 5), R, LEN, seed=G))
    assert got["nrounds"] == 1 and got["out"].shape == (G, R, 5, 4)


def test_budgets_and_seeds(gpu_ctx):
    t = synthetic_tables(8)
    draws = t.ngenomes * t.nreplicates
    one = both(gpu_ctx, t)
    assert one["nrounds"] == 1
    several, each = both(gpu_ctx, t, budget_bytes=3000), both(gpu_ctx, t, budget_bytes=1)
    assert 1 < several["nrounds"] < draws and each["nrounds"] == draws and same(several, one) and same(each, one)
    assert same(both(gpu_ctx, synthetic_tables(8)), one)                       # the same seed twice
    t.seed += 1
    assert not all(np.array_equal(a, b) for a, b in zip(both(gpu_ctx, t)["rows"], one["rows"]))


# ---- MarkerSetSelection ----------------------------------------------------------------------------------------------------------------------------
def test_golden_nodes_with_host_draws(gpu_ctx, tmp_path):
    """random.uniform and sampleGenome on the host, scored by genomeChecks on the device: the reference's tuples."""
    sel, tree, nodes = selection_of(tmp_path, None)
    assert wanted_tuples(sel, tree, nodes, "host") == [tuple(n["tuple"]) for n in GOLDEN["nodes"]]
    assert sel.markerSetBuilder.last_sim_timing["device"]


def test_a_node_with_device_draws(gpu_ctx, tmp_path, monkeypatch):
    sel, tree, nodes = selection_of(tmp_path, None)
    got = wanted_tuples(sel, tree, nodes, "device")
    assert sel.markerSetBuilder.last_select_timing["device"] and sel.markerSetBuilder.last_select_timing["kernel"] > 0
    monkeypatch.setattr(_lib, "select_run", emu.select_run)
    assert wanted_tuples(sel, tree, nodes, "device") == got and any(t[0] != "NA" for t in got)


def test_a_threshold_word_that_two_contigs_share(gpu_ctx):
    """The two radix passes over the contig index run only where the threshold word repeats; see tied_tables."""
    for ncomp, first, second in ((TIE_RANK + 1, 1, 0), (TIE_RANK + 2, 1, 1), (TIE_RANK, 0, 0)):
        row = both(gpu_ctx, tied_tables(ncomp))["rows"][0][0]
        assert (int(row[TIE_CONTIGS[0]]), int(row[TIE_CONTIGS[1]])) == (first, second) and int(row.sum()) == ncomp
