"""The placement on the device: the kernels of libcheckm_hip (kernels_place.hip) against the host executor of the same arithmetic
(tests/emu/placement) at == -- the uint64 views of the mantissas, the exponents, the kept edges and the grid indices -- on the smallest
shapes that can still break: site counts around a wavefront and around the scan's LDS tile, trees of every shape the level schedule
distinguishes, query counts around a wavefront and beyond one workgroup of the scan, one to eight rates, branch lengths from zero to
ten, products far below the double range, maxPitches of one and of more than the edges, budgets that cut the sites into many chunks; the
recovery fixture through the real PplacerRunner.place; PplacerRunner.run on a small tree directory, then TreeParser."""
import os
import re

import numpy as np
import pytest

from checkm_amd import _lib, runtime
from checkm_amd.pplacer import PplacerRunner, RefPkg, log_likelihood
from tests.emu import placement as emu
from tests.emu import placement_oracle as orc
from tests.test_placement_host import ROOT, check_lineage_lines, check_recovery, emu_site_bytes, run_on_the_tree_directory, same_bits, synthetic, world      # noqa: F401

pytestmark = pytest.mark.gpu

_DEV_H = open(os.path.join(ROOT, "checkm_amd", "csrc", "place_dev.h")).read()
SCAN_SITES = int(re.search(r"SCAN_SITES = (\d+);", _DEV_H).group(1))          # what the scan chose to keep in LDS
SCAN_QUERIES = int(re.search(r"SCAN_QUERIES = (\d+);", _DEV_H).group(1))

PEND, FRAC = (0.01, 0.2, 1.5), (0.25, 0.75)


def queries_from(rng, aln, nsites, count):
    """count queries: copies of leaves with a tenth of the sites redrawn, then an all-gap one, one with a single residue, one in lower
    case and X, as far as count allows."""
    names = sorted(aln)
    letters = np.array(list("ARNDCQEGHILKMFPSTWYV-"))
    out = {}
    for k in range(count):
        s = np.array(list(aln[names[int(rng.integers(len(names)))]]))
        hit = rng.random(nsites) < 0.1
        s[hit] = rng.choice(letters, size=int(hit.sum()))
        out["q%04d" % k] = "".join(s)
    special = ["-" * nsites, "-" * (nsites // 2) + "W" + "-" * (nsites - nsites // 2 - 1), "".join("xX"[k % 2] if k % 3 else aln[names[0]][k].lower() for k in range(nsites))]
    for k, s in enumerate(special[:max(0, count - 1)]):
        out["q%04d" % (count - 1 - k)] = s
    return out


def same(gpu_ctx, t, budget_bytes=0):
    want, got = emu.place_run(None, t, budget_bytes), _lib.place_run(gpu_ctx, t, budget_bytes)
    same_bits(want, got)
    assert got["nchunks"] == want["nchunks"] and got["chunk_sites"] == want["chunk_sites"]
    nedges = t.nnodes - 1
    kept = min(nedges, t.max_pitches)
    assert (got["top_edge"][:, :kept] >= 0).all() and (got["top_edge"][:, kept:] == -1).all() and (got["ref_m"][:, :kept] > 0).all()
    return got


def tables(seed, tree_text, nsites, nqueries, rates=(0.3, 1.7), weights=(0.4, 0.6), pitches=3, pend=PEND, frac=FRAC):
    ref, aln, _ = synthetic(seed, tree_text, nsites, rates, weights)
    return PplacerRunner(1)._tables(ref, queries_from(np.random.default_rng(seed + 1000), aln, nsites, nqueries), pend, frac, 0.1, pitches)


def caterpillar(nleaves):
    text = "(a0:0.1,a1:0.2)"
    for k in range(2, nleaves):
        text = "(%s:0.05,a%d:0.1)" % (text, k)
    return text + ";"


def balanced(names):
    if len(names) == 1:
        return names[0]
    h = len(names) // 2
    return "(%s:0.1,%s:0.15)" % (balanced(names[:h]), balanced(names[h:]))


TREES = {
    "two_leaves": "(a:0.1,b:0.2);",
    "three_on_a_trifurcating_root": "(a:0.1,b:0.2,c:0.3);",
    "caterpillar_65": caterpillar(65),
    "balanced_64": balanced(["b%d" % k for k in range(64)]) + ";",
    "random_130": orc.random_tree(np.random.default_rng(130), 130, 0.01, 0.4, root_degree=3),
    "degree_5": "((a:0.1,b:0.2,c:0.1,d:0.3,e:0.2):0.1,(f:0.1,g:0.1):0.2,h:0.3);",
}


@pytest.mark.parametrize("nsites", [1, 63, 64, 65, SCAN_SITES - 1, SCAN_SITES, SCAN_SITES + 1])
def test_sites_at_the_wavefront_and_tile_edges(gpu_ctx, nsites):
    assert SCAN_SITES == 256
    same(gpu_ctx, tables(nsites, TREES["degree_5"], nsites, 5, pitches=4))


@pytest.mark.parametrize("name", sorted(TREES))
def test_trees(gpu_ctx, name):
    got = same(gpu_ctx, tables(len(name), TREES[name], 65, 4))
    levels = {"two_leaves": 2, "three_on_a_trifurcating_root": 2, "caterpillar_65": 65, "balanced_64": 7, "degree_5": 3}
    assert name not in levels or got["nlevels_up"] == levels[name]


@pytest.mark.parametrize("nqueries", [1, 63, 64, 65, 200, SCAN_QUERIES + 1])
def test_queries(gpu_ctx, nqueries):
    t = tables(nqueries, TREES["three_on_a_trifurcating_root"], 70, nqueries, rates=(1.0,), weights=(1.0,), pitches=2, pend=(0.1, 0.5), frac=(0.5,))
    got = same(gpu_ctx, t)
    if nqueries > 1:
        gaps = nqueries - 1                                        # the all-gap query: every edge ties, the lower edge number wins
        assert got["top_edge"][gaps].tolist() == [0, 1] and got["scan_m"][gaps, 0] == got["scan_m"][gaps, 1] and got["scan_e"][gaps, 0] == got["scan_e"][gaps, 1]
        assert got["ref_f"][gaps].tolist() == [0, 0] and got["ref_g"][gaps].tolist() == [0, 0]


@pytest.mark.parametrize("rates,weights", [((1.0,), (1.0,)), ((0.1, 0.5, 1.0, 2.4), (0.25, 0.25, 0.25, 0.25)),
                                           ((0.05, 0.2, 0.4, 0.7, 1.0, 1.5, 2.5, 4.0), (0.3, 0.2, 0.15, 0.1, 0.1, 0.05, 0.05, 0.05))])
def test_rates(gpu_ctx, rates, weights):
    same(gpu_ctx, tables(len(rates), TREES["degree_5"], 66, 4, rates=rates, weights=weights))


def test_a_branch_of_length_ten(gpu_ctx):
    same(gpu_ctx, tables(3, "((a:10.0,b:0.1):0.2,c:0.1,d:10);", 65, 4))


def test_zero_length_edges_with_identical_siblings(gpu_ctx):
    text = "((a:0.0,b:0.0):0.0,(c:0.1,d:0):0.2,e:0.3);"
    ref, aln, model = synthetic(4, text, 65)
    assert aln["a"] == aln["b"]                                    # nothing changes along an edge of length zero
    t = PplacerRunner(1)._tables(ref, queries_from(np.random.default_rng(9), aln, 65, 5), PEND, FRAC, 0.1, 7)
    same(gpu_ctx, t)


def test_products_far_below_the_double_range(gpu_ctx):
    t = tables(6, "(a:2.0,b:2.0,c:2.0);", 4096, 2, rates=(1.0,), weights=(1.0,), pitches=1, pend=(0.5,), frac=(0.5,))
    got = same(gpu_ctx, t)
    assert got["scan_e"][0, 0] < -4 * 1074 and 0.5 <= got["scan_m"][0, 0] < 1.0 and log_likelihood(got["ref_m"][0, 0], int(got["ref_e"][0, 0])) < -4 * 745


@pytest.mark.parametrize("pitches", [1, 1000])
def test_max_pitches(gpu_ctx, pitches):
    got = same(gpu_ctx, tables(pitches, TREES["degree_5"], 30, 3, pitches=pitches))
    assert got["top_edge"].shape == (3, pitches)


def test_budgets_and_repeats(gpu_ctx):
    t = tables(8, TREES["degree_5"], 3 * SCAN_SITES + 70, 6, pitches=4)
    one = same(gpu_ctx, t)
    again = _lib.place_run(gpu_ctx, t)
    same_bits(one, again)
    assert one["nchunks"] == 1
    for budget, chunks in ((1, 14), (200 * emu_site_bytes(t), 5), (600 * emu_site_bytes(t), 2)):
        cut = same(gpu_ctx, t, budget)
        same_bits(one, cut)
        assert cut["nchunks"] == chunks


def test_refused_on_the_host_before_any_launch(gpu_ctx):
    t = tables(2, TREES["two_leaves"], 10, 2)
    t.length[0] = -1.0
    with pytest.raises(_lib.CkmError) as e:
        _lib.place_run(gpu_ctx, t)
    assert e.value.code == -1
    t = tables(2, TREES["two_leaves"], 10, 2)
    t.child[1] = t.child[0]
    with pytest.raises(_lib.CkmError) as e:
        _lib.place_run(gpu_ctx, t)
    assert e.value.code == -1


def test_recovery_fixture_through_the_runner(gpu_ctx, monkeypatch):
    monkeypatch.setattr(runtime, "get_ctx", lambda: gpu_ctx)
    check_recovery(PplacerRunner(1).place)


def test_run_then_tree_parser(gpu_ctx, world, monkeypatch):      # noqa: F811
    monkeypatch.setattr(runtime, "get_ctx", lambda: gpu_ctx)
    check_lineage_lines(run_on_the_tree_directory(world))
