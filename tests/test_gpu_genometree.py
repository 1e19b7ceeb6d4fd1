"""The genome tree on the device: the kernels of libcheckm_hip (kernels_gtree.hip) against the host executor of the same header
(tests/emu/genometree) at == -- every count, the bits of every distance, every merge row -- on the smallest shapes that can still
break: row counts around the 64-row tile of the count kernel, column counts around the 8-byte word, the 16-byte padding and the
128-byte chunk (so that the rows of the caller's text start at every alignment), every kind of byte; joins around the wavefront of the
row minima and the 256 lanes of the sums, tied, duplicate and saturated matrices; replicate counts and budgets that cut them into
batches; the refusals; and the fixture end to end through GenomeTree, RefPkg and PplacerRunner."""
import random

import numpy as np
import pytest

from checkm_amd import _lib, runtime
from checkm_amd.genomeTree import GenomeTree
from checkm_amd.pplacer import PplacerRunner, RefPkg, nodes_of, parse_newick, plain_name
from tests.emu import genometree as emu
from tests.emu import placement_oracle as orc
from tests.test_genometree_host import AA, canon, evolved_case, inner

pytestmark = pytest.mark.gpu

SYMBOLS = AA + AA.lower() + "-.XBZJUO*~? xbzjuo@[`{0\x00\x7f"


def bits(a):
    return a.view(np.uint64) if a.dtype == np.float64 else a


def both(gpu_ctx, t, budget_bytes=0, **what):
    want, got = emu.gtree_run(None, t, budget_bytes, **what), _lib.gtree_run(gpu_ctx, t, budget_bytes, **what)
    for f in ("compared", "differ", "dist", "merge_ij", "merge_len"):
        assert (want[f] is None) == (got[f] is None)
        if want[f] is not None:
            assert want[f].shape == got[f].shape and np.array_equal(bits(want[f]), bits(got[f])), f
    assert got["nrounds"] == want["nrounds"] and got["ntrees"] == want["ntrees"]
    return got


def random_text(rng, n, ncols):
    """n rows of every kind of byte: residues in both cases, every non-residue symbol; row 0 with gaps only (two rows or more), row 1
    a copy of the last row in the other case."""
    sym = np.frombuffer(SYMBOLS.encode("latin-1"), dtype=np.uint8)
    text = sym[rng.randint(0, len(sym), (n, ncols))]
    mostly = rng.random_sample((n, ncols)) < 0.7                      # (most cells residues, so that the counts are not all tiny)
    text = np.where(mostly, np.frombuffer(AA.encode(), dtype=np.uint8)[rng.randint(0, 20, (n, ncols))], text)
    if n > 2:
        text[0] = ord("-")
        text[1] = np.frombuffer(text[n - 1].tobytes().swapcase(), dtype=np.uint8)
    return np.ascontiguousarray(text)


@pytest.mark.parametrize("n", [2, 3, 63, 64, 65, 129])
def test_counts_and_distances(gpu_ctx, n):
    rng = np.random.RandomState(n)
    for ncols in (1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 257):
        text = random_text(rng, n, ncols)
        for model in ("kimura", "poisson", "p"):
            t = _lib.GtreeTables(text=text.reshape(-1), nrows=n, ncols=ncols, model=model, max_dist=1.25)
            got = both(gpu_ctx, t, counts=True, dist=True, merges=(model == "kimura"))
        if n > 2:
            assert not got["compared"][0].any() and (got["dist"][0, 1:] == 1.25).all()
            assert got["differ"][1, n - 1] == 0 and got["compared"][1, n - 1] == got["compared"][1, 1]
        # the plain byte-wise statement of the counts
        up = np.frombuffer(text.tobytes().upper(), dtype=np.uint8).reshape(n, ncols)
        known = np.isin(up, np.frombuffer(AA.encode(), dtype=np.uint8))
        both_known = known[:, None, :] & known[None, :, :]
        assert np.array_equal(got["compared"], both_known.sum(axis=2)) and np.array_equal(got["differ"], (both_known & (up[:, None, :] != up[None, :, :])).sum(axis=2))


@pytest.mark.parametrize("n", [3, 4, 5, 63, 64, 65, 257])
def test_joins(gpu_ctx, n):
    rng = np.random.RandomState(1000 + n)
    sym = lambda m: np.triu(m, 1) + np.triu(m, 1).T
    rand = sym(rng.uniform(0.1, 1.0, (n, n)))
    equal = np.ones((n, n)) - np.eye(n)
    dup = rand.copy()                                                   # rows 0 and n - 1 identical: distance 0, the same distances to the rest
    dup[n - 1, :], dup[:, n - 1] = dup[0, :], dup[:, 0]
    dup[0, n - 1] = dup[n - 1, 0] = dup[n - 1, n - 1] = 0.0
    sat = np.full((n, n), 3.0) - 3.0 * np.eye(n)                        # maxDist everywhere but one pair
    sat[1, 2] = sat[2, 1] = 0.25
    got = both(gpu_ctx, _lib.GtreeTables(matrices=np.stack([rand, equal, dup, sat])))
    for k in range(4):
        ij = got["merge_ij"][k]
        assert (ij[:, 0] < ij[:, 1]).all() and sorted(ij[:, 1].tolist()) == list(range(1, n)) and (got["merge_len"][k] >= 0.0).all()
    if n > 4:
        assert got["merge_ij"][1][0].tolist() == [0, 1] and got["merge_ij"][3][0].tolist() == [1, 2]


@pytest.mark.parametrize("nreps", [0, 1, 5])
def test_replicates_and_budgets(gpu_ctx, nreps):
    n, ncols = 21, 130
    rng = np.random.RandomState(77 + nreps)
    text = random_text(rng, n, ncols)
    text[0] = text[2]                                                   # (no all-gap row here: it would tie every replicate's joins)
    cols = rng.randint(0, ncols, (nreps, ncols)) if nreps else None
    t = _lib.GtreeTables(text=text.reshape(-1), nrows=n, ncols=ncols, cols=cols, model="kimura")
    per_tree = n * 144 + n * n * 16 + n * 64
    trees = 1 + nreps
    whole = both(gpu_ctx, t, budget_bytes=per_tree * trees)
    assert whole["nrounds"] == 1 and whole["merge_ij"].shape == (trees, n - 1, 2)
    for budget, rounds in ((per_tree * 3, (trees + 2) // 3), (1, trees)):
        cut = both(gpu_ctx, t, budget_bytes=budget)
        assert cut["nrounds"] == rounds
        assert np.array_equal(cut["merge_ij"], whole["merge_ij"]) and np.array_equal(bits(cut["merge_len"]), bits(whole["merge_len"]))
    if nreps:
        # the replicates alone: 5 of them in 1, 2 and 5 rounds
        alone = _lib.GtreeTables(text=text.reshape(-1), nrows=n, ncols=ncols, cols=cols, base=False, model="kimura")
        for budget, rounds in ((per_tree * nreps, 1), (per_tree * 3, (nreps + 2) // 3), (1, nreps)):
            only = both(gpu_ctx, alone, budget_bytes=budget)
            assert only["nrounds"] == rounds
            assert np.array_equal(only["merge_ij"], whole["merge_ij"][1:]) and np.array_equal(bits(only["merge_len"]), bits(whole["merge_len"][1:]))


def test_refused_on_the_host_before_any_launch(gpu_ctx):
    N, L = _lib.GTREE_MAX_ROWS, _lib.GTREE_MAX_COLS
    for bad in (_lib.GtreeTables(text=np.full(N + 1, 65, dtype=np.uint8), nrows=N + 1, ncols=1),
                _lib.GtreeTables(text=np.full(2 * (L + 1), 65, dtype=np.uint8), nrows=2, ncols=L + 1),
                _lib.GtreeTables(text=np.array([65, 65, 65, 255], dtype=np.uint8), nrows=2, ncols=2)):
        with pytest.raises(_lib.CkmError) as e:
            _lib.gtree_run(gpu_ctx, bad)
        assert e.value.code == -7
    ok = _lib.GtreeTables(text=np.full(2 * L, 65, dtype=np.uint8), nrows=2, ncols=L)          # the limit itself is taken
    got = both(gpu_ctx, ok, counts=True)
    assert got["compared"][0, 1] == L and got["differ"][0, 1] == 0


def test_end_to_end_on_the_evolved_fixture(gpu_ctx, monkeypatch):
    monkeypatch.setattr(runtime, "get_ctx", lambda: gpu_ctx)
    ids, seqs, truth = evolved_case()
    gt, n = GenomeTree(), len(ids)
    text = gt.infer(seqs, model="poisson")
    random.seed(11)
    supported = gt.bootstrap(seqs, text, numBootstraps=20, model="poisson")
    root = parse_newick(supported)
    clade = GenomeTree._clades(root, {name: k for k, name in enumerate(ids)})
    seen = {canon(clade[v], n): float(v.name) for v in nodes_of(root) if v.children and v.parent is not None}
    assert set(seen) == inner(truth, n) and min(seen.values()) > 0.5
    random.seed(11)
    assert supported == GenomeTree(runner=emu.runner).bootstrap(seqs, text, numBootstraps=20, model="poisson")
    # the text loads in RefPkg with the placement tests' synthetic model; a copy of a leaf's row lands on the leaf's own pendant edge
    S, pi = orc.random_model(np.random.default_rng(7))
    ref = RefPkg(supported, seqs, S, pi, (0.3, 1.7), (0.4, 0.6))
    leaf = [v for v in ref.nodes if not v.children and plain_name(v.name) == "g05"][0]
    placed = PplacerRunner(1).place(ref, {"copy": seqs["g05"]})["copy"]
    assert placed[0][0] == leaf.num
