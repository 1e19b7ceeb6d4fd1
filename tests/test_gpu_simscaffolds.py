"""The scaffold simulation on the device: simscaf_kernel of libcheckm_hip (kernels_simscaf.hip) against the host executor of the same
arithmetic (tests/emu/simscaf) on uint64 views at ==, on the smallest shapes that can still break -- genomes of 1 to 65 scaffolds and
just at and beyond the LDS staging size of a bit row, marker counts around a wavefront and beyond the LDS counts, co-located sets around
the sixty-four a wavefront takes at a time, more marker sets than wavefronts, many replicates with mixed contaminants in one launch,
empty and full bit rows, a genome contaminating itself, budgets that cut the call into rounds -- and the golden cases of the reference
through the real MarkerSetBuilder.scaffoldChecks and SimulationScaffolds."""
import os
import re

import numpy as np
import pytest

from checkm_amd import _lib, runtime
from tests.emu import simscaf as emu
from tests.test_simscaffolds_host import CASES, MODES, ROOT, builder_of, check_case

pytestmark = pytest.mark.gpu

STAGE_BITS = int(re.search(r"STAGE_BITS = (\d+);", open(os.path.join(ROOT, "checkm_amd", "csrc", "simscaf_dev.h")).read()).group(1))      # what the kernel keeps in LDS
STAGE_COUNTS = int(re.search(r"STAGE_COUNTS = (\d+);", open(os.path.join(ROOT, "checkm_amd", "csrc", "sim_dev.h")).read()).group(1))
NONE = _lib.SIMSCAF_NONE
EDGES = [1, 31, 32, 33, 63, 64, 65, STAGE_BITS, STAGE_BITS + 1]


def random_tables(seed, nscaf, nmarkers, cs_per_set, replicates):
    """A call as arrays: per (genome, marker) cell none to five copies on scaffolds drawn at random (so copies share scaffolds, and the
    last scaffold of a genome is used), co-located sets of one to seven members drawn from all markers (so markers repeat within a marker
    set).  replicates: (test genome, contaminant or NONE, fill) with fill 'half', 'zero' or 'one' for both bit rows."""
    rng = np.random.default_rng(seed)
    G = len(nscaf)
    ncopy = rng.choice([0, 1, 1, 1, 1, 2, 3, 5], size=G * nmarkers)
    sc = np.concatenate([rng.integers(0, nscaf[g], size=int(ncopy[g * nmarkers:(g + 1) * nmarkers].sum())) for g in range(G)] + [np.zeros(0, dtype=np.int64)])
    start = 0
    for g in range(G):                                                                # a copy on the last scaffold of every genome that has copies
        n = int(ncopy[g * nmarkers:(g + 1) * nmarkers].sum())
        if n:
            sc[start] = nscaf[g] - 1
        start += n
    sizes = rng.choice([1, 1, 2, 3, 7], size=int(np.sum(cs_per_set)))

    def row(g, fill):
        n, w = nscaf[g], (nscaf[g] + 31) // 32
        bits = np.zeros(w * 32, dtype=bool)
        bits[:n] = rng.random(n) < 0.5 if fill == "half" else fill == "one"
        return np.packbits(bits.reshape(w, 32), axis=1, bitorder="little").view("<u4").reshape(w)

    rows, lens = [], []
    for g, h, fill in replicates:
        mine = [row(g, fill)] + ([row(h, fill)] if h != NONE else [])
        rows += mine
        lens.append(sum(r.size for r in mine))
    off = lambda n: np.concatenate([np.zeros(1, dtype=np.uint64), np.cumsum(n, dtype=np.uint64)])
    return _lib.SimScafTables(nscaf, nmarkers, off(ncopy), sc, off(cs_per_set), off(sizes), rng.integers(0, nmarkers, size=int(sizes.sum())),
                              [r[0] for r in replicates], [r[1] for r in replicates], off(lens), np.concatenate(rows) if rows else [])


def same(gpu_ctx, tables, budget_bytes=0):
    want, got = emu.simscaf_run(None, tables, budget_bytes), _lib.simscaf_run(gpu_ctx, tables, budget_bytes)
    assert got["out"].dtype == np.float64 and got["out"].shape == want["out"].shape
    assert np.array_equal(got["out"].view(np.uint64), want["out"].view(np.uint64)) and got["nrounds"] == want["nrounds"]
    assert not np.isnan(want["out"]).any()
    return got


def test_scaffolds_at_the_word_and_staging_edges(gpu_ctx):
    assert STAGE_BITS == 32768 and STAGE_COUNTS == 4096
    G = len(EDGES)
    replicates = [(g, (g + 1) % G, "half") for g in range(G)] + [(g, NONE, "half") for g in range(G)] + [(G - 1, G - 1, "half"), (G - 2, G - 1, "one"), (G - 1, G - 2, "one")]
    got = same(gpu_ctx, random_tables(1, EDGES, 65, [1, 64, 65], replicates))
    assert got["out"][:, :, 0].max() > 50.0 and got["out"][-1, :, 1].max() > 0.0


def test_empty_and_full_bit_rows_and_a_genome_contaminating_itself(gpu_ctx):
    nscaf = [33, 64, 7]
    tables = random_tables(2, nscaf, 130, [5, 66], [(0, 1, "zero"), (0, 1, "one"), (1, NONE, "one"), (1, NONE, "zero"), (2, 2, "one"), (2, NONE, "one"), (0, 0, "half")])
    got = same(gpu_ctx, tables)["out"]
    assert not got[0].any() and not got[3].any() and got[1].all()
    assert np.all(got[4, :, 0] == got[5, :, 0]) and np.all(got[4, :, 1] > got[5, :, 1])     # its own scaffolds twice: as complete, more contaminated


@pytest.mark.parametrize("nmarkers", [1, 63, 64, 65, STAGE_COUNTS, STAGE_COUNTS + 1])
def test_markers(gpu_ctx, nmarkers):
    same(gpu_ctx, random_tables(10 + nmarkers, [40, 3, 65], nmarkers, [3, 65, 1], [(0, 1, "half"), (2, NONE, "half"), (1, 2, "one"), (2, 0, "half")]))


@pytest.mark.parametrize("ncs", [1, 64, 65, 400])
def test_colocated_sets_per_marker_set(gpu_ctx, ncs):
    got = same(gpu_ctx, random_tables(20 + ncs, [90, 20], 300, [ncs, 1, ncs], [(0, 1, "half"), (1, NONE, "half")]))
    assert ncs == 1 or len(set(got["out"][0, 0].tolist())) == 4


@pytest.mark.parametrize("nsets", [1, 3, 70])
def test_marker_sets(gpu_ctx, nsets):
    rng = np.random.default_rng(nsets)
    same(gpu_ctx, random_tables(30 + nsets, [50, 33], 130, rng.integers(1, 90, size=nsets).tolist(), [(0, 1, "half"), (1, 0, "half"), (0, NONE, "zero")]))


@pytest.mark.parametrize("nreplicates", [1, 2, 3600])
def test_replicates_in_one_launch(gpu_ctx, nreplicates):
    rng = np.random.default_rng(nreplicates)
    nscaf = [1, 31, 33, 64, 65, 130]
    conts = rng.choice([NONE, 0, 1, 2, 3, 4, 5], size=nreplicates).tolist()
    tables = random_tables(40 + nreplicates, nscaf, 65, [5, 66], [(int(rng.integers(0, 6)), int(h), "half") for h in conts])
    got = same(gpu_ctx, tables)
    assert got["nrounds"] == 1 and (nreplicates < 3600 or len(set(conts)) == 7)


def test_budgets_and_repeats(gpu_ctx):
    replicates = [(0, 1, "half"), (1, NONE, "half"), (2, 0, "half"), (0, 0, "one"), (1, 2, "half"), (2, NONE, "zero"), (0, 2, "half")]
    tables = random_tables(50, [300, 64, 2000], STAGE_COUNTS + 1, [70, 3], replicates)      # the counts in the blocks' scratch rows
    one = same(gpu_ctx, tables)
    again = _lib.simscaf_run(gpu_ctx, tables)
    assert np.array_equal(again["out"], one["out"]) and one["nrounds"] == 1
    for budget in (1, 40000, 70000):
        cut = same(gpu_ctx, tables, budget)
        assert np.array_equal(cut["out"], one["out"]) and (cut["nrounds"] == 7 if budget == 1 else 1 < cut["nrounds"] < 7), budget
    small = random_tables(51, [40, 5], 65, [5], [(0, 1, "half")] * 9)
    assert same(gpu_ctx, small, 1)["nrounds"] == 9


def test_refused_on_the_host_before_any_launch(gpu_ctx):
    t = random_tables(60, [40, 5], 10, [2], [(0, 1, "half"), (1, NONE, "half")])
    t.sc[0] = 40
    with pytest.raises(_lib.CkmError) as e:
        _lib.simscaf_run(gpu_ctx, t)
    assert e.value.code == -1
    t = random_tables(60, [40, 5], 10, [2], [(0, 1, "half"), (1, NONE, "half")])
    t.bits[1] |= 1 << 8                                                              # bit 40 of a genome of 40 scaffolds
    with pytest.raises(_lib.CkmError) as e:
        _lib.simscaf_run(gpu_ctx, t)
    assert e.value.code == -1
    t = random_tables(60, [40, 5], 10, [2], [(0, 1, "half"), (1, NONE, "half")])
    t.cont[0] = 2
    with pytest.raises(_lib.CkmError) as e:
        _lib.simscaf_run(gpu_ctx, t)
    assert e.value.code == -1
    t = random_tables(60, [40, 2**30 + 1], 10, [2], [])
    with pytest.raises(_lib.CkmError) as e:
        _lib.simscaf_run(gpu_ctx, t)
    assert e.value.code == -7
    empty = _lib.simscaf_run(gpu_ctx, random_tables(61, [40, 5], 10, [2], []))
    assert empty["out"].shape == (0, 1, 4) and empty["nrounds"] == 0


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(CASES))
def test_golden_case_through_the_classes(gpu_ctx, name, mode, monkeypatch, tmp_path):
    monkeypatch.setattr(runtime, "get_ctx", lambda: gpu_ctx)
    c = CASES[name]
    check_case(builder_of(tmp_path, c), c, mode)
