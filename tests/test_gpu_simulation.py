"""The marker-set simulation on the device: sim_kernel of libcheckm_hip (kernels_sim.hip) against the host executor of the same arithmetic
(tests/emu/simulation) at ==, on the smallest shapes that can still break -- start lists around a wavefront and just beyond the LDS
staging size, marker counts around a wavefront and beyond the LDS counts, co-located sets around the sixty-four a wavefront takes at a
time, more marker sets than wavefronts, many replicates with mixed contig lengths in one launch, budgets that cut the call into rounds --
and the golden cases of the reference through the real MarkerSetBuilder.genomeChecks and Simulation."""
import os
import re

import numpy as np
import pytest

from checkm_amd import _lib, runtime
from tests.emu import simulation as emu
from tests.test_simulation_host import CASES, ROOT, check_case

pytestmark = pytest.mark.gpu

_DEV_H = open(os.path.join(ROOT, "checkm_amd", "csrc", "sim_dev.h")).read()
SIM_STAGE_STARTS = int(re.search(r"STAGE_STARTS = (\d+);", _DEV_H).group(1))        # what the kernel chose to keep in LDS
SIM_STAGE_COUNTS = int(re.search(r"STAGE_COUNTS = (\d+);", _DEV_H).group(1))

SPAN = 300000
LENS = (1, 700, 1000, 5000, 2**31 - 1)


def random_tables(seed, nmarkers, cs_per_set, starts_per_replicate):
    """A call as arrays: markers with none to five copies in [0, SPAN) (a few at the ends of the int32 range), co-located sets of one to
    seven members drawn from all markers (so markers repeat within a marker set), sorted starts with repeats, contig lengths from LENS."""
    rng = np.random.default_rng(seed)
    ncopy = rng.choice([0, 1, 1, 1, 1, 2, 3, 5], size=nmarkers)
    key = rng.integers(0, SPAN, size=int(ncopy.sum()), dtype=np.int64)
    if key.size > 4:
        key[0], key[1], key[2] = 0, 2**31 - 1, 2**31 - 2
    sizes = rng.choice([1, 1, 2, 3, 7], size=int(np.sum(cs_per_set)))
    starts = []
    for n in starts_per_replicate:
        s = np.where(rng.random(n) < 0.5, rng.integers(0, SPAN, size=n), rng.integers(0, SPAN // 1000, size=n) * 1000)
        if n > 2:
            s[1] = s[0]
        starts.append(np.sort(s))
    off = lambda lens: np.concatenate([np.zeros(1, dtype=np.uint64), np.cumsum(lens, dtype=np.uint64)])
    return _lib.SimTables(off(ncopy), key, off(cs_per_set), off(sizes), rng.integers(0, nmarkers, size=int(sizes.sum())), off(starts_per_replicate),
                          np.concatenate(starts) if starts else [], rng.choice(LENS, size=len(starts_per_replicate)))


def same(gpu_ctx, tables, budget_bytes=0):
    want, got = emu.sim_run(None, tables, budget_bytes), _lib.sim_run(gpu_ctx, tables, budget_bytes)
    assert got["out"].dtype == np.float64 and got["out"].shape == want["out"].shape
    assert np.array_equal(got["out"].view(np.uint64), want["out"].view(np.uint64)) and got["nrounds"] == want["nrounds"]
    assert not np.isnan(want["out"]).any()
    return got


def test_start_lists_at_the_staging_edges(gpu_ctx):
    assert SIM_STAGE_STARTS == 6144
    got = same(gpu_ctx, random_tables(1, 65, [1, 64, 65], [0, 1, 63, 64, 65, SIM_STAGE_STARTS, SIM_STAGE_STARTS + 1]))
    assert not got["out"][0].any() and got["out"][5:].max() > 100.0                 # no start: nothing; thousands of starts: contamination


@pytest.mark.parametrize("nmarkers", [1, 63, 64, 65, 300, SIM_STAGE_COUNTS, SIM_STAGE_COUNTS + 1])
def test_markers(gpu_ctx, nmarkers):
    same(gpu_ctx, random_tables(10 + nmarkers, nmarkers, [3, 65, 1], [40, 0, 200, SIM_STAGE_STARTS + 1]))


@pytest.mark.parametrize("ncs", [1, 64, 65, 400])
def test_colocated_sets_per_marker_set(gpu_ctx, ncs):
    got = same(gpu_ctx, random_tables(20 + ncs, 300, [ncs, 1, ncs], [150, 7]))
    assert ncs == 1 or len(set(got["out"][0, 0].tolist())) == 4


@pytest.mark.parametrize("nsets", [1, 3, 70])
def test_marker_sets(gpu_ctx, nsets):
    rng = np.random.default_rng(nsets)
    same(gpu_ctx, random_tables(30 + nsets, 130, rng.integers(1, 90, size=nsets).tolist(), [90, 3, 0]))


@pytest.mark.parametrize("nreplicates", [1, 2, 3600])
def test_replicates_in_one_launch(gpu_ctx, nreplicates):
    rng = np.random.default_rng(nreplicates)
    tables = random_tables(40 + nreplicates, 65, [5, 66], rng.choice([0, 1, 5, 63, 64, 65, 130], size=nreplicates).tolist())
    got = same(gpu_ctx, tables)
    assert got["nrounds"] == 1 and (nreplicates < 3600 or len(set(tables.contig_len.tolist())) == len(LENS))


def test_budgets_and_repeats(gpu_ctx):
    tables = random_tables(50, SIM_STAGE_COUNTS + 1, [70, 3], [10, 0, 65, 300, 64, 1, 2])       # the counts in the blocks' scratch rows
    one = same(gpu_ctx, tables)
    again = _lib.sim_run(gpu_ctx, tables)
    assert np.array_equal(again["out"], one["out"]) and one["nrounds"] == 1
    for budget in (1, 40000, 70000):
        cut = same(gpu_ctx, tables, budget)
        assert np.array_equal(cut["out"], one["out"]) and (cut["nrounds"] == 7 if budget == 1 else 1 < cut["nrounds"] < 7), budget
    small = random_tables(51, 65, [5], [3] * 9)
    assert same(gpu_ctx, small, 1)["nrounds"] == 9


def test_refused_on_the_host_before_any_launch(gpu_ctx):
    t = random_tables(60, 10, [2], [4, 4])
    t.starts[5], t.starts[6] = 9, 3
    with pytest.raises(_lib.CkmError) as e:
        _lib.sim_run(gpu_ctx, t)
    assert e.value.code == -1
    t = random_tables(60, 10, [2], [4, 4])
    t.key[0] = 2**31
    with pytest.raises(_lib.CkmError) as e:
        _lib.sim_run(gpu_ctx, t)
    assert e.value.code == -7
    empty = _lib.sim_run(gpu_ctx, random_tables(61, 10, [2], []))
    assert empty["out"].shape == (0, 1, 4) and empty["nrounds"] == 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_golden_case_through_the_classes(gpu_ctx, name, monkeypatch):
    monkeypatch.setattr(runtime, "get_ctx", lambda: gpu_ctx)
    check_case(CASES[name])
