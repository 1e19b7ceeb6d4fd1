"""MarkerSetBuilder on the device: the marker pass and the co-location pass of libcheckm_hip (kernels_markerset.hip) against the host
executor of the same arithmetic (tests/emu/markerset) at ==, on the smallest shapes that can still break -- the tile edges of the marker
lists, the chunk edges of the genome lists, more than one block of families, copies beyond the first, many unequal queries in one call,
budgets that cut the work into rounds and batches -- and the golden cases of the reference through the real MarkerSetBuilder."""
import numpy as np
import pytest

from checkm_amd import _lib, runtime
from tests.emu import markerset as emu
from tests.test_markerset_host import CASES, check_case, plain_colocated, synthetic_table, triples

pytestmark = pytest.mark.gpu

G, C = 66, 130
MARKERS = (1, 2, 63, 64, 65, 129)
GENOMES = (0, 1, 2, 64, 65)


@pytest.fixture(scope="module")
def world(gpu_ctx):
    """One table on the device and in the host executor, and the queries of every (markers, genomes) shape."""
    arrays = synthetic_table(21, G, C)
    rng = np.random.default_rng(22)
    glists, mlists = [], []
    for nm in MARKERS:
        for ng in GENOMES:
            glists.append(rng.permutation(G)[:ng].tolist())                 # overlapping lists, in no order
            mlists.append(rng.permutation(C)[:nm].tolist())
    dev, host = _lib.MsetTable(gpu_ctx, *arrays), emu.MsetTable(None, *arrays)
    yield dict(arrays=arrays, dev=dev, host=host, glists=glists, mlists=mlists)
    dev.close()


def same(a, b):
    assert a["tests"] == b["tests"] and a["npairs"] == b["npairs"]
    for k in ("pair_off", "i", "j", "count"):
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("families", [1, 64, 65, 300])
def test_marker_pass(gpu_ctx, families):
    arrays = synthetic_table(30 + families, G, families)
    dev, host = _lib.MsetTable(gpu_ctx, *arrays), emu.MsetTable(None, *arrays)
    try:
        rng = np.random.default_rng(families)
        for nq in (1, 3, 70):
            glists = [rng.permutation(G)[:GENOMES[q % 5] if q < 10 else int(rng.integers(0, G + 1))].tolist() for q in range(nq)]
            if nq == 70:
                glists[11] = list(range(G)) * 5                             # more than one chunk of the staged genome list; genomes repeated
            tU = [float(rng.choice([0.0, 0.5, 0.97, 1.0])) * len(g) for g in glists]
            tS = [float(rng.choice([0.0, 0.3, 0.97])) * len(g) for g in glists]
            want = emu.mset_markers(None, host, glists, tU, tS, want_counts=True)
            got = _lib.mset_markers(gpu_ctx, dev, glists, tU, tS, want_counts=True)
            assert np.array_equal(got["flag"], want["flag"]) and np.array_equal(got["counts"], want["counts"])
            assert nq < 70 or len(set(want["flag"].reshape(-1).tolist())) > 1
            plain = _lib.mset_markers(gpu_ctx, dev, glists, tU, tS)
            assert plain["counts"] is None and np.array_equal(plain["flag"], want["flag"])
            cut = _lib.mset_markers(gpu_ctx, dev, glists, tU, tS, want_counts=True, budget_bytes=13 * families * 2)       # two queries per launch
            assert cut["nbatches"] == (nq + 1) // 2 and np.array_equal(cut["flag"], want["flag"]) and np.array_equal(cut["counts"], want["counts"])
    finally:
        dev.close()


def test_colocated_every_shape_in_one_call(gpu_ctx, world):
    w = world
    want = emu.mset_colocated(None, w["host"], w["glists"], w["mlists"], 5000, 0.5)
    got = _lib.mset_colocated(gpu_ctx, w["dev"], w["glists"], w["mlists"], 5000, 0.5)
    same(got, want)
    assert got["npairs"] > 1000 and got["nrounds"] == 1 and got["nbatches"] == 1
    per_query = np.diff(got["pair_off"].astype(np.int64)).reshape(len(MARKERS), len(GENOMES))
    assert not per_query[0].any() and not per_query[:, 0].any() and per_query[2:, 1:].all()          # one marker, no genome: nothing; 63 markers or more: something
    # the multi-copy walk decided some of them: with the first copies alone the result differs
    cls, pos_off, pos = w["arrays"]
    q = len(GENOMES) * 2 + 4                                                  # 63 markers, 65 genomes
    assert triples(got, q) == plain_colocated(cls, pos_off, pos, w["glists"][q], w["mlists"][q], 5000, 0.5)
    keep = np.zeros(pos.shape[0], dtype=bool)
    keep[pos_off[:-1][np.diff(pos_off.astype(np.int64)) > 0].astype(np.int64)] = True
    first_off = np.zeros_like(pos_off)
    np.cumsum(np.minimum(np.diff(pos_off.astype(np.int64)), 1), out=first_off[1:])
    assert triples(got, q) != plain_colocated(cls, first_off, pos[keep], w["glists"][q], w["mlists"][q], 5000, 0.5)


@pytest.mark.parametrize("nq", [1, 3, 70])
def test_colocated_queries_in_one_call(gpu_ctx, world, nq):
    w = world
    rng = np.random.default_rng(nq)
    pick = [len(GENOMES) * 5 + 4] if nq == 1 else rng.integers(0, len(w["glists"]), size=nq).tolist()      # 129 markers, 65 genomes alone
    glists, mlists = [w["glists"][k] for k in pick], [w["mlists"][k] for k in pick]
    same(_lib.mset_colocated(gpu_ctx, w["dev"], glists, mlists, 5000, 0.5), emu.mset_colocated(None, w["host"], glists, mlists, 5000, 0.5))


def test_colocated_budgets_and_repeats(gpu_ctx, world):
    w = world
    one = _lib.mset_colocated(gpu_ctx, w["dev"], w["glists"], w["mlists"], 5000, 0.5)
    again = _lib.mset_colocated(gpu_ctx, w["dev"], w["glists"], w["mlists"], 5000, 0.5)
    same(again, one)
    for budget in (1, 3000, 40000):
        cut = _lib.mset_colocated(gpu_ctx, w["dev"], w["glists"], w["mlists"], 5000, 0.5, budget_bytes=budget)
        same(cut, one)
        assert cut["nbatches"] >= 3 and cut["nrounds"] >= 3, budget
    # other thresholds: nothing near, everything near, every pair reported
    for D, thr in ((0, 0.0), (2**31 - 1, 0.99), (5000, -1.0), (4999, 0.25)):
        same(_lib.mset_colocated(gpu_ctx, w["dev"], w["glists"][20:], w["mlists"][20:], D, thr), emu.mset_colocated(None, w["host"], w["glists"][20:], w["mlists"][20:], D, thr))


def test_refused_on_the_host_before_any_launch(gpu_ctx, world):
    cls, pos_off, pos = world["arrays"]
    big = pos.copy(); big[7] = 2**31
    with pytest.raises(_lib.CkmError) as e:
        _lib.MsetTable(gpu_ctx, cls, pos_off, big)
    assert e.value.code == -7
    for bad in (dict(dist_threshold=4999.5), dict(dist_threshold=2.0**31)):
        with pytest.raises(_lib.CkmError):
            _lib.mset_colocated(gpu_ctx, world["dev"], [[0, 1]], [[0, 1]], **bad)
    with pytest.raises(_lib.CkmError) as e:
        _lib.mset_colocated(gpu_ctx, world["dev"], [[0, G]], [[0, 1]])
    assert e.value.code == -1
    with pytest.raises(_lib.CkmError):
        _lib.mset_markers(gpu_ctx, world["dev"], [[G]], [1.0], [1.0])
    empty = _lib.mset_colocated(gpu_ctx, world["dev"], [], [])
    assert empty["npairs"] == 0 and empty["pair_off"].tolist() == [0]


@pytest.mark.parametrize("name", sorted(CASES))
def test_golden_case_through_the_class(gpu_ctx, name, tmp_path, monkeypatch):
    monkeypatch.setattr(runtime, "get_ctx", lambda: gpu_ctx)
    check_case(CASES[name], str(tmp_path))
    if CASES[name]["error"] is None:
        check_case(CASES[name], str(tmp_path / "batch"), batch=True)
