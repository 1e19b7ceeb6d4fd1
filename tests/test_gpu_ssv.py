"""The SSV kernel (checkm_amd/csrc/kernels_ssv.hip) against the plain reference of tests/ssv_reference.py, launched the way the search
launches it (ckm_debug_ssv): Smax and the route of the fused finish, per pair, for every launch class -- the 8-lane instances, the
16-lane instances the search reaches, and the 16-lane instances of short models that only `lanes=16` reaches.

Per class: a model at each edge of the class (tests/ssv_reference.py: launch_classes) against noise, degenerate records, planted and
restarted domains and fragments that fill the band between noise and overflow; the coverage condition is asserted on the reference
before anything is compared.  Per model: nine list lengths around the wavefront and the block size (per_block overrides) plus one call
with the search's own block size, each in three list orders.  Every call is compared with the same per-pair reference, so Smax and route
are also shown to be independent of the wavefront slot, the round, the block and the list order.  All comparisons are exact."""
import numpy as np
import pytest

from checkm_amd import _lib
from tests import common
from tests import ssv_reference as R

pytestmark = pytest.mark.gpu

POOL = 280          # list entries per model: copies of its records (2 * per_block + 3 of the largest override, per_block + 9 of the largest default)
CLASSES = R.launch_classes()


@pytest.fixture(scope="module")
def ssv_world(gpu_ctx):
    w = R.World.get()
    prof = _lib.Profiles(gpu_ctx, w.path)
    state = dict(ctx=gpu_ctx, w=w, prof=prof, seqs={}, oracle={}, exact_checked=set())
    yield state
    for s in state["seqs"].values():
        s.close()
    prof.close()


def _model_state(st, M):
    """The sequence set of model M (POOL entries cycling through its records) and the oracle's MSV stage of its records."""
    if M not in st["seqs"]:
        recs = st["w"].recs[M]
        pool = [("%s_c%d" % (recs[i % len(recs)][0], i // len(recs)), "", recs[i % len(recs)][1]) for i in range(POOL)]
        st["seqs"][M] = _lib.Seqs(st["ctx"], [pool])
        st["oracle"][M] = st["w"].hs.msv_stage(st["w"].index[M], st["w"].dsq[M])
    return st["seqs"][M], st["oracle"][M]


def _orders(w, M):
    """Three orders of the POOL list entries: longest first (the search's), shortest first, and a fixed permutation whose head holds
    one wavefront with the ~3100-residue sequence among sequences of at most 2 residues (entries 0..7; 0..3 for four per wavefront)
    and, for the 8-lane kernel, an overflowing hit and an all-X record in one DPP row in both slot orders (entries 8, 9 and 10, 11)."""
    recs, dec = w.recs[M], w.decisions[M]
    n = len(recs)
    L = np.array([dec[i % n].L for i in range(POOL)])
    desc = np.argsort(-L, kind="stable")
    asc = np.argsort(L, kind="stable")
    names = [r[0] for r in recs]
    tiny = [i for i, nm in enumerate(names) if nm.startswith("tiny_")]
    long_ = next(i for i, nm in enumerate(names) if nm.startswith("r3100"))
    allx = names.index("deg_allx")
    hit = max(range(n), key=lambda i: (dec[i].overflow, dec[i].smax, -dec[i].L))
    head = tiny[:3] + [long_] + tiny[3:7] + [hit, allx, allx + n, hit + n]
    assert len(set(head)) == 12 and all(dec[i % n].L <= 2 for i in tiny) and dec[long_].L >= 3000
    perm = np.random.default_rng(600 + M).permutation(POOL)
    for t, r in enumerate(head):
        j = int(np.nonzero(perm == r)[0][0])
        perm[t], perm[j] = perm[j], perm[t]
    return [("longest first", desc), ("shortest first", asc), ("permutation", perm)], dec[hit].overflow


def _run_model(st, label, lanes, Q, M):
    w, ctx, prof = st["w"], st["ctx"], st["prof"]
    seqs, (o_xJ, o_sc, _o_pass) = _model_state(st, M)
    dec = w.decisions[M]
    n = len(dec)
    model = w.index[M]
    want_smax = np.array([dec[i % n].smax for i in range(POOL)], dtype=np.int64)
    want_route = np.array([dec[i % n].route for i in range(POOL)], dtype=np.int64)
    want_bits = np.array([common.float_bits(o_sc[i % n]) for i in range(POOL)], dtype=np.uint32)
    lens = np.array([dec[i % n].L for i in range(POOL)])
    _s, _r, _u, info = _lib.debug_ssv(ctx, prof, seqs, model, [0], 0, lanes)
    eight = info["cls"] >= 100
    assert info["cls"] == (100 + Q if eight else Q) and eight == (lanes == 0 and M <= 512), (label, M, info)
    s = 8 if eight else 4
    nwaves = info["threads"] // 64
    pb0 = info["per_block"]
    assert pb0 == nwaves * s * 4
    pbo = nwaves * s + 2 * s + 1                  # an override: a second round for some wavefronts, blocks that do not start on a wavefront boundary
    shapes = [(c, 0) for c in (1, s - 1, s, s + 1, 2 * s + 1)] + [(c, pbo) for c in (pbo - 1, pbo, pbo + 1, 2 * pbo + 3)] + [(pb0 + s + 1, 0)]
    assert max(c for c, _pb in shapes) <= POOL
    orders, hit_overflows = _orders(w, M)
    if eight and M >= 32:
        assert hit_overflows, (label, M)
    bad = []
    for oname, order in orders:
        for count, pb in shapes:
            ids = order[:count]
            smax, route, usc, inf = _lib.debug_ssv(ctx, prof, seqs, model, ids, pb, lanes)
            per_block = inf["per_block"]
            wrong = (smax.astype(np.int64) != want_smax[ids]) | (route.astype(np.int64) != want_route[ids])
            wrong |= (route == 1) & (usc.view(np.uint32) != want_bits[ids])
            for i in np.nonzero(wrong)[0][:10]:
                within = int(i) % per_block
                bad.append("class %s M=%d count=%d per_block=%d order=%s: entry %d (block %d, group %d, slot %d of %d) L=%d %s: Smax %d want %d, route %d want %d, "
                           "usc %r oracle %r" % (label, M, count, per_block, oname, i, int(i) // per_block, within // s, within % s, s, lens[ids[i]],
                                                w.recs[M][ids[i] % n][0], smax[i], want_smax[ids[i]], route[i], want_route[ids[i]], float(usc[i]),
                                                float(o_sc[ids[i] % n])))
    assert not bad, "\n".join(["%d mismatches, the first ten:" % len(bad)] + bad[:10])
    # the pairs the finish hands to the exact MSV kernel: that kernel (run_msv_exact, through ckm_debug_stages) against the oracle's bytes
    if M not in st["exact_checked"]:
        st["exact_checked"].add(M)
        exact = [i for i in range(n) if dec[i].route == R.EXACT]
        got = _lib.debug_stages(ctx, prof, seqs, np.full(len(exact), model), np.array(exact)) if exact else []
        for g, i in zip(got, exact):
            assert g.msvp_xJ == o_xJ[i] and common.float_bits(g.msvp_sc) == common.float_bits(o_sc[i]), (label, M, w.recs[M][i][0], g.msvp_xJ, int(o_xJ[i]))
            assert g.ssv_maxv == dec[i].smax, (label, M, w.recs[M][i][0], g.ssv_maxv, dec[i].smax)


@pytest.mark.parametrize("label,lanes,Q,lengths", CLASSES, ids=[c[0].replace(" ", "_") for c in CLASSES])
def test_smax_and_route_of_every_pair(ssv_world, label, lanes, Q, lengths):
    w = ssv_world["w"]
    counts, distinct = R.coverage([d for M in lengths for d in w.decisions[M]])
    assert R.coverage_met(counts, distinct), (label, counts, distinct)          # on the reference alone, before anything is compared
    for M in lengths:
        _run_model(ssv_world, label, lanes, Q, M)


def test_forced_mapping_without_an_image_is_refused(ssv_world):
    """lanes=8 on a model of more than 512 nodes: CKM_ERANGE; a sequence listed twice, an empty list, an unknown mapping: CKM_EINVAL."""
    st = ssv_world
    M = 513
    seqs, _o = _model_state(st, M)
    model = st["w"].index[M]
    for args, code in ((([0, 1], 0, 8), -7), (([0, 0], 0, 0), -1), (([], 0, 0), -1), (([0], 0, 4), -1), (([POOL], 0, 0), -1)):
        with pytest.raises(_lib.CkmError) as e:
            _lib.debug_ssv(st["ctx"], st["prof"], seqs, model, *args)
        assert e.value.code == code, (args, e.value)
