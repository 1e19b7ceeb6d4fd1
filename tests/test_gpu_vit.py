"""The FAST Viterbi kernels and the F2 decisions of the Viterbi epilogues (checkm_amd/csrc/kernels_filter.hip: vit16_kernel<Q>,
vit_kernel<QH, true>, vit_kernel<QH, false> with `decide`) and the device bias filter against the plain reference of
tests/vit_reference.py, launched the way the device-driven search launches them (ckm_debug_filters), pair by pair, for every class.

Scores: vit_fast bits, xC (where the mode returns it) and vit_flag equal the reference exactly; vit_exact bits equal the oracle's for
every pair that reached the exact queue.  Decisions, with v = (score - filtersc) * log2(e) in float64 and thr the bit score at which the
Gumbel tail equals F2: no pair whose exact decision passes is lost, each is forwarded once; a forwarded pair that fails exactly lies
within margin_vit (+ the float32 rounding of v) of thr; the exact queue holds the pairs with flag 1 and v < thr + margin, each once, with
route 2; the status word is 0.  The rounding allowance is 2^-22 (|v| + |thr| + margin): v is two float32 operations on exact inputs and
a rounded constant (3 * 2^-24 |v|), the threshold a float32 next to thr (2^-23 |thr|) and its sum with the margin one more rounding."""
import ctypes
import math

import numpy as np
import pytest

from checkm_amd import _lib
from tests import common
from tests import vit_reference as R

pytestmark = pytest.mark.gpu

MARGIN_MSV, MARGIN_VIT = R.MARGIN_MSV, R.MARGIN_VIT
GRID_VIT = 2048
CLASSES = R.launch_classes()
_logf = ctypes.CDLL("libm.so.6").logf
_logf.restype, _logf.argtypes = ctypes.c_float, [ctypes.c_float]


@pytest.fixture(scope="module")
def vit_world(gpu_ctx):
    w = R.World.get()
    prof = _lib.Profiles(gpu_ctx, w.path)
    state = dict(ctx=gpu_ctx, w=w, prof=prof, seqs={})
    yield state
    for s in state["seqs"].values():
        s.close()
    prof.close()


def _seqs(st, M):
    if M not in st["seqs"]:
        st["seqs"][M] = _lib.Seqs(st["ctx"], [[(n, "", t) for n, t in st["w"].recs[M]]])
    return st["seqs"][M]


def _sorted_slots(lengths):
    """Where vit16_kernel runs each queue entry: it sorts every chunk of 64 entries by the key (L + 1) << 6 | lane, largest first, and
    takes quads of neighbours of the sorted order.  Returns the entry's position in its sorted chunk, per queue position."""
    slot = [0] * len(lengths)
    for c0 in range(0, len(lengths), 64):
        keys = sorted((((lengths[c0 + lane] + 1) << 6) | lane, lane) for lane in range(min(64, len(lengths) - c0)))[::-1]
        for p, (_key, lane) in enumerate(keys):
            slot[c0 + lane] = p
    return slot


def _where(label, M, name, pos, L, slot):
    if slot is None:
        return "class %s M=%d %s: queue position %d (a wavefront of its own) L=%d" % (label, M, name, pos, L)
    return "class %s M=%d %s: queue position %d (chunk %d; after the chunk's sort: quad %d, group %d) L=%d" % (label, M, name, pos, pos // 64, slot // 4, slot % 4, L)


def _check(st, label, mode, items, out, status, nblocks, order_name, filtersc=None):
    """items: [(M, record index)] in queue order; out: the entry's records.  Returns failure lines."""
    w = st["w"]
    bad = []
    if status != 0:
        bad.append("class %s: status %#x" % (label, status))
    slots = _sorted_slots([w.pairs[M][k].L for M, k in items]) if mode == _lib.FILTERS_VIT16 else None
    for pos, (M, k) in enumerate(items):
        q, ref, o = w.pairs[M][k], w.refs[M], out[pos]
        where = _where(label, M, w.recs[M][k][0], pos, q.L, None if slots is None else slots[pos]) + " order=%s nblocks=%d" % (order_name, nblocks)
        fsc = q.bias if filtersc is None else filtersc[pos]
        if int(common.float_bits(o["vit_fast"])) != int(common.float_bits(q.fast)) or int(o["vit_flag"]) != q.flag:
            bad.append("%s: vit_fast %r flag %d, reference %r flag %d (xE %d)" % (where, float(o["vit_fast"]), int(o["vit_flag"]), float(q.fast), q.flag, q.xE))
            continue
        if mode == _lib.FILTERS_WAVE_FAST_PLAIN:
            if int(o["vit_xC"]) != (32767 if q.overflow else q.xC):
                bad.append("%s: xC %d, reference %d" % (where, int(o["vit_xC"]), q.xC))
            continue
        thr, m = ref.thr_vit, MARGIN_VIT
        v = float(R.v_bits(q.fast, fsc))
        eps = 2.0 ** -22 * ((abs(v) if math.isfinite(v) else 0.0) + abs(thr) + m)
        in_vxq, fwd = int(o["n_vxq"]), int(o["n_fwork"])
        if q.flag == 1 and v < thr + m - eps and in_vxq != 1:
            bad.append("%s: flag 1, v %.6f < thr %.6f + margin, but %d times in the exact queue" % (where, v, thr, in_vxq))
        if (q.flag == 0 or v > thr + m + eps) and in_vxq != 0:
            bad.append("%s: flag %d, v %.6f, thr %.6f, yet in the exact queue" % (where, q.flag, v, thr))
        if in_vxq:
            if int(o["route"]) != 2:
                bad.append("%s: in the exact queue with route %#x" % (where, int(o["route"])))
            if int(common.float_bits(o["vit_exact"])) != int(common.float_bits(q.exact)):
                bad.append("%s: vit_exact %r, oracle %r" % (where, float(o["vit_exact"]), float(q.exact)))
            v = float(R.v_bits(q.exact, fsc))                   # the score that decides
        if q.pass_exact and fwd != 1:
            bad.append("%s: passes exactly (v %.6f, thr %.6f) but was forwarded %d times" % (where, v, thr, fwd))
        if fwd and not q.pass_exact and not (abs(v - thr) <= m + eps):
            bad.append("%s: forwarded, fails exactly, v %.6f outside the band around thr %.6f" % (where, v, thr))
        if fwd > 1:
            bad.append("%s: forwarded %d times" % (where, fwd))
    return bad


def _run(st, label, mode, items, nblocks=0, order_name="records"):
    w = st["w"]
    # one sequence set per set of models: a mixed queue needs one set holding the records of all its models
    models = sorted(set(M for M, _k in items))
    key = tuple(models)
    if key not in st["seqs"]:
        recs = [("%d_%s" % (M, n), "", t) for M in models for n, t in w.recs[M]]
        st["seqs"][key] = _lib.Seqs(st["ctx"], [recs])
    base, at = {}, 0
    for M in models:
        base[M] = at
        at += len(w.recs[M])
    model = [w.index[M] for M, _k in items]
    seq = [base[M] + k for M, k in items]
    usc = [w.pairs[M][k].msv for M, k in items]
    fsc = [w.pairs[M][k].bias for M, k in items]
    out, status = _lib.debug_filters(st["ctx"], st["prof"], st["seqs"][key], model, seq, usc, fsc, mode, nblocks)
    return _check(st, label, mode, items, out, status, nblocks, order_name)


def _report(bad):
    assert not bad, "\n".join(["%d mismatches, the first ten:" % len(bad)] + bad[:10])


@pytest.mark.parametrize("label,kind,Q,lengths", CLASSES, ids=[c[0] for c in CLASSES])
def test_scores_and_decisions_of_every_pair(vit_world, label, kind, Q, lengths):
    w = vit_world["w"]
    counts, distinct, _ninf = R.coverage([q for M in lengths for q in w.pairs[M]])
    assert R.coverage_met(counts, distinct), (label, counts, distinct)          # on the reference alone, before anything is compared
    bad = []
    for M in lengths:
        items = [(M, k) for k in range(len(w.recs[M]))]
        modes = [_lib.FILTERS_VIT16] if kind == "vit16" else [_lib.FILTERS_WAVE_FAST, _lib.FILTERS_WAVE_FAST_PLAIN]
        for mode in modes:
            bad += _run(vit_world, label, mode, items)
    _report(bad)


@pytest.mark.parametrize("label,kind,Q,lengths", [c for c in CLASSES if c[1] == "vit16"], ids=[c[0] for c in CLASSES if c[1] == "vit16"])
def test_vit16_queue_shapes_orders_and_grids(vit_world, label, kind, Q, lengths):
    """Queue lengths around the quad, the chunk of 64 and beyond; ascending, descending and shuffled orders (the 3100-residue target
    next to length-1 targets at the head); the models of the class mixed in one queue; 1, 5, 10 and GRID_VIT workgroups of four
    wavefronts.  The kernel doubles S, the wavefronts that share a chunk, while S < 16 and chunks * S < wavefronts: the 10 chunks of 600
    entries run with S = 1 (several chunks per wavefront), 2, 4 and 16, the 3 chunks of 130 entries with S = 2, 8, 16 and 16, the one
    chunk of 5 entries with S = 4, 16, 16 and 16."""
    w = vit_world["w"]
    pool = [(M, k) for M in lengths for k in range(len(w.recs[M]))]
    L = np.array([w.pairs[M][k].L for M, k in pool])
    names = [w.recs[M][k][0] for M, k in pool]
    rng = np.random.default_rng(700 + Q)
    perm = list(rng.permutation(len(pool)))
    long_ = next(i for i, n in enumerate(names) if n.startswith("r3100"))
    tiny = [i for i, n in enumerate(names) if n.startswith("tiny_")][:3]
    head = tiny[:2] + [long_] + tiny[2:]
    perm = head + [i for i in perm if i not in head]
    orders = [("ascending", list(np.argsort(L, kind="stable"))), ("descending", list(np.argsort(-L, kind="stable"))), ("shuffled", perm)]
    bad = []
    assert len(pool) >= 300
    for oname, order in orders:
        full = (order * (600 // len(order) + 1))[:600]
        for count in (1, 3, 4, 5, 63, 64, 65, 130, 600):
            for nblocks in ((1, 5, 10, GRID_VIT) if count in (5, 130, 600) else (GRID_VIT,)):
                items = [pool[i] for i in full[:count]]
                # (a pair may sit in the queue twice here only as two list entries of different candidates: every entry is its own candidate)
                bad += _run(vit_world, label, _lib.FILTERS_VIT16, items, nblocks, oname)
    _report(bad)


def test_chain_routes_every_pair_of_a_mixed_world(vit_world):
    """bias_filter_kernel and everything behind it on all pairs of a world that mixes classes: the raw bias numbers against the oracle's
    bias_sc, the approximate null score within margin_msv, the route against the exact F1 / F2 tests, and the Viterbi rules downstream."""
    st, w = vit_world, vit_world["w"]
    lengths = R.CHAIN_LENGTHS
    items = [(M, k) for M in lengths for k in range(len(w.recs[M]))]
    models = sorted(set(lengths))
    recs = [("%d_%s" % (M, n), "", t) for M in models for n, t in w.recs[M]]
    seqs = _lib.Seqs(st["ctx"], [recs])
    base, at = {}, 0
    for M in models:
        base[M] = at
        at += len(w.recs[M])
    out, status = _lib.debug_filters(st["ctx"], st["prof"], seqs, [w.index[M] for M, _k in items], [base[M] + k for M, k in items],
                                     [w.pairs[M][k].msv for M, k in items], None, _lib.FILTERS_CHAIN)
    seqs.close()
    assert status == 0
    bad, worst, undecided = [], 0.0, {}
    for pos, (M, k) in enumerate(items):
        q, ref, o = w.pairs[M][k], w.refs[M], out[pos]
        where = "M=%d %s L=%d (candidate %d)" % (M, w.recs[M][k][0], q.L, pos)
        p1 = np.float32(q.L) / np.float32(q.L + 1)
        nullsc = np.float32(math.log(float(o["bias_d"])) + float(o["bias_e"]) * math.log(2.0))
        host = np.float32(np.float32(nullsc + np.float32(np.float32(q.L) * np.float32(_logf(p1)))) + np.float32(_logf(np.float32(np.float32(1.0) - p1))))
        if int(common.float_bits(host)) != int(common.float_bits(q.bias)):
            bad.append("%s: filtersc from (bias_d, bias_e) %r, oracle %r" % (where, float(host), float(q.bias)))
        err = abs(float(o["filtersc"]) - float(q.bias)) / math.log(2.0)
        worst = max(worst, err)
        route, fwd, nvq, nvxq = int(o["route"]), int(o["n_fwork"]), int(o["n_vq"]), int(o["n_vxq"])
        sc = float(R.v_bits(q.msv, q.bias))
        eps = 2.0 ** -20 * (abs(sc) if math.isfinite(sc) else 0.0) + err
        if q.pass_f1 and route == 0xff:
            bad.append("%s: passes F1 exactly, route 0xff" % where)
        if sc < ref.thr_f1 - MARGIN_MSV - eps and route != 0xff:
            bad.append("%s: %.4f bits below F1 %.4f by more than the margin, route %#x" % (where, sc, ref.thr_f1, route))
        if q.pass_f1 and not q.need_vit and fwd != 1:
            bad.append("%s: passes F2 on the MSV score, forwarded %d times" % (where, fwd))
        if q.pass_f1 and q.need_vit and route not in (1, 2, 0x12):
            bad.append("%s: needs the Viterbi filter, route %#x" % (where, route))
        if route in (1, 2) and nvq != 1:
            bad.append("%s: route %#x, %d times in the FAST queue" % (where, route, nvq))
        if route in (2, 0x12) and nvxq != 1:
            bad.append("%s: route %#x, %d times in the exact queue" % (where, route, nvxq))
        if route in (0, 0xff, 0x12) and nvq != 0:
            bad.append("%s: route %#x, in the FAST queue" % (where, route))
        if route == 0x12 and fwd != 1:
            bad.append("%s: route 0x12 goes on regardless, forwarded %d times" % (where, fwd))
        if route == 0 and fwd != 1:
            bad.append("%s: route 0, forwarded %d times" % (where, fwd))
        if route == 0xff and fwd != 0:
            bad.append("%s: dead, forwarded" % where)
        if abs(sc - ref.thr_f1) <= MARGIN_MSV + eps or abs(sc - ref.thr_f2) <= MARGIN_MSV + eps:
            undecided[M] = undecided.get(M, 0) + 1
    print("bias filter: max |approximate - exact filtersc| = %.3g bits over %d pairs" % (worst, len(items)))
    assert worst < MARGIN_MSV, worst
    for M, n in undecided.items():
        assert n <= 0.02 * len(w.recs[M]), (M, n)
    # the Viterbi rules on the pairs the bias filter queued for the FAST kernels, with the filtersc the device stored
    vq = [pos for pos in range(len(items)) if int(out[pos]["route"]) in (1, 2)]
    bad += _check(st, "chain", _lib.FILTERS_CHAIN, [items[p] for p in vq], out[vq], status, 0, "device", filtersc=[float(out[p]["filtersc"]) for p in vq])
    for pos in range(len(items)):
        if int(out[pos]["route"]) == 0x12:
            M, k = items[pos]
            if int(common.float_bits(out[pos]["vit_exact"])) != int(common.float_bits(w.pairs[M][k].exact)):
                bad.append("M=%d %s: vit_exact %r, oracle %r" % (M, w.recs[M][k][0], float(out[pos]["vit_exact"]), float(w.pairs[M][k].exact)))
    _report(bad)


def test_bad_arguments_are_refused(vit_world):
    """A model without a 16-lane image in VIT16 mode: CKM_ERANGE.  An unknown mode, a sequence index out of range, two 16-lane classes in
    one VIT16 call, no filtersc outside CHAIN, and an EMPTY sequence in any mode (the kernels' contract, and the reason why the sort key's
    + 1 and the padding keys never meet): CKM_EINVAL."""
    st, w = vit_world, vit_world["w"]
    M = 513
    seqs = _seqs(st, M)
    i513, i32, i33 = w.index[513], w.index[32], w.index[33]
    for args, code in ((([i513], [0], [0.0], [0.0], _lib.FILTERS_VIT16), -7), (([i513], [0], [0.0], [0.0], 9), -1),
                       (([i513], [10 ** 6], [0.0], [0.0], _lib.FILTERS_WAVE_FAST), -1), (([i32, i33], [0, 0], [0.0, 0.0], [0.0, 0.0], _lib.FILTERS_VIT16), -1),
                       (([i513], [0], [0.0], None, _lib.FILTERS_WAVE_FAST), -1), (([i32], [0], [0.0], None, _lib.FILTERS_VIT16), -1),
                       (([i513], [0], [0.0], None, _lib.FILTERS_WAVE_FAST_PLAIN), -1)):
        with pytest.raises(_lib.CkmError) as e:
            _lib.debug_filters(st["ctx"], st["prof"], seqs, *args)
        assert e.value.code == code, (args, e.value)
    empty = _lib.Seqs(st["ctx"], [[("full", "", "ACDEFGHIKL"), ("empty", "", "")]])
    try:
        for mode, model in ((_lib.FILTERS_VIT16, i32), (_lib.FILTERS_WAVE_FAST, i513), (_lib.FILTERS_WAVE_FAST_PLAIN, i513), (_lib.FILTERS_CHAIN, i32)):
            with pytest.raises(_lib.CkmError) as e:
                _lib.debug_filters(st["ctx"], st["prof"], empty, [model, model], [0, 1], [0.0, 0.0], [0.0, 0.0], mode)
            assert e.value.code == -1 and "empty" in str(e.value), (mode, e.value)
            out, status = _lib.debug_filters(st["ctx"], st["prof"], empty, [model], [0], [0.0], [0.0], mode)      # (the full one alone is fine)
            assert status == 0 and len(out) == 1
    finally:
        empty.close()
