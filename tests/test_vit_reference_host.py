"""The plain reference of the FAST Viterbi kernels (tests/vit_reference.py) pinned to the oracle's Viterbi filter, without a GPU: its C loops
(without and with the J state) against its numpy statements on a sample, the with-J loop against the oracle's exact filter and
HmmSet.vit_stage against stages() on EVERY pair of the worlds tests/test_gpu_vit.py runs, the two properties the kernels rely on (flag 0:
the bound is the exact score; flag 1: the bound is not above it) on every pair, the coverage condition of every class, the share of
pairs the device's margins leave undecided, and the pairs at the flag's edge.

The numpy statements are a Python loop over rows and, for the D state, over cells: they run on the pairs of the models of up to 33 nodes
with targets of up to 70 residues; the scalar C loops of the same recurrences (p7.vit_fast) carry them to every pair."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from tests import common
from tests import vit_reference as R


def _sample(w):
    for M in w.lengths:
        if M <= 33:
            for k, (d, q) in enumerate(zip(w.dsq[M], w.pairs[M])):
                if len(d) <= 70:
                    yield M, k, d, q


def test_c_loops_equal_the_numpy_statements():
    w = R.World.get()
    n = 0
    for M, k, d, q in _sample(w):
        ref = w.refs[M]
        xE, _ = R.viterbi_numpy(ref.sc, ref.emis, ref.trans, q.w_move, d)
        assert xE == q.xE, (M, w.recs[M][k][0], xE, q.xE)
        xC, overflow = R.viterbi_numpy(ref.sc, ref.emis, ref.trans, q.w_move, d, with_j=True)
        assert xC == q.plain_xC and overflow == (q.plain_xC == R.POS), (M, w.recs[M][k][0], xC, q.plain_xC)
        n += 1
    assert n > 400, n


def test_exact_statement_equals_the_oracle_on_every_pair():
    """The with-J recurrence (its C loop, pinned to the numpy statement above) against the oracle's vit_xC and vit_sc, every pair."""
    w = R.World.get()
    bad, n = [], 0
    for M in w.lengths:
        ref = w.refs[M]
        for k, q in enumerate(w.pairs[M]):
            n += 1
            sc = R.vit_score(ref.sc, q.plain_xC, q.w_move, q.plain_xC == R.POS)
            if q.plain_xC != q.exact_xC or int(common.float_bits(sc)) != int(common.float_bits(q.exact)):
                bad.append((M, w.recs[M][k][0], q.plain_xC, q.exact_xC, float(sc), float(q.exact)))
    assert n == sum(len(v) for v in w.pairs.values()) and n > 6000
    assert not bad, bad[:10]


def test_vit_stage_equals_stages_on_every_pair():
    w = R.World.get()
    jobs = [(M, k) for M in sorted(w.lengths, reverse=True) for k in range(len(w.pairs[M]))]

    def one(job):
        M, k = job
        q, st = w.pairs[M][k], w.hs.stages(w.index[M], w.dsq[M][k])
        got = (int(common.float_bits(q.msv)), int(common.float_bits(q.bias)), q.exact_xC, int(common.float_bits(q.exact)))
        want = (int(common.float_bits(st.msv_sc)), int(common.float_bits(st.bias_sc)), st.vit_xC, int(common.float_bits(st.vit_sc)))
        ok = got == want and q.pass_exact == R.passes(st.vit_sc, st.bias_sc, w.refs[M].vmu, w.refs[M].vlam, R.F2)
        if st.pass_bias and not q.need_vit:
            ok = ok and st.pass_vit == 1
        if st.pass_bias and q.need_vit:
            ok = ok and st.pass_vit == int(q.pass_exact)
        return None if ok else (M, w.recs[M][k][0], got, want)
    with ThreadPoolExecutor(max_workers=12) as ex:                          # (the oracle's C code releases the interpreter lock)
        bad = [r for r in ex.map(one, jobs) if r is not None]
    assert len(jobs) > 6000
    assert not bad, bad[:10]


def test_the_bound_is_exact_without_the_flag_and_never_above():
    w = R.World.get()
    bad, n = [], 0
    for M in w.lengths:
        for k, q in enumerate(w.pairs[M]):
            n += 1
            fast_xC = 32767 if q.overflow else q.xC
            if q.flag == 0 and (fast_xC != q.exact_xC or int(common.float_bits(q.fast)) != int(common.float_bits(q.exact))):
                bad.append((M, w.recs[M][k][0], "flag 0", fast_xC, q.exact_xC))
            if q.flag == 1 and not (fast_xC <= q.exact_xC and q.fast <= q.exact):
                bad.append((M, w.recs[M][k][0], "flag 1", fast_xC, q.exact_xC))
    assert n > 6000
    assert not bad, bad[:10]


def test_coverage_condition_of_every_class():
    """On the reference alone: every class has at least 3 pairs in every outcome and 30 distinct xC values; -inf occurs."""
    w = R.World.get()
    table = w.class_coverage()
    for label, ms, counts, distinct, ninf in table:
        print("%-10s M=%-18s %s distinct=%d -inf=%d" % (label, ms, " ".join("%s=%d" % (o, counts[o]) for o in R.OUTCOMES), distinct, ninf))
    assert len(table) == len(R.VIT16_Q) + len(R.WAVE_QH)
    missing = [(label, counts, distinct) for label, _ms, counts, distinct, _n in table if not R.coverage_met(counts, distinct)]
    assert not missing, missing
    assert sum(ninf for _l, _m, _c, _d, ninf in table) >= 1


def test_undecided_pairs_are_few():
    """Pairs within a margin of a threshold they are tested against (the device's rules leave them to either side) are at most 2 % of
    every class and of every model of the CHAIN test's world: from the margins, the thresholds and the oracle's scores alone."""
    w = R.World.get()
    for label, _kind, _q, ms in R.launch_classes():
        pairs = [(M, q) for M in ms for q in w.pairs[M]]
        n = sum(1 for M, q in pairs if R.undecided(w.refs[M], q))
        assert n <= 0.02 * len(pairs), (label, n, len(pairs))
    for M in R.CHAIN_LENGTHS:
        n = sum(1 for q in w.pairs[M] if R.undecided(w.refs[M], q))
        assert n <= 0.02 * len(w.pairs[M]), (M, n, len(w.pairs[M]))


def test_the_flag_edge_is_in_the_worlds():
    """Pairs whose xE + wE_loop equals base_w exactly (flag clear, by one word) exist in a model the 16-lane kernel runs (VIT16 mode:
    every model of the 16-lane classes) and in a model of the wave-per-pair class wave<1> (1, 5, 9 and 128 nodes: the only wave class
    whose models the edge search covers), so a flag test written with >= fails in either kernel."""
    w = R.World.get()
    at_edge = lambda M, q: q.xE + w.refs[M].sc["wE_loop"] == w.refs[M].sc["base_w"]
    edge = sorted(set(M for M in w.lengths for q in w.pairs[M] if at_edge(M, q)))
    vit16 = set(M for _l, kind, _q, ms in R.launch_classes() if kind == "vit16" for M in ms)
    wave = set(M for _l, kind, _q, ms in R.launch_classes() if kind == "wave" for M in ms)
    assert any(M in vit16 for M in edge) and any(M in wave for M in edge), edge
    assert all(q.flag == 0 for M in w.lengths for q in w.pairs[M] if at_edge(M, q))
