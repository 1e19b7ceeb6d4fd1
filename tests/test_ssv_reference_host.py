"""The plain SSV reference (tests/ssv_reference.py) pinned to the oracle's byte MSV filter, without a GPU: its byte costs against the
second formulation of tests/test_oracle_integer_filters.py, its C loop against its numpy statement, the coverage condition of every
launch class, and -- on every pair of the worlds tests/test_gpu_ssv.py runs -- its overflow, final byte and survivor decision against
the oracle."""
import os

import numpy as np

from oracle import p7
from synthdata import synth
from tests import common
from tests import ssv_reference as R
from tests import test_oracle_integer_filters as second


def test_byte_costs_equal_the_second_formulation(tmp_path):
    lengths = [5, 9, 32, 33, 129, 513]
    profs = [R.make_profile(M) for M in lengths]
    path = os.path.join(str(tmp_path), "costs.hmm")
    synth.write_hmm(path, profs)
    models = second.read_models(path)
    hs = p7.HmmSet(path)
    target_lengths = sorted(set(R.RANDOM_LENGTHS + list(range(1, 130)) + [2047, 4000]))
    for i, (M, mat, _tr) in enumerate(models):
        sc, cost, tjb = hs.msv_costs(i, target_lengths)
        bias, emission_cost, entry, leave = second.msv_model_costs(M, mat)
        assert (sc["base"], sc["bias"], sc["tbm"], sc["tec"]) == (190, bias, entry, leave), (M, sc)
        assert cost.shape == (29, M)
        want = np.array([[emission_cost(k, x) for k in range(1, M + 1)] for x in range(20)])
        assert (cost[:20] == want).all(), (M, np.argwhere(cost[:20] != want)[:5])
        assert (cost[20] == 255).all() and (cost[27] == 255).all() and (cost[28] == 255).all()      # gap, stop, missing: impossible
        assert [int(t) for t in tjb] == [second.msv_move_cost(L) for L in target_lengths], M
    hs.close()


def test_c_loop_equals_the_numpy_statement():
    w = R.World.get()
    checked = 0
    for M in w.lengths:
        if M > 64 and M not in (513, 2048):
            continue
        ref = w.refs[M]
        short = [(d, dec) for d, dec in zip(w.dsq[M], w.decisions[M]) if len(d) <= (130 if M <= 64 else 40)]
        for d, dec in short:
            best, running = R.smax_numpy(ref.cost, ref.sc["bias"], d)
            assert best == dec.smax and (len(running) == 0 or running[-1] == best), (M, len(d), best, dec.smax)
            checked += 1
    assert checked > 400


def test_coverage_condition_of_every_launch_class():
    """On the reference alone: every launch class sees every outcome and at least 20 distinct Smax values below the overflow threshold."""
    w = R.World.get()
    table = w.class_coverage()
    for label, ms, counts, distinct in table:
        print("%-14s M=%-22s %s distinct=%d" % (label, ms, " ".join("%s=%d" % (o, counts[o]) for o in R.OUTCOMES), distinct))
    assert len(table) == len(R.EIGHT_LANE_Q) + len(R.SIXTEEN_LANE_Q) + len(R.FORCED_SIXTEEN_Q)
    missing = [(label, counts, distinct) for label, _ms, counts, distinct in table if not R.coverage_met(counts, distinct)]
    assert not missing, missing


def test_reference_pinned_to_the_oracle_on_every_pair():
    """Every pair of every world.  The oracle side is the MSV stage alone (HmmSet.msv_stage: the msv_xJ, msv_sc and pass_msv of
    stages() without Viterbi and Forward on 2048 x 3100 cells); stages() itself is compared with it on the short models."""
    w = R.World.get()
    bad, n = [], 0
    for M in w.lengths:
        i = w.index[M]
        xJ, sc, ok = w.hs.msv_stage(i, w.dsq[M])
        base = w.refs[M].sc["base"]
        for k, (d, dec) in enumerate(zip(w.dsq[M], w.decisions[M])):
            name = w.recs[M][k][0]
            n += 1
            if M <= 64 or (len(d) <= 40 and k % 7 == 0):
                st = w.hs.stages(i, d)
                assert (st.msv_xJ, int(common.float_bits(st.msv_sc)), st.pass_msv) == (int(xJ[k]), int(common.float_bits(sc[k])), int(ok[k])), (M, name)
            oracle_overflow = bool(np.isposinf(sc[k]))
            assert oracle_overflow == (xJ[k] == -1)
            if dec.route != R.EXACT and dec.overflow != oracle_overflow:      # (a pair whose J state is usable may overflow LATER, through J: the exact kernel's business)
                bad.append((M, name, "overflow", dec.overflow, float(sc[k])))
                continue
            if dec.outcome == "smax0" and (oracle_overflow or xJ[k] > base):
                bad.append((M, name, "Smax 0", int(xJ[k])))
            if dec.route != R.EXACT:
                if bool(ok[k]) != (dec.route == R.SURVIVOR):
                    bad.append((M, name, "survivor", dec.route, int(ok[k])))
                if not dec.overflow and (int(xJ[k]) != dec.xJ or int(common.float_bits(sc[k])) != int(common.float_bits(dec.usc))):
                    bad.append((M, name, "xJ", dec.xJ, int(xJ[k]), float(dec.usc), float(sc[k])))
            elif dec.outcome == "j_usable" and not (xJ[k] == -1 or xJ[k] >= dec.xJ > base):
                bad.append((M, name, "J usable", dec.xJ, int(xJ[k])))          # (exact kernel: the reference claims no more than that J was reachable)
    assert n > 4000
    assert not bad, bad[:10]
