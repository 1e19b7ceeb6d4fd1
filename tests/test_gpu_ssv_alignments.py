"""What only the two-alignment row of the 8-lane SSV kernel (checkm_amd/csrc/kernels_ssv.hip: ssv_rows2_h2) and the choice between it and
the striped row can get wrong, through ckm_debug_ssv against the plain reference of tests/ssv_reference.py.  All comparisons are exact.

Models: M = 16q - 1, 16q and 16q + 1 for the 8-lane classes q = 2, 5, 13 and 16, and M = 512; M = 513, 32 * 18 and 32 * 40 for the 16-lane
kernel.  A model of fewer than 16q nodes in an 8-lane class q <= 16 takes the two-alignment row; a model that fills its class (M = 16q),
the 8-lane classes beyond 16 registers (M = 257, 512) and every 16-lane class keep the striped row, so both rows and the switch between
them inside one launch class are covered.

Targets, about 50 per model:
  * ungapped hits that end in node M on an odd and on an even row (the last cell of the class, which no lane holds at odd rows when the
    model leaves it out, and which is a model cell when M fills the class);
  * ungapped hits that start in node 1 on the row right after a row where node M scores high, in both row parities: a carry that leaks
    the last cell into node 1 would add the two.  On the models that fill their class (M = 16q, 32q) the reference with such a leak is
    asserted to give a different Smax for these pairs, before anything is compared;
  * an ungapped hit across every lane boundary of the consecutive-cell mapping (cells z * 2Q) -- one target per boundary;
  * lengths 1 .. 20, 31, 32, 33 in list order, so that odd and even lengths share a wavefront group, and for a few lengths a target
    whose best segment lies in its first two rows and one whose best segment lies in its last two, the rest being residues that score
    nothing (asserted on the reference's running maximum)."""
import numpy as np
import pytest

from checkm_amd import _lib
from oracle import p7
from synthdata import synth
from tests import common
from tests import ssv_reference as R

pytestmark = pytest.mark.gpu

EIGHT_Q = (2, 5, 13, 16)
MODELS = sorted(set([16 * q + d for q in EIGHT_Q for d in (-1, 0, 1)] + [512, 513, 32 * 18, 32 * 40]))
LENGTHS = list(range(1, 21)) + [31, 32, 33]
EDGE_LENGTHS = (2, 3, 15, 16, 17, 18, 32, 33)


def launch_class(M):
    """(class number as ckm_debug_ssv reports it, lanes per sequence, packed registers per lane)"""
    if M <= 512:
        q = next(q for q in R.EIGHT_LANE_Q if 16 * q >= M)
        return 100 + q, 8, q
    q = next(q for q in R.SIXTEEN_LANE_Q if 32 * q >= M)
    return q, 16, q


def fills_class(M):
    _cls, lanes, q = launch_class(M)
    return M == 2 * q * lanes


def smax_with_leak(cost, bias, dsq):
    """The recurrence with the fault under test: node M of the previous row is taken as the predecessor of node 1."""
    d = int(bias) - cost.astype(np.int32)
    U = np.zeros(cost.shape[1] + 1, dtype=np.int32)
    best = 0
    for x in dsq:
        U[0] = U[-1]
        U[1:] = np.clip(U[:-1] + d[x], 0, R.CEILING)
        best = max(best, int(U[1:].max()))
    return best


def _best_residues(cost):
    return np.argmin(cost[:20].astype(np.int32), axis=0)                # per node k (at k - 1): the residue of the lowest byte cost


def build_targets(M, ref):
    """[(name, text)], and the names of the pairs a leak of node M into node 1 must change."""
    rng = np.random.default_rng(43000 + M)
    best = _best_residues(ref.cost)
    _cls, lanes, q = launch_class(M)

    def hit(a, b):                                                      # the ungapped best residues of nodes a .. b
        return synth.to_text(best[a - 1:b])

    def noise(n):
        return synth.to_text(synth.random_residues(rng, n))

    recs, leak_sensitive = [], []
    for k, L in enumerate(LENGTHS):
        recs.append(("len%d" % L, noise(L)))
    w = min(6, M - 1)
    for lead in (4, 5):                                                 # the hit's last residue on row lead + w (1-based): even, odd
        recs.append(("end_in_M_lead%d" % lead, noise(lead) + hit(M - w, M)))
        recs.append(("end_in_M_lead%d_tail" % lead, noise(lead) + hit(M - w, M) + "X" * 3))
    for lead in (2, 3):
        name = "M_then_1_lead%d" % lead
        recs.append((name, "X" * lead + hit(M - 4, M) + hit(1, 5) + "X" * 2))
        leak_sensitive.append(name)
    for z in range(1, lanes):                                           # cells z * 2q - 1 -> z * 2q: nodes z * 2q, z * 2q + 1
        b = z * 2 * q
        if b + 1 > M:
            break
        a0, a1 = max(1, b - 3), min(M, b + 4)
        recs.append(("boundary%d_%d_%d" % (z, a0, a1), "X" * (z % 3) + hit(a0, a1) + "X" * (1 + z % 2)))
    k0 = max(1, M // 2)
    for L in EDGE_LENGTHS:
        recs.append(("first2_L%d" % L, hit(k0, k0 + 1) + "X" * (L - 2)))
        recs.append(("last2_L%d" % L, "X" * (L - 2) + hit(k0, k0 + 1)))
    return recs, leak_sensitive


class World(object):
    _instance = None

    def __init__(self):
        self.profs = [R.make_profile(M) for M in MODELS]
        self.path = common.hmm_file("ssv_alignments", self.profs)
        self.hs = p7.HmmSet(self.path)
        self.index = dict((M, i) for i, M in enumerate(MODELS))
        self.refs, self.recs, self.dsq, self.decisions, self.leaky = {}, {}, {}, {}, {}
        for M, p in zip(MODELS, self.profs):
            ref = R.ModelReference(self.hs, self.index[M], p.stats)
            recs, leaky = build_targets(M, ref)
            dsq = [p7.digitize(t) for _n, t in recs]
            self.refs[M], self.recs[M], self.dsq[M], self.decisions[M], self.leaky[M] = ref, recs, dsq, ref.decisions(dsq), leaky

    @classmethod
    def get(cls):
        if cls._instance is None:
            cls._instance = World()
        return cls._instance

    def check_reference(self, M):
        """What the targets are meant to be, on the reference alone."""
        ref, names = self.refs[M], [n for n, _t in self.recs[M]]
        dec = self.decisions[M]
        for i, name in enumerate(names):
            dsq = self.dsq[M][i]
            if name.startswith(("first2_", "last2_", "end_in_M", "M_then_1", "boundary")):
                assert 0 < dec[i].smax < R.CEILING, (M, name, dec[i].smax)
                best, running = R.smax_numpy(ref.cost, ref.sc["bias"], dsq)
                assert best == dec[i].smax, (M, name)
                if name.startswith("first2_"):
                    assert running[1] == best, (M, name, running.tolist())
                if name.startswith("last2_") and len(dsq) > 2:
                    assert running[len(dsq) - 3] < best, (M, name, running.tolist())
            if name in self.leaky[M] and fills_class(M):
                leak = smax_with_leak(ref.cost, ref.sc["bias"], dsq)
                assert leak != dec[i].smax, (M, name, leak, dec[i].smax)


@pytest.fixture(scope="module")
def world(gpu_ctx):
    w = World.get()
    prof = _lib.Profiles(gpu_ctx, w.path)
    yield dict(ctx=gpu_ctx, w=w, prof=prof)
    prof.close()


def test_models_cover_both_rows():
    """Some model of the list takes each row, and the lists of tests/ssv_reference.py still put M = 16q into class q."""
    two = [M for M in MODELS if M <= 512 and launch_class(M)[2] <= 16 and not fills_class(M)]
    striped8 = [M for M in MODELS if M <= 512 and M not in two]
    assert set(two) == set([31, 33, 79, 81, 207, 209, 255]) and set(striped8) == set([32, 80, 208, 256, 257, 512])
    for q in EIGHT_Q:
        assert launch_class(16 * q) == (100 + q, 8, q) and launch_class(16 * q + 1)[2] > q
    assert launch_class(513) == (18, 16, 18) and launch_class(32 * 18) == (18, 16, 18) and launch_class(32 * 40) == (40, 16, 40)


@pytest.mark.parametrize("M", MODELS)
def test_smax_and_route(world, M):
    w, ctx, prof = world["w"], world["ctx"], world["prof"]
    w.check_reference(M)
    recs, dec = w.recs[M], w.decisions[M]
    n = len(recs)
    model = w.index[M]
    _o_xJ, o_sc, _o_pass = w.hs.msv_stage(model, w.dsq[M])
    seqs = _lib.Seqs(ctx, [[(name, "", text) for name, text in recs]])
    try:
        want_smax = np.array([d.smax for d in dec], dtype=np.int64)
        want_route = np.array([d.route for d in dec], dtype=np.int64)
        want_bits = common.float_bits(o_sc)
        cls, lanes, _q = launch_class(M)
        bad = []
        for oname, order in (("as listed", np.arange(n)), ("reversed", np.arange(n)[::-1].copy())):
            smax, route, usc, info = _lib.debug_ssv(ctx, prof, seqs, model, order, 0, 0)
            assert info["cls"] == cls, (M, info)
            wrong = (smax.astype(np.int64) != want_smax[order]) | (route.astype(np.int64) != want_route[order])
            wrong |= (route == 1) & (usc.view(np.uint32) != want_bits[order])
            for i in np.nonzero(wrong)[0]:
                bad.append("M=%d class %d order %s: entry %d (slot %d of %d) %s L=%d: Smax %d want %d, route %d want %d" % (
                    M, cls, oname, i, int(i) % (64 // lanes), 64 // lanes, recs[order[i]][0], dec[order[i]].L, smax[i], want_smax[order[i]],
                    route[i], want_route[order[i]]))
        assert not bad, "\n".join(["%d mismatches, the first ten:" % len(bad)] + bad[:10])
    finally:
        seqs.close()
