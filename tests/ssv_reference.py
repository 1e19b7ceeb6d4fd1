"""A plain CPU reference of the SSV kernel's contract (checkm_amd/csrc/kernels_ssv.hip), and the worlds it is tested on.

Never calls checkm_amd's library.  The byte costs come from the oracle's accessor (oracle/p7.py: HmmSet.msv_costs), never from the
product's DevModel or its emission tables; tests/test_ssv_reference_host.py checks them against the second formulation of
tests/test_oracle_integer_filters.py and pins everything below to the oracle's MSV filter, pair by pair, without a GPU.

Smax:     U(i,k) = min(256, max(0, U(i-1,k-1) + bias - cost[x_i][k])), U(.,0) = U(0,.) = 0; Smax = max U, in integers.  The ceiling of
          256 is the kernel's documented contract (the f16 clamp at 1.0).  smax_numpy below states it; the bulk runs through the
          same recurrence as a scalar C loop of the oracle (p7.ssv_smax), and the host test compares the two.
Routing:  the byte arithmetic of the MSV filter as the fused finish restates it --
            xB = max(base - ((tjb + tbm) & 0xff), 0);  xE = xB + Smax;  xJ = max(xE - tec, 0);  overflow iff xE + bias >= 255
            exact kernel (2) iff Smax == 0 or (not overflow and xJ > base); otherwise survivor (1) iff overflow or the F1 test passes
            on the score (xJ - tjb - base) / scale - 3 nats; otherwise dropped (0).
"""
import math

import numpy as np

from oracle import p7
from synthdata import synth

DROPPED, SURVIVOR, EXACT = 0, 1, 2
CEILING = 256
F1 = 0.02
OUTCOMES = ("smax0", "dropped", "survivor", "j_usable", "overflow", "smax256")


def smax_numpy(cost, bias, dsq):
    """The recurrence, one row at a time; also returns the running maximum after every row."""
    d = int(bias) - cost.astype(np.int32)
    U = np.zeros(cost.shape[1] + 1, dtype=np.int32)
    best, running = 0, np.zeros(len(dsq), dtype=np.int32)
    for i, x in enumerate(dsq):
        U[1:] = np.clip(U[:-1] + d[x], 0, CEILING)
        best = max(best, int(U.max()))
        running[i] = best
    return best, running


def null1_score(L):
    """The null model's score of a target of length L, in the oracle's precision."""
    p1 = np.float32(L) / np.float32(L + 1)
    return np.float32(float(np.float32(L)) * math.log(float(p1)) + math.log(1.0 - float(p1)))


def msv_score(xJ, tjb, base):
    """(xJ - tjb - base) / scale - 3 nats in float32, operation by operation."""
    scale = np.float32(3.0 / math.log(2.0))
    sc = np.float32(np.float32(xJ - tjb) - np.float32(base))
    sc = np.float32(sc / scale)
    return np.float32(sc - np.float32(3.0))


def f1_passes(usc, L, mu, lam):
    bits = np.float32(float(np.float32(usc - null1_score(L))) / math.log(2.0))
    y = float(np.float32(lam)) * (float(bits) - float(np.float32(mu)))
    ey = -math.exp(-y)
    P = -ey if abs(ey) < 5e-9 else 1.0 - math.exp(ey)
    return not (P > F1)


class Decision(object):
    __slots__ = ("L", "smax", "xB", "xJ", "overflow", "route", "usc", "outcome")


def decide(sc, tjb, L, smax, mu, lam):
    """Route of one pair from its Smax: the byte arithmetic, nothing else."""
    d = Decision()
    d.L, d.smax = L, int(smax)
    d.xB = max(sc["base"] - ((int(tjb) + sc["tbm"]) & 0xff), 0)
    xE = d.xB + d.smax
    d.xJ = max(xE - sc["tec"], 0)
    d.overflow = xE + sc["bias"] >= 255
    d.usc = np.float32(np.inf) if d.overflow else msv_score(d.xJ, int(tjb), sc["base"])
    if d.smax == 0:
        d.route, d.outcome = EXACT, "smax0"
    elif not d.overflow and d.xJ > sc["base"]:
        d.route, d.outcome = EXACT, "j_usable"
    elif d.overflow:
        d.route, d.outcome = SURVIVOR, "smax256" if d.smax == CEILING else "overflow"
    elif f1_passes(d.usc, L, mu, lam):
        d.route, d.outcome = SURVIVOR, "survivor"
    else:
        d.route, d.outcome = DROPPED, "dropped"
    return d


def smax_of(hs, index, dsqs):
    """Smax of model `index` of an oracle HmmSet against digitized sequences, from the oracle's byte costs."""
    sc, cost, _tjb = hs.msv_costs(index, [])
    return p7.ssv_smax(cost, sc["bias"], dsqs)


class ModelReference(object):
    """The reference of one model of an oracle HmmSet against digitized sequences."""

    def __init__(self, hs, index, stats):
        self.hs, self.index, self.M = hs, index, hs.M(index)
        self.mu, self.lam = float("%9.4f" % stats[0]), float("%8.5f" % stats[1])      # as the HMM file carries them
        self.sc, self.cost, _ = hs.msv_costs(index, [])

    def tjb(self, lengths):
        return self.hs.msv_costs(self.index, lengths)[2]

    def decisions(self, dsqs):
        smax = p7.ssv_smax(self.cost, self.sc["bias"], dsqs)
        tjb = self.tjb([len(d) for d in dsqs])
        return [decide(self.sc, tjb[i], len(d), smax[i], self.mu, self.lam) for i, d in enumerate(dsqs)]


# ---- the worlds: two models per launch class, targets that fill the band between noise and overflow -----------------------------

EIGHT_LANE_Q = list(range(2, 17)) + list(range(18, 33, 2))                  # ssv_kernel_h8<Q8>: models of up to 16 * Q8 nodes
SIXTEEN_LANE_Q = list(range(18, 33, 2)) + [36, 40, 48, 56, 64]              # ssv_kernel_h<Q> the search reaches: 513 .. 32 * Q nodes
FORCED_SIXTEEN_Q = list(range(1, 17))                                       # ssv_kernel_h<Q> of the short models: reachable only when forced
RANDOM_LENGTHS = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 300, 1023, 1024, 1025, 3100]


def launch_classes():
    """[(label, lanes argument, Q, [model lengths])]: each class's lower edge (the previous class's upper edge + 1, so that the last
    lanes hold out-of-model cells) and its upper edge; the shortest class also takes M = 5 and 9."""
    out, prev = [], 0
    for q in EIGHT_LANE_Q:
        out.append(("h8<%d>" % q, 0, q, [5, 9, 16 * q] if prev == 0 else [prev + 1, 16 * q]))
        prev = 16 * q
    for q in SIXTEEN_LANE_Q:
        out.append(("h<%d>" % q, 0, q, [prev + 1, 32 * q]))
        prev = 32 * q
    short = sorted(set(m for _l, _a, _q, ms in out[:len(EIGHT_LANE_Q)] for m in ms))
    for q in FORCED_SIXTEEN_Q:
        out.append(("h<%d> forced" % q, 16, q, [m for m in short if (m + 31) // 32 == q]))
    return out


def model_lengths():
    return sorted(set(m for _l, _a, _q, ms in launch_classes() for m in ms))


def make_profile(M):
    """A synthetic calibrated profile of M nodes, built as tests/test_gpu_scan.py::test_register_class_boundaries builds its own."""
    rng = np.random.default_rng(52000 + M)
    p = synth.random_profile(rng, M, "SSV%04d" % M, "PF%05d.1" % (70000 + M))
    p.stats = (-8.5 - 0.002 * M, 0.71, -9.5 - 0.002 * M, 0.71, -3.8, 0.71)
    return p


def _flanked(rng, core, lo=3, hi=9):
    return np.concatenate([synth.random_residues(rng, int(rng.integers(lo, hi))), core, synth.random_residues(rng, int(rng.integers(lo, hi)))])


def base_targets(p):
    """(name, text) records of one model, without the band prefixes (those need the reference: see targets())."""
    M = p.M
    rng = np.random.default_rng(91000 + M)
    recs = []
    for k, L in enumerate(RANDOM_LENGTHS):
        recs.append(("r%d_%d" % (L, k), synth.to_text(synth.random_residues(rng, L)) + ("*" if k % 5 == 4 and L > 1 else "")))
    for k in range(7):                                                              # the company of the longest sequence in one wavefront
        recs.append(("tiny_%d" % k, synth.to_text(synth.random_residues(rng, 1 + k % 2))))
    recs += [("deg_bjzoux", "BJZOUX" * 20), ("deg_allx", "X" * 30 + "*"), ("deg_stop", "*"), ("deg_x3", "XXX"), ("deg_lower", "acdefghiklmnpqrstvwy" * 9 + "*")]
    recs.append(("planted", synth.to_text(np.concatenate([synth.random_residues(rng, 7), synth.sample_domain(rng, p), synth.random_residues(rng, 11)])) + "*"))
    consensus = np.argmax(p.mat[1:] / synth.BGF, axis=1)
    recs.append(("consensus", synth.to_text(_flanked(rng, consensus))))
    recs.append(("consensus_x3", synth.to_text(np.concatenate([consensus, synth.random_residues(rng, 4), consensus, consensus]))))
    if M >= 9:
        a = int(rng.integers(M // 2, M)); b = int(rng.integers(1, M // 2 + 1))
        recs.append(("restart", synth.to_text(np.concatenate([synth.sample_domain(rng, p, 1, a), synth.sample_domain(rng, p, b, M)]))))
    # fragments of 3 .. 61 nodes: from node 1, up to node M, across M / 2, anywhere
    for k, w in enumerate(range(3, 62, 2)):
        w = min(w, M - 1)
        if k % 4 == 0:
            a = 1
        elif k % 4 == 1:
            a = M - w
        elif k % 4 == 2:
            a = max(1, M // 2 - w // 2)
        else:
            a = int(rng.integers(1, M - w + 1))
        recs.append(("frag%d_%d_%d" % (k, a, a + w), synth.to_text(_flanked(rng, synth.sample_domain(rng, p, a, a + w)))))
    # longer than 2 Q + 2 cells (Q = ceil(M / 16) or ceil(M / 32) packed registers per lane): the diagonal crosses a lane seam of the striping
    for k, q in enumerate(((M + 15) // 16, (M + 31) // 32)):
        w = min(M - 1, 2 * q + 6 + k)
        a = int(rng.integers(1, M - w + 1))
        recs.append(("seam%d_%d_%d" % (k, a, a + w), synth.to_text(_flanked(rng, synth.sample_domain(rng, p, a, a + w)))))
    return recs


def targets(p, ref):
    """base_targets plus prefixes of planted domains (their first 120 nodes) cut where the reference's running Smax puts the final byte just below the base of
    190 (survivors below overflow: a band a few bytes wide) and just above it (J usable)."""
    recs = base_targets(p)
    rng = np.random.default_rng(77000 + p.M)
    sc, seen = ref.sc, set()
    for rep in range(3):
        dsq = np.concatenate([synth.random_residues(rng, 2 + rep), synth.sample_domain(rng, p, 1, min(p.M, 120))]).astype(np.uint8)
        _best, running = smax_numpy(ref.cost, sc["bias"], dsq)
        tjb = ref.tjb(list(range(1, len(dsq) + 1)))
        for i in range(len(dsq)):
            xB = max(sc["base"] - ((int(tjb[i]) + sc["tbm"]) & 0xff), 0)
            xJ = xB + int(running[i]) - sc["tec"]
            if xB + int(running[i]) + sc["bias"] < 255 and sc["base"] - 7 <= xJ <= sc["base"] + 4 and xJ not in seen:
                seen.add(xJ)
                recs.append(("band%d_%d" % (rep, i + 1), synth.to_text(dsq[:i + 1])))
    return recs


def coverage(decisions):
    """Outcome counts and the number of distinct Smax values strictly between 0 and the overflow threshold."""
    counts = dict((o, 0) for o in OUTCOMES)
    for d in decisions:
        counts[d.outcome] += 1
    distinct = len(set(d.smax for d in decisions if d.smax > 0 and not d.overflow))
    return counts, distinct


def coverage_met(counts, distinct):
    return all(counts[o] >= 1 for o in OUTCOMES) and distinct >= 20


class World(object):
    """Every model of every launch class with its targets and the reference's decisions (built once per process)."""
    _instance = None

    def __init__(self):
        from tests import common
        self.lengths = model_lengths()
        self.profs = [make_profile(M) for M in self.lengths]
        self.path = common.hmm_file("ssv_classes", self.profs)
        self.hs = p7.HmmSet(self.path)
        self.index = dict((M, i) for i, M in enumerate(self.lengths))
        self.refs, self.recs, self.dsq, self.decisions = {}, {}, {}, {}
        for M, p in zip(self.lengths, self.profs):
            ref = ModelReference(self.hs, self.index[M], p.stats)
            recs = targets(p, ref)
            dsq = [p7.digitize(t) for _n, t in recs]
            self.refs[M], self.recs[M], self.dsq[M], self.decisions[M] = ref, recs, dsq, ref.decisions(dsq)

    @classmethod
    def get(cls):
        if cls._instance is None:
            cls._instance = World()
        return cls._instance

    def class_coverage(self):
        """[(label, lengths, outcome counts, distinct Smax values)] per launch class, on the reference alone."""
        out = []
        for label, _lanes, _q, ms in launch_classes():
            counts, distinct = coverage([d for M in ms for d in self.decisions[M]])
            out.append((label, ms, counts, distinct))
        return out
