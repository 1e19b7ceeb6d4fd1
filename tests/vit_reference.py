"""A plain CPU reference of the FAST Viterbi filter kernels (checkm_amd/csrc/kernels_filter.hip: vit16_kernel<Q>, vit_kernel<QH, true>),
of the F2 decisions of their epilogues, and the worlds they are tested on.

Never calls checkm_amd's library.  The word costs come from the oracle's accessor (oracle/p7.py: HmmSet.vit_costs), never from the
product's DevModel or its tables; tests/test_vit_reference_host.py pins everything below to the oracle's Viterbi filter, pair by pair,
without a GPU.

Recurrence (J-free): int32 with explicit clamps to [-32768, 32767]; xB = base_w + w_move(L) is a constant of the pair;
            M(i,k) = clamp(max(clamp(xB + BM_k), clamp(M(i-1,k-1) + MM_k), clamp(I(i-1,k-1) + IM_k), clamp(D(i-1,k-1) + DM_k)) + e_k(x_i))
            I(i,k) = max(clamp(M(i-1,k) + MI_k), clamp(I(i-1,k) + II_k));  D(i,k) = max(clamp(M(i,k-1) + MD_{k-1}), clamp(D(i,k-1) + DD_{k-1}))
          xE = the maximum over all rows and cells;  overflow iff xE >= 32767;  xC = max(-32768, xE + wE_move);
          flag = (xE + wE_loop > base_w) and not overflow;  score = ((float)xC + (float)w_move - (float)base_w) / scale_w - 3 in float32,
          operation by operation (+inf on overflow, -inf when xC = -32768).
          viterbi_numpy states it (and, with J, the exact filter); the bulk runs through the same recurrence as a scalar C loop of the
          oracle (p7.vit_fast), and the host test compares the two.
Decision: v = (score - filtersc) * log2(e); the exact test is the oracle's (P-value of the Gumbel tail against F2 = 1e-3).
"""
import math
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from oracle import p7
from synthdata import synth

NEG, POS = -32768, 32767
F1, F2 = 0.02, 1e-3
VIT16_Q = [1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16]                          # vit16_kernel<Q>: models of up to 32 * Q nodes
WAVE_QH = [1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 24, 32]                  # vit_kernel<QH, .>: models of up to 128 * QH nodes
RANDOM_LENGTHS = [1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 300, 1023, 1024, 1025, 3100]
OUTCOMES = ("dead", "pass_flag0", "pass_flag1", "rerun_pass", "rerun_fail", "overflow")
MIN_PER_OUTCOME, MIN_DISTINCT_XC = 3, 30
MARGIN_MSV, MARGIN_VIT = 0.01, 0.01          # bits: the conservative bands of the device's tests (checkm_amd/csrc/ckm_host.h: kMarginMsv, kMarginVit)
CHAIN_LENGTHS = [5, 32, 33, 129, 256, 449, 512, 513, 768, 2049]      # the mixed-class world of the CHAIN test


def viterbi_numpy(sc, emis, trans, w_move, dsq, with_j=False):
    """The recurrence, one row at a time.  J-free: (xE, None).  With the J state (the exact filter): (xC or 32767 on overflow, overflow)."""
    M = emis.shape[1]
    e32, t = emis.astype(np.int32), trans.astype(np.int32)
    BM, MM, IM, DM, MD, MI, II, DD = (t[k] for k in range(8))
    clamp = lambda a: np.clip(a, NEG, POS)
    mm = np.full(M + 1, NEG, dtype=np.int32); im = mm.copy(); dm = mm.copy()      # index k = node k, index 0 = nothing
    xN = sc["base_w"]
    xB, xJ, xC, best = xN + int(w_move), NEG, NEG, NEG
    for x in dsq:
        sv = clamp(xB + BM)
        sv = np.maximum(sv, clamp(mm[:-1] + MM))
        sv = np.maximum(sv, clamp(im[:-1] + IM))
        sv = np.maximum(sv, clamp(dm[:-1] + DM))
        sv = clamp(sv + e32[x])
        ni = np.maximum(clamp(mm[1:] + MI), clamp(im[1:] + II))
        nd = np.full(M + 1, NEG, dtype=np.int32)
        for k in range(2, M + 1):
            nd[k] = max(min(max(int(sv[k - 2]) + int(MD[k - 2]), NEG), POS), min(max(int(nd[k - 1]) + int(DD[k - 2]), NEG), POS))
        mm[1:], im[1:], dm = sv, ni, nd
        xE = int(sv.max())
        best = max(best, xE)
        if with_j:
            if xE >= POS:
                return POS, True
            xC = max(xC, xE + sc["wE_move"])
            xJ = max(xJ, xE + sc["wE_loop"])
            xB = max(xJ + int(w_move), xN + int(w_move))
    return (xC, False) if with_j else (best, None)


def vit_score(sc, xC, w_move, overflow):
    """((float)xC + (float)w_move - (float)base_w) / scale_w - 3 in float32, operation by operation."""
    if overflow:
        return np.float32(np.inf)
    if xC <= NEG:
        return np.float32(-np.inf)
    s = np.float32(np.float32(xC) + np.float32(w_move))
    s = np.float32(s - np.float32(sc["base_w"]))
    s = np.float32(s / np.float32(sc["scale_w"]))
    return np.float32(s - np.float32(3.0))


def gumbel_surv(x, mu, lam):
    y = lam * (x - mu)
    ey = -math.exp(-y) if y > -700 else -math.inf
    return -ey if abs(ey) < 5e-9 else 1.0 - math.exp(ey)


def passes(score, filtersc, mu, lam, F):
    """The pipeline's test in the oracle's precision: bits in float32 from a double division, the P-value in double."""
    with np.errstate(invalid="ignore"):
        bits = np.float32(float(np.float32(np.float32(score) - np.float32(filtersc))) / math.log(2.0))
    if np.isnan(bits):
        return False
    if np.isposinf(bits):
        return True
    if np.isneginf(bits):
        return False
    return not (gumbel_surv(float(bits), float(np.float32(mu)), float(np.float32(lam))) > F)


def threshold_bits(mu, lam, F):
    """The bit score at which the Gumbel tail equals F, in double."""
    return float(np.float32(mu)) - math.log(-math.log1p(-F)) / float(np.float32(lam))


def v_bits(score, filtersc):
    with np.errstate(invalid="ignore"):
        return (np.asarray(score, dtype=np.float64) - np.asarray(filtersc, dtype=np.float64)) * (1.0 / math.log(2.0))


class Pair(object):
    __slots__ = ("L", "w_move", "xE", "overflow", "xC", "flag", "fast", "exact", "exact_xC", "msv", "bias", "pass_fast", "pass_exact",
                 "pass_f1", "need_vit", "outcome", "plain_xC")


class ModelReference(object):
    """The reference of one model of an oracle HmmSet against digitized sequences."""

    def __init__(self, hs, index, stats):
        self.hs, self.index, self.M = hs, index, hs.M(index)
        self.mmu, self.mlam = float("%9.4f" % stats[0]), float("%8.5f" % stats[1])      # as the HMM file carries them
        self.vmu, self.vlam = float("%9.4f" % stats[2]), float("%8.5f" % stats[3])
        self.sc, self.emis, self.trans, _ = hs.vit_costs(index, [])
        self.thr_vit = threshold_bits(self.vmu, self.vlam, F2)
        self.thr_f1, self.thr_f2 = threshold_bits(self.mmu, self.mlam, F1), threshold_bits(self.mmu, self.mlam, F2)

    def w_move(self, lengths):
        return self.hs.vit_costs(self.index, lengths)[3]

    def pairs(self, dsqs):
        lengths = [len(d) for d in dsqs]
        wm = self.w_move(lengths)
        xE = p7.vit_fast(self.sc, self.emis, self.trans, wm, dsqs)
        xCj = p7.vit_fast(self.sc, self.emis, self.trans, wm, dsqs, with_j=True)
        st = self.hs.vit_stage(self.index, dsqs)
        out = []
        for i in range(len(dsqs)):
            p = Pair()
            p.L, p.w_move, p.xE = lengths[i], int(wm[i]), int(xE[i])
            p.overflow = p.xE >= POS
            p.xC = max(NEG, p.xE + self.sc["wE_move"])
            p.flag = int(p.xE + self.sc["wE_loop"] > self.sc["base_w"] and not p.overflow)
            p.fast = vit_score(self.sc, p.xC, p.w_move, p.overflow)
            p.exact, p.exact_xC, p.msv, p.bias = st["vit_sc"][i], int(st["vit_xC"][i]), st["msv_sc"][i], st["bias_sc"][i]
            p.plain_xC = int(xCj[i])                            # the with-J statement's C loop: the host test sets it against exact_xC
            p.pass_fast = passes(p.fast, p.bias, self.vmu, self.vlam, F2)
            p.pass_exact = bool(st["vit_ok"][i])
            p.pass_f1 = passes(p.msv, p.bias, self.mmu, self.mlam, F1)
            p.need_vit = bool(st["need_vit"][i])
            if p.overflow:
                p.outcome = "overflow"
            elif not p.flag:
                p.outcome = "pass_flag0" if p.pass_fast else "dead"
            elif p.pass_fast:
                p.outcome = "pass_flag1"
            else:
                p.outcome = "rerun_pass" if p.pass_exact else "rerun_fail"
            out.append(p)
        return out


# ---- the worlds: a model at either edge of every class, targets that fill the outcomes --------------------------------------------

def launch_classes():
    """[(label, kind, Q, [model lengths])]: each class's lower edge (the previous class's upper edge + 1, so that the last stripes hold
    out-of-model cells) and its upper edge; the shortest classes also take M = 5 and 9."""
    out, prev = [], 0
    for q in VIT16_Q:
        out.append(("vit16<%d>" % q, "vit16", q, [1, 5, 9, 32] if prev == 0 else [prev + 1, 32 * q]))
        prev = 32 * q
    prev = 0
    for q in WAVE_QH:
        out.append(("wave<%d>" % q, "wave", q, [1, 5, 9, 128] if prev == 0 else [prev + 1, 128 * q]))
        prev = 128 * q
    return out


def model_lengths():
    return sorted(set(m for _l, _k, _q, ms in launch_classes() for m in ms))


def make_profile(M):
    """A synthetic calibrated profile of M nodes, built as tests/test_gpu_scan.py::test_register_class_boundaries builds its own."""
    rng = np.random.default_rng(53000 + M)
    p = synth.random_profile(rng, M, "VIT%04d" % M, "PF%05d.1" % (80000 + M))
    p.stats = (-8.5 - 0.002 * M, 0.71, -9.5 - 0.002 * M, 0.71, -3.8, 0.71)
    return p


def _flanked(rng, core, lo=3, hi=9):
    return np.concatenate([synth.random_residues(rng, int(rng.integers(lo, hi))), core, synth.random_residues(rng, int(rng.integers(lo, hi)))])


def _fragment(rng, p, w):
    """A pass through w + 1 consecutive nodes somewhere in the model (the whole model when it is shorter)."""
    w = min(w, p.M - 1)
    a = int(rng.integers(1, p.M - w + 1))
    return synth.sample_domain(rng, p, a, a + w)


def base_targets(p):
    """(name, text) records of one model, without the graded two-fragment records (those need the reference: see targets())."""
    M = p.M
    rng = np.random.default_rng(92000 + M)
    recs = []
    for k, L in enumerate(RANDOM_LENGTHS):
        recs.append(("r%d_%d" % (L, k), synth.to_text(synth.random_residues(rng, L))))
    for k in range(7):                                                              # the company of the longest sequence in one wavefront
        recs.append(("tiny_%d" % k, synth.to_text(synth.random_residues(rng, 1))))
    recs += [("deg_bjzoux", "BJZOUX" * 20), ("deg_allx", "X" * 30 + "*"), ("deg_stop", "*"), ("deg_x3", "XXX"), ("deg_lower", "acdefghiklmnpqrstvwy" * 9 + "*"),
             ("deg_edge5", "BJZOUX*acdefghiklmnpqrstvwy")]
    for k in range(5):                                                              # full planted domains
        recs.append(("planted_%d" % k, synth.to_text(np.concatenate([synth.random_residues(rng, 7 + k), synth.sample_domain(rng, p), synth.random_residues(rng, 11 - k)])) + "*"))
    consensus = np.argmax(p.mat[1:] / synth.BGF, axis=1)
    recs.append(("consensus", synth.to_text(_flanked(rng, consensus))))
    recs.append(("consensus_x2", synth.to_text(np.concatenate([consensus, consensus]))))
    recs.append(("consensus_x3", synth.to_text(np.concatenate([consensus, synth.random_residues(rng, 4), consensus, consensus]))))
    # graded fragments between short flanks ...
    for w in list(range(1, 40)) + list(range(42, 83, 4)):
        recs.append(("frag_%d" % w, synth.to_text(_flanked(rng, _fragment(rng, p, w)))))
    # ... and in 1500 residues of noise (the bias filter's null score falls with the length: the F2 test passes on a weaker fragment)
    for w in range(1, 31, 2):
        core = _fragment(rng, p, w)
        recs.append(("fraglong_%d" % w, synth.to_text(np.concatenate([synth.random_residues(rng, 700), core, synth.random_residues(rng, 800 - len(core))]))))
    # two weak fragments in a row
    for w in range(2, 41, 2):
        recs.append(("double_%d" % w, synth.to_text(np.concatenate([synth.random_residues(rng, 4), _fragment(rng, p, w), synth.random_residues(rng, 5), _fragment(rng, p, w),
                                                                   synth.random_residues(rng, 4)]))))
    return recs


def _first(ref, make, lo, hi, pred):
    """Smallest a in [lo, hi] for which pred(the reference's pair of make(a)) holds, pred being monotone in a; None when it never holds."""
    one = lambda a: ref.pairs([p7.digitize(make(a))])[0]
    if not pred(one(hi)):
        return None
    while lo < hi:
        mid = (lo + hi) // 2
        if pred(one(mid)):
            hi = mid
        else:
            lo = mid + 1
    return lo


def targets(p, ref):
    """base_targets plus two families the reference places (a few bisections each), because the outcomes they fill are narrow:
    tail   two fragments in a row followed by a run of the residue that raises the bias filter's null score most: the run's length
           grades the pair from `the bound passes` through `the bound fails, the rerun passes` to `the rerun fails`;
    poor   3000 times the residue that lowers the null score most, then a prefix of a planted domain cut just before the J flag
           rises: the F2 test passes on a bound whose flag is clear (models of up to 1536 nodes; longer ones get there on fragments)."""
    recs = base_targets(p)
    rng = np.random.default_rng(78000 + p.M)
    probe = ref.hs.vit_stage(ref.index, [np.full(400, x, dtype=np.uint8) for x in range(20)])["bias_sc"]
    rich, poor = synth.to_text([int(np.argmax(probe))]), synth.to_text([int(np.argmin(probe))])
    A = 3000
    for rep in range(4):
        for w in (8, 12, 16, 24, 32, 48, 64):
            frag = _fragment(rng, p, w)                        # (the same fragment twice: both lift each other)
            core = synth.to_text(np.concatenate([synth.random_residues(rng, 4), frag, synth.random_residues(rng, 5), frag, synth.random_residues(rng, 3)]))
            ends = ref.pairs([p7.digitize(core), p7.digitize(core + rich * A)])
            if all(q.flag and q.xE >= 14000 for q in ends) or w >= p.M:      # (14000: the first fragment lifts the second by 3 bits or more)
                break
        if not all(q.flag for q in ends):
            continue
        make = lambda a: core + rich * a
        a0 = _first(ref, make, 0, A, lambda q: not q.pass_fast)
        if a0 is None:
            continue
        a1 = _first(ref, make, a0, A, lambda q: not q.pass_exact)
        a1 = A - 2 if a1 is None else a1
        for a in sorted(set(max(0, min(A, v)) for v in (a0 - 1, a0, (2 * a0 + a1) // 3, (a0 + 2 * a1) // 3, a1 - 1, a1, a1 + 1, a1 + 2))):
            recs.append(("tail%d_%d" % (rep, a), make(a)))
    if 9 <= p.M <= 128:
        # xE + wE_loop == base_w exactly: the last value whose flag is clear (a bound test written with >= would set it)
        cand = [synth.to_text(_flanked(rng, _fragment(rng, p, int(rng.integers(3, 24))), 1, 12)) for _ in range(6000)]
        dsq = [p7.digitize(t) for t in cand]
        xE = p7.vit_fast(ref.sc, ref.emis, ref.trans, ref.w_move([len(d) for d in dsq]), dsq)
        for k in np.nonzero(xE == ref.sc["base_w"] - ref.sc["wE_loop"])[0][:3]:
            recs.append(("edge_%d" % k, cand[k]))
    if p.M <= 1536:
        for rep in range(3):
            dom = synth.to_text(synth.sample_domain(rng, p))
            make = lambda i: poor * 3000 + dom[:i]
            hi = min(len(dom), 120)
            i1 = _first(ref, make, 1, hi, lambda q: bool(q.flag or q.overflow))
            i1 = hi + 1 if i1 is None else i1
            for i in range(max(1, i1 - 3), i1):
                recs.append(("poor%d_%d" % (rep, i), make(i)))
    return recs


def undecided(ref, q):
    """The pair is one the device's rules leave to either side: a score within the margin of a threshold it is tested against."""
    def near(score, thr, m):
        v = float(v_bits(score, q.bias))
        return math.isfinite(v) and abs(v - thr) <= m
    return near(q.msv, ref.thr_f1, MARGIN_MSV) or near(q.msv, ref.thr_f2, MARGIN_MSV) or near(q.fast, ref.thr_vit, MARGIN_VIT) or \
        (q.flag == 1 and near(q.exact, ref.thr_vit, MARGIN_VIT))


def coverage(pairs):
    """Outcome counts, the number of distinct xC values, the number of -inf scores."""
    counts = dict((o, 0) for o in OUTCOMES)
    for q in pairs:
        counts[q.outcome] += 1
    return counts, len(set(q.xC for q in pairs if not q.overflow)), sum(1 for q in pairs if q.xC <= NEG)


def coverage_met(counts, distinct):
    return all(counts[o] >= MIN_PER_OUTCOME for o in OUTCOMES) and distinct >= MIN_DISTINCT_XC


class World(object):
    """Every model of every class with its targets and the reference's pairs (built once per process)."""
    _instance = None

    def __init__(self):
        from tests import common
        self.lengths = model_lengths()
        self.profs = [make_profile(M) for M in self.lengths]
        self.path = common.hmm_file("vit_classes", self.profs)
        self.hs = p7.HmmSet(self.path)
        self.index = dict((M, i) for i, M in enumerate(self.lengths))
        self.refs, self.recs, self.dsq, self.pairs = {}, {}, {}, {}

        def one(Mp):
            M, p = Mp
            ref = ModelReference(self.hs, self.index[M], p.stats)
            recs = targets(p, ref)
            dsq = [p7.digitize(t) for _n, t in recs]
            return M, ref, recs, dsq, ref.pairs(dsq)
        with ThreadPoolExecutor(max_workers=12) as ex:                      # (the oracle's C loops release the interpreter lock)
            for M, ref, recs, dsq, pairs in ex.map(one, sorted(zip(self.lengths, self.profs), reverse=True)):
                self.refs[M], self.recs[M], self.dsq[M], self.pairs[M] = ref, recs, dsq, pairs

    @classmethod
    def get(cls):
        if cls._instance is None:
            cls._instance = World()
        return cls._instance

    def class_coverage(self):
        """[(label, lengths, outcome counts, distinct xC values, -inf scores)] per class, on the reference alone."""
        out = []
        for label, _kind, _q, ms in launch_classes():
            counts, distinct, ninf = coverage([q for M in ms for q in self.pairs[M]])
            out.append((label, ms, counts, distinct, ninf))
        return out
