"""A plain float64 reference of the float half of the scan (checkm_amd/csrc/kernels_fb.hip: fwd_kernel<Q>, bwd_kernel<Q>, oa_kernel<Q>;
kernels_cascade.hip: region_kernel; the device bias filter), the world it is tested on and the tolerances it is held to.

Never imports checkm_amd.  From the project it takes the alphabet codes (oracle.p7.digitize), the generators and the background of
synthdata.synth, and the HMM text, which it parses itself: a parameter is exp(-float(token)) of the file's %8.5f field, `*` is 0.  It shares
no canonical order, no padded layout, no expf table and no rescaling rule with oracle/p7oracle.c or the kernels.

Profile   occ[1] = t0.MM + t0.MI, occ[k] = occ[k-1] (MM + MI)[k-1] + (1 - occ[k-1]) DM[k-1];  B -> M_k = occ[k] / sum_i occ[i] (M - i + 1);
          every M_k and D_k reaches E at cost 1; node M has no MI, II, MD, DD; match odds mat[k][x] / BGF[x], insert odds 1; a degenerate
          code's odds are exp of the BGF-weighted mean log-odds of its members; gap, `*`, `~` have odds 0.
Specials  move = (2 + nj) / (L + 2 + nj), loop = 1 - move (N, J, C), nj = 1 multihit, 0 unihit;  E -> C = E -> J = 1/2 multihit; E -> C = 1 unihit.
Forward   M(i,k) = odds_k(x_i) (B(i-1) BM_k + M(i-1,k-1) MM_{k-1} + I(i-1,k-1) IM_{k-1} + D(i-1,k-1) DM_{k-1})
          I(i,k) = M(i-1,k) MI_k + I(i-1,k) II_k;   D(i,k) = M(i,k-1) MD_{k-1} + D(i,k-1) DD_{k-1};   E(i) = sum_k M(i,k) + D(i,k)
          N(i) = N(i-1) loop;  J(i) = J(i-1) loop + E(i) EJ;  C(i) = C(i-1) loop + E(i) EC;  B(i) = (N(i) + J(i)) move;  score = log(C(L) move).
Backward  the same graph read from the end: C(L) = move, E(L) = C(L) EC, ...; its N(0) is the same total.
Decoding  P(M_k emits i) = fM(i,k) bM(i,k) / Z; P(N emits i) = fN(i-1) loop bN(i) / Z, likewise J and C; the five sum to 1 per residue.
null2     odds of residue x under the envelope's state usage: sum_k me[k] odds_k(x) + ie[k] + (xN + xJ + xC) / Ld.
OA        the path of largest summed posterior over transitions of probability > 0; its score oC(Ld), the trace's coordinates, the residue
          of every match node on it and the posterior of every residue on it in the state that emits it (the alignment and its PP line).
Regions   mocc(i) = 1 - P(N, J or C emits i), btot / etot the cumulated use of B and E; thresholds 0.25, 0.1, 0.2 as HMMER's
          p7_domaindef_ByPosteriorHeuristics applies them.
Bias      Forward of the two-state model (background, model composition) as odds against the background, plus the length model.

forward_numpy ... envelope_numpy below are the definition, one row at a time; the bulk runs through the same recurrences as a scalar C loop
(oracle/fb_plain.c through oracle.p7.fb_plain(), which takes the arrays parsed here), and tests/test_fb_reference_host.py holds the two
together to 1e-12.  Ranges are kept by exact powers of two with the exponent beside the row, so nothing here depends on a scaling rule.
Where one exponent per row is not enough even in float64 (a unihit envelope that spans two copies of a long model: consistent() notices),
the same statement runs in WIDE.
"""
import math
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from oracle import p7
from synthdata import synth

KFB_Q = [1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64]            # fwd_kernel<Q>: models of up to 64 * Q nodes
RANDOM_LENGTHS = [1, 2, 3, 17, 63, 64, 65, 300]
RT1, RT2, RT3 = 0.25, 0.1, 0.2
RESCALE_AT = 1.0e4                                           # the kernels' Forward rescales a row whose xE exceeds this
RESCALE_BAND = 1e-3                                          # ... and a pair whose xE comes this close (relative) is left undecided
EPS32 = 2.0 ** -24
WIDE = np.longdouble                                         # the envelopes' reference (see forward_numpy): float64's mantissa or more, a wider exponent
MM, MI, MD, IM, II, DM, DD = range(7)
MEMBERS = {21: "DN", 22: "IL", 23: "EQ", 24: "K", 25: "C", 26: synth.AMINO}   # B J Z O U X of oracle.p7.digitize's codes; 20 gap, 27 *, 28 ~


# ---- the HMM text ------------------------------------------------------------------------------------------------------------------

def _probs(tokens):
    return np.array([0.0 if t == "*" else math.exp(-float(t)) for t in tokens])


def parse_hmm(text):
    """[dict(name, M, mat[M+1][20], t[M+1][7], compo[20])] of every record of an HMMER3 ASCII file, as probabilities in float64."""
    out = []
    for rec in text.split("\n//"):
        lines = [ln for ln in rec.split("\n") if ln.strip()]
        if not lines:
            continue
        head = dict((ln.split()[0], ln.split(None, 1)[1]) for ln in lines if len(ln.split()) > 1 and ln.split()[0] in ("NAME", "LENG"))
        at = next(k for k, ln in enumerate(lines) if ln.startswith("HMM ")) + 2
        M = int(head["LENG"])
        compo = None
        if lines[at].split()[0] == "COMPO":
            compo = _probs(lines[at].split()[1:21]); at += 1
        mat, t = np.zeros((M + 1, 20)), np.zeros((M + 1, 7))
        t[0] = _probs(lines[at + 1].split()[:7]); at += 2
        for k in range(1, M + 1):
            f = lines[at].split()
            assert int(f[0]) == k
            mat[k] = _probs(f[1:21]); t[k] = _probs(lines[at + 2].split()[:7]); at += 3
        out.append(dict(name=head["NAME"].strip(), M=M, mat=mat, t=t, compo=compo))
    return out


class Model(object):
    """The configured local profile of one parsed record.  cfg(dtype) configures it with every array and scalar in that type: the file's
    parameters rounded to it, then the occupancy recurrence, the entry distribution and the odds computed in it."""

    def __init__(self, rec):
        self.rec, self.M = rec, rec["M"]
        self._cfg = {}
        c = self.cfg(np.float64)
        self.bm, self.t, self.odds, self.bias_p, self.eo1 = c["bm"], c["t"], c["odds"], c["bias_p"], c["eo1"]

    def _configure(self, dt):
        M, rec = self.M, self.rec
        t, mat, compo, bgf = rec["t"].astype(dt), rec["mat"].astype(dt), rec["compo"].astype(dt), synth.BGF.astype(dt)
        occ = np.zeros(M + 1, dtype=dt)
        occ[1] = t[0, MM] + t[0, MI]
        for k in range(2, M + 1):
            occ[k] = occ[k - 1] * (t[k - 1, MM] + t[k - 1, MI]) + (dt(1) - occ[k - 1]) * t[k - 1, DM]
        bm = np.zeros(M + 1, dtype=dt)
        bm[1:] = occ[1:] / _ksum(occ[1:] * (M - np.arange(1, M + 1) + 1).astype(dt))
        t[M, [MI, II, MD, DD]] = 0
        odds = np.zeros((29, M + 1), dtype=dt)
        odds[:20, 1:] = (mat[1:] / bgf).T
        with np.errstate(divide="ignore"):
            lo = np.log(mat[1:] / bgf)                                   # [M][20]
        for x, members in MEMBERS.items():
            idx = [synth.AMINO.index(a) for a in members]
            w = bgf[idx]
            odds[x, 1:] = np.exp((lo[:, idx] * w).sum(axis=1) / w.sum())
        # the bias filter's two-state model: state 0 emits the background and stays 400 residues on average, state 1 emits the model's
        # composition and stays M / 8; it starts in state 0 with probability 0.999 and either state ends at cost 1
        L0, L1 = dt(400), dt(M) / dt(8)
        bias_p = np.array([L0 / (L0 + 1), 1 / (L0 + 1), 1 / (L1 + 1), L1 / (L1 + 1), dt(0.999), dt(0.001)], dtype=dt)
        eo1 = np.ones(29, dtype=dt)
        eo1[:20] = compo / bgf
        for x, members in MEMBERS.items():
            idx = [synth.AMINO.index(a) for a in members]
            eo1[x] = compo[idx].sum() / bgf[idx].sum()
        return dict(M=M, dtype=dt, bm=np.ascontiguousarray(bm), t=np.ascontiguousarray(t), odds=np.ascontiguousarray(odds), bias_p=bias_p, eo1=eo1)

    def cfg(self, dtype=np.float64):
        if dtype not in self._cfg:
            self._cfg[dtype] = self._configure(dtype)
        return self._cfg[dtype]


def specials(L, multihit, dtype=np.float64):
    """[move, loop, E->J, E->C] for a sequence of L residues."""
    nj = dtype(1.0 if multihit else 0.0)
    move = (dtype(2.0) + nj) / (dtype(L) + dtype(2.0) + nj)
    return np.array([move, dtype(1.0) - move, 0.5 if multihit else 0.0, 0.5 if multihit else 1.0], dtype=dtype)


def null_score(L, dtype=np.float64):
    """L log(L / (L + 1)) + log(1 / (L + 1))."""
    p1 = dtype(L) / dtype(L + 1)
    return dtype(L) * np.log(p1) + np.log(dtype(1.0) - p1)


# ---- the numpy statement (the definition) -------------------------------------------------------------------------------------------

def _ksum(a):
    """Sum in plain k order, in the array's own precision."""
    return np.cumsum(a)[-1] if len(a) else a.dtype.type(0)


def _down(arrs, scalars, top):
    """Multiply a row by the exact power of two that brings `top` to [1, 2); returns the exponent taken out."""
    d = -int(math.floor(math.log2(float(top))))
    return [np.ldexp(a, d) for a in arrs], [s.dtype.type(np.ldexp(s, d)) for s in scalars], -d


def _out_of_range(top):
    return top > 2.0 ** 30 or 0 < top < 2.0 ** -30


def _sc(v, d):
    return v.dtype.type(np.ldexp(v, int(d)))


def forward_numpy(c, sp, dsq):
    """(score, fM[L+1][M+1], fI, xs[L+1][5] = E N J B C, ex[L+1], exc[L+1], lxe[L+1]).  Rows as stored: the core cells, E, J and B are
    true value / 2^ex; N is its true value; C is true value / 2^exc (an exponent of its own: in a unihit envelope that holds two domains C
    carries the first one's mass while the second one's cells still descend from N, further apart than one exponent per row can hold)."""
    M, dt, t, bm = c["M"], c["dtype"], c["t"], c["bm"]
    move, loop, ej, ec = sp
    L = len(dsq)
    fM, fI = np.zeros((L + 1, M + 1), dtype=dt), np.zeros((L + 1, M + 1), dtype=dt)
    xs, ex, exc, lxe = np.zeros((L + 1, 5), dtype=dt), np.zeros(L + 1, dtype=np.int32), np.zeros(L + 1, dtype=np.int32), np.full(L + 1, -np.inf)
    pM, pI, pD = (np.zeros(M + 1, dtype=dt) for _ in range(3))
    xN, xJ, xC = dt(1), dt(0), dt(0)
    xB, e, eC = xN * move, 0, 0
    xs[0] = [0, xN, 0, xB, 0]
    for i in range(1, L + 1):
        o = c["odds"][dsq[i - 1]]
        cM, cI, cD = (np.zeros(M + 1, dtype=dt) for _ in range(3))
        cM[1:] = (xB * bm[1:] + pM[:-1] * t[:-1, MM] + pI[:-1] * t[:-1, IM] + pD[:-1] * t[:-1, DM]) * o[1:]
        cI[1:] = pM[1:] * t[1:, MI] + pI[1:] * t[1:, II]
        for k in range(2, M + 1):
            cD[k] = cM[k - 1] * t[k - 1, MD] + cD[k - 1] * t[k - 1, DD]
        xE = _ksum(cM[1:] + cD[1:])
        xN = xN * loop
        xJ = xJ * loop + xE * ej
        ne = eC if (xC > 0 and eC > e) else e
        xC, eC = _sc(xC, eC - ne) * loop + _sc(xE, e - ne) * ec, ne
        xB = (_sc(xN, -e) + xJ) * move
        if xC > 2.0 ** 30:
            _, (xC,), de = _down([], [xC], xC)
            eC += de
        top = max(float(xE), float(xB))
        if top < 2.0 ** -30:
            top = max(top, float(cI.max()))
        if _out_of_range(top):
            (cM, cI, cD), (xE, xJ, xB), de = _down([cM, cI, cD], [xE, xJ, xB], top)
            e += de
        fM[i], fI[i], xs[i], ex[i], exc[i] = cM, cI, [xE, xN, xJ, xB, xC], e, eC
        lxe[i] = math.log(float(xE)) + e * math.log(2.0) if xE > 0 else -np.inf
        pM, pI, pD = cM, cI, cD
    with np.errstate(divide="ignore"):
        score = float(np.log(np.float64(xC * move))) + eC * math.log(2.0)
    return score, fM, fI, xs, ex, exc, lxe


def backward_numpy(c, sp, dsq):
    """(bM[L+1][M+2], bI, xb[L+1][5] = E N J B C, eb[L+1], ebn[L+1]).  Rows as stored: the core cells, E, J and B are true value / 2^eb; C is its
    true value; N is true value / 2^ebn."""
    M, dt, t, bm = c["M"], c["dtype"], c["t"], c["bm"]
    move, loop, ej, ec = sp
    L = len(dsq)
    bM, bI = np.zeros((L + 1, M + 2), dtype=dt), np.zeros((L + 1, M + 2), dtype=dt)
    xb, eb, ebn = np.zeros((L + 1, 5), dtype=dt), np.zeros(L + 1, dtype=np.int32), np.zeros(L + 1, dtype=np.int32)
    xC, xJ, xN, xB = move, dt(0), dt(0), dt(0)
    xE = xC * ec + xJ * ej
    cM, cI, cD = (np.zeros(M + 2, dtype=dt) for _ in range(3))
    for k in range(M, 0, -1):
        cD[k] = xE + t[k, DD] * cD[k + 1]
        cM[k] = xE + t[k, MD] * cD[k + 1]
    bM[L], bI[L], xb[L], e, eN = cM, cI, [xE, xN, xJ, xB, xC], 0, 0
    for i in range(L - 1, -1, -1):
        nM, nI = cM, cI
        mn = np.zeros(M + 2, dtype=dt)
        mn[1:M + 1] = nM[1:M + 1] * c["odds"][dsq[i]][1:]
        xB = _ksum(bm[1:] * mn[1:M + 1])
        xJ = xB * move + xJ * loop
        xC = xC * loop
        xE = _sc(xC, -e) * ec + xJ * ej
        ne = eN if (xN > 0 and eN > e) else e
        xN, eN = _sc(xB, e - ne) * move + _sc(xN, eN - ne) * loop, ne
        cM, cI, cD = (np.zeros(M + 2, dtype=dt) for _ in range(3))
        for k in range(M, 0, -1):
            cD[k] = xE + t[k, DM] * mn[k + 1] + t[k, DD] * cD[k + 1]
        cI[1:M + 1] = t[1:, IM] * mn[2:] + t[1:, II] * nI[1:M + 1]
        cM[1:M + 1] = xE + t[1:, MM] * mn[2:] + t[1:, MI] * nI[1:M + 1] + t[1:, MD] * cD[2:]
        top = max(float(cM.max()), float(cI.max()), float(cD.max()), float(xE), float(xJ), float(xB))
        if _out_of_range(top):
            (cM, cI, cD), (xE, xJ, xB), de = _down([cM, cI, cD], [xE, xJ, xB], top)
            e += de
        if xN > 2.0 ** 30:
            _, (xN,), de = _down([], [xN], xN)
            eN += de
        bM[i], bI[i], xb[i], eb[i], ebn[i] = cM, cI, [xE, xN, xJ, xB, xC], e, eN
    return bM, bI, xb, eb, ebn


def _specials_posterior(xs, ex, exc, xb, eb, ebn, i, loop, z, ez):
    """P(N emits i), P(J emits i), P(C emits i)."""
    return np.array([_sc(xs[i - 1, 1] * loop * xb[i, 1] / z, int(ebn[i]) - ez), _sc(xs[i - 1, 2] * loop * xb[i, 2] / z, int(ex[i - 1]) + int(eb[i]) - ez),
                     _sc(xs[i - 1, 4] * loop * xb[i, 4] / z, int(exc[i - 1]) - ez)])


def envelope_numpy(c, sp, dsq):
    """Forward, Backward, decoding, null2 and optimal accuracy of one envelope's residues: dict(envsc, btotal, ppM, ppI, ppX[Ld+1][3] = N J C,
    null2[20], oasc, coords = (hmm_from, hmm_to, ali_from, ali_to) envelope-local, gap, path[M+1] = the envelope-local residue match node k
    emits on the trace (0: none), pp_path[Ld+1] = the posterior of residue i in the state that emits it on the trace (M or I; 0 off
    ali_from..ali_to), flank = the posteriors the trace collects outside the core (C's behind the last match state, N's before the first):
    sum(pp_path) + flank is oasc)."""
    M, dt, t, bm = c["M"], c["dtype"], c["t"], c["bm"]
    Ld = len(dsq)
    envsc, fM, fI, xs, ex, exc, _ = forward_numpy(c, sp, dsq)
    bM, bI, xb, eb, ebn = backward_numpy(c, sp, dsq)
    z, ez = xs[Ld, 4] * sp[0], int(exc[Ld])
    ppM, ppI, ppX = np.zeros((Ld + 1, M + 1), dtype=dt), np.zeros((Ld + 1, M + 1), dtype=dt), np.zeros((Ld + 1, 3), dtype=dt)
    for i in range(1, Ld + 1):
        d = int(ex[i]) + int(eb[i]) - ez
        ppM[i] = np.ldexp(fM[i] * bM[i, :M + 1] / z, d)
        ppI[i] = np.ldexp(fI[i] * bI[i, :M + 1] / z, d)
        ppX[i] = _specials_posterior(xs, ex, exc, xb, eb, ebn, i, sp[1], z, ez)
    me, ie = np.zeros(M + 1, dtype=dt), np.zeros(M + 1, dtype=dt)
    xfac = dt(0)
    for i in range(Ld, 0, -1):                                      # (accumulated from the last residue, as the rolling Backward meets them)
        me, ie = me + ppM[i], ie + ppI[i]
        xfac = xfac + (ppX[i, 0] + ppX[i, 1] + ppX[i, 2])
    null2 = np.array([float(_ksum(me[1:] / dt(Ld) * c["odds"][x][1:] + ie[1:] / dt(Ld)) + xfac / dt(Ld)) for x in range(20)])
    # optimal accuracy
    NEG = dt(-np.inf)
    gate = lambda p, v: np.where(p > 0, v, NEG)
    oM, oI, oD = (np.full((Ld + 1, M + 1), NEG, dtype=dt) for _ in range(3))
    oN, oB, oE, oJ, oC = (np.full(Ld + 1, NEG, dtype=dt) for _ in range(5))
    oN[0] = oB[0] = 0
    for i in range(1, Ld + 1):
        best = gate(bm[1:], oB[i - 1])
        best = np.maximum(best, gate(t[:-1, MM], oM[i - 1, :-1]))
        best = np.maximum(best, gate(t[:-1, IM], oI[i - 1, :-1]))
        best = np.maximum(best, gate(t[:-1, DM], oD[i - 1, :-1]))
        oM[i, 1:] = best + ppM[i, 1:]
        oI[i, 1:] = np.maximum(gate(t[1:, MI], oM[i - 1, 1:]), gate(t[1:, II], oI[i - 1, 1:])) + ppI[i, 1:]
        for k in range(2, M + 1):
            oD[i, k] = max(oM[i, k - 1] if t[k - 1, MD] > 0 else NEG, oD[i, k - 1] if t[k - 1, DD] > 0 else NEG)
        oE[i] = oM[i, 1:].max()
        oJ[i] = max(oJ[i - 1] + ppX[i, 1], oE[i] if sp[2] > 0 else NEG)
        oC[i] = max(oC[i - 1] + ppX[i, 2], oE[i] if sp[3] > 0 else NEG)
        oN[i] = oN[i - 1] + ppX[i, 0]
        oB[i] = max(oN[i], oJ[i])
    gap = [np.inf]

    def upd(vals):
        v = sorted((float(x) for x in vals), reverse=True)
        if len(v) > 1 and v[1] > -np.inf:
            gap[0] = min(gap[0], v[0] - v[1])
    i, k, st, first, last = Ld, 0, "C", (0, 0), (0, 0)
    path, pp_path, flank = np.zeros(M + 1, dtype=np.int32), np.zeros(Ld + 1), 0.0
    while True:
        if st == "C":
            if i == 0:
                break
            a, b = oC[i - 1] + ppX[i, 2], oE[i]
            upd([a, b])
            if a >= b:
                flank += float(ppX[i, 2])
                i -= 1
            else:
                st = "E"
        elif st == "E":
            k = int(np.argmax(oM[i, 1:])) + 1
            if not oM[i, k] > -np.inf:
                break
            upd(oM[i, 1:])
            last, st = (i, k), "M"
        elif st == "M":
            first = (i, k)
            path[k], pp_path[i] = i, float(ppM[i, k])
            cand = [oM[i - 1, k - 1] if t[k - 1, MM] > 0 else NEG, oI[i - 1, k - 1] if t[k - 1, IM] > 0 else NEG,
                    oD[i - 1, k - 1] if t[k - 1, DM] > 0 else NEG, oB[i - 1] if bm[k] > 0 else NEG]
            upd(cand)
            b = int(np.argmax(cand))
            i -= 1
            if b == 3:
                flank += sum(float(v) for v in ppX[1:i + 1, 0])
                break
            k, st = k - 1, "MID"[b]
        elif st == "I":
            a, b = (oM[i - 1, k] if t[k, MI] > 0 else NEG), (oI[i - 1, k] if t[k, II] > 0 else NEG)
            upd([a, b])
            pp_path[i] = float(ppI[i, k])
            i, st = i - 1, ("M" if a >= b else "I")
        else:
            a, b = (oM[i, k - 1] if t[k - 1, MD] > 0 else NEG), (oD[i, k - 1] if t[k - 1, DD] > 0 else NEG)
            upd([a, b])
            k, st = k - 1, ("M" if a >= b else "D")
    with np.errstate(divide="ignore"):
        btotal = math.log(float(xb[0, 1])) + int(ebn[0]) * math.log(2.0)
    return dict(envsc=envsc, btotal=btotal, ppM=ppM, ppI=ppI, ppX=ppX, null2=null2, oasc=float(oC[Ld]),
                coords=(first[1], last[1], first[0], last[0]), gap=gap[0], path=path, pp_path=pp_path, flank=flank)


def occupancy_numpy(c, sp, dsq):
    """(mocc, bt, et)[L+1] of the whole sequence (index 0 unused)."""
    L = len(dsq)
    _, _fM, _fI, xs, ex, exc, _ = forward_numpy(c, sp, dsq)
    _bM, _bI, xb, eb, ebn = backward_numpy(c, sp, dsq)
    z, ez = xs[L, 4] * sp[0], int(exc[L])
    mocc, bt, et = np.zeros(L + 1), np.zeros(L + 1), np.zeros(L + 1)
    for i in range(1, L + 1):
        et[i] = np.ldexp(xs[i, 0] * xb[i, 0] / z, int(ex[i]) + int(eb[i]) - ez)
        bt[i] = np.ldexp(xs[i - 1, 3] * xb[i - 1, 3] / z, int(ex[i - 1]) + int(eb[i - 1]) - ez)
        n, j, cc = _specials_posterior(xs, ex, exc, xb, eb, ebn, i, sp[1], z, ez)
        mocc[i] = c["dtype"](1) - (n + j + cc)
    return mocc, bt, et


def bias_numpy(c, dsq):
    """log of the two-state model's Forward total, as odds against the background (at least one residue)."""
    p, eo1 = c["bias_p"], c["eo1"]
    d0, d1, e = p[4], p[5] * eo1[dsq[0]], 0
    for x in dsq[1:]:
        d0, d1 = d0 * p[0] + d1 * p[2], (d0 * p[1] + d1 * p[3]) * eo1[x]
        top = max(d0, d1)
        if top > 2.0 ** 30 or 0 < top < 2.0 ** -30:
            _, (d0, d1), de = _down([], [d0, d1], top)
            e += de
    return math.log(float(d0 + d1)) + e * math.log(2.0)


# ---- the same recurrences through the C loop ----------------------------------------------------------------------------------------

def _sfx(c):
    return {np.float64: "_f64", np.float32: "_f32", np.longdouble: "_f80"}[c["dtype"]]


def _model_args(c, sp):
    return (c["M"], c["bm"].ctypes.data, c["t"].ctypes.data, c["odds"].ctypes.data, sp.ctypes.data)


def forward_c(c, sp, dsq):
    """(score, lxe[L+1])."""
    d = np.ascontiguousarray(dsq, dtype=np.uint8)
    out, lxe = np.zeros(1), np.zeros(len(d) + 1)
    getattr(p7.fb_plain(), "fbp_forward" + _sfx(c))(*_model_args(c, sp), d.ctypes.data, len(d), out.ctypes.data, lxe.ctypes.data)
    return float(out[0]), lxe


def occupancy_c(c, sp, dsq):
    """(Forward score, Backward total, mocc, bt, et)."""
    d = np.ascontiguousarray(dsq, dtype=np.uint8)
    out = np.zeros(2)
    mocc, bt, et = (np.zeros(len(d) + 1) for _ in range(3))
    getattr(p7.fb_plain(), "fbp_occupancy" + _sfx(c))(*_model_args(c, sp), d.ctypes.data, len(d), out.ctypes.data, mocc.ctypes.data, bt.ctypes.data, et.ctypes.data)
    return float(out[0]), float(out[1]), mocc, bt, et


def envelope_c(c, sp, dsq, keep=False):
    """envelope_numpy's dictionary (plus rowdev, the largest |sum of a residue's posteriors - 1|); the matrices only with keep."""
    d = np.ascontiguousarray(dsq, dtype=np.uint8)
    Ld, M, dt = len(d), c["M"], c["dtype"]
    ppM, ppI, ppX = np.zeros((Ld + 1, M + 1), dtype=dt), np.zeros((Ld + 1, M + 1), dtype=dt), np.zeros((Ld + 1, 3), dtype=dt)
    null2, coords, out = np.zeros(20), np.zeros(4, dtype=np.int32), np.zeros(6)
    lxe, lbt = np.zeros(Ld + 1), np.zeros(Ld + 1)
    path, pp_path = np.zeros(M + 1, dtype=np.int32), np.zeros(Ld + 1)
    getattr(p7.fb_plain(), "fbp_envelope" + _sfx(c))(*_model_args(c, sp), d.ctypes.data, Ld, ppM.ctypes.data, ppI.ctypes.data, ppX.ctypes.data,
                                                     null2.ctypes.data, coords.ctypes.data, out.ctypes.data, lxe.ctypes.data, lbt.ctypes.data,
                                                     path.ctypes.data, pp_path.ctypes.data)
    r = dict(lxe=lxe, lbt=lbt, envsc=float(out[0]), btotal=float(out[1]), rowdev=float(out[2]), null2=null2, oasc=float(out[3]), coords=tuple(int(v) for v in coords),
             gap=float(out[4]), ppX=ppX, path=path, pp_path=pp_path, flank=float(out[5]))
    if keep:
        r["ppM"], r["ppI"] = ppM, ppI
    return r


def consistent(r, tol=1e-9):
    """Whether an evaluation of an envelope hangs together: every residue's posteriors sum to 1 and Backward's total is Forward's.  One
    that left its number format's range does not (World falls back to WIDE then; measure_tolerances leaves a float32 evaluation out)."""
    return r["rowdev"] <= tol and abs(r["btotal"] - r["envsc"]) <= tol * max(1.0, abs(r["envsc"]))


def bias_c(c, dsq):
    d = np.ascontiguousarray(dsq, dtype=np.uint8)
    out = np.zeros(1)
    getattr(p7.fb_plain(), "fbp_bias" + _sfx(c))(c["bias_p"].ctypes.data, c["eo1"].ctypes.data, d.ctypes.data, len(d), out.ctypes.data)
    return float(out[0])


def bias_score(c, dsq):
    """The bias filter's null score: the two-state total plus the length model, in the configuration's precision."""
    dt, L = c["dtype"], len(dsq)
    p1 = dt(L) / dt(L + 1)
    return float(dt(bias_c(c, dsq)) + dt(L) * np.log(p1) + np.log(dt(1) - p1))


def regions_of(mocc, bt, et):
    """([(i, j, multi, margin)], tail): the regions of one sequence, whether rt3 sends each to the trace ensemble, the smallest margin of
    any threshold comparison that shaped it (rt3's included); tail = the smallest margin of the comparisons after the last region."""
    L = len(mocc) - 1
    btot, etot = np.cumsum(bt), np.cumsum(et)
    out, i, trig, margin = [], -1, False, np.inf
    for j in range(1, L + 1):
        if not trig:
            v = mocc[j] - bt[j]
            margin = min(margin, abs(v - RT2), abs(mocc[j] - RT1))
            if v < RT2:
                i = j
            elif i == -1:
                i = j
            if mocc[j] >= RT1:
                trig = True
        else:
            v = mocc[j] - et[j]
            margin = min(margin, abs(v - RT2))
            if v < RT2:
                z = np.arange(i, j + 1)
                top = float(np.minimum(etot[z] - etot[i - 1], btot[j] - btot[z - 1]).max())
                out.append((i, j, top >= RT3, min(margin, abs(top - RT3))))
                i, trig, margin = -1, False, np.inf
    return out, margin


def expected_nscale(lxe):
    """(number of rescale events of a Forward that divides a row by its xE whenever that exceeds RESCALE_AT, whether any comparison came
    within RESCALE_BAND of the threshold), from the true log xE of every row."""
    base, n, close = 0.0, 0, False
    thr = math.log(RESCALE_AT)
    for v in lxe[1:]:
        if abs(v - base - thr) <= RESCALE_BAND:
            close = True
        if v - base > thr:
            base, n = v, n + 1
    return n, close


FLT_MAX_LOG = math.log(float(np.finfo(np.float32).max))


def backward_overflow(lxe, lbt):
    """By how many nats the largest value a float32 Backward must hold exceeds float32's largest number (positive: it overflows), from
    the true magnitudes of the reference's rows.  The kernels' Backward divides row i by the factors Forward rescaled rows i + 1 .. Ld by
    (Forward divides a row by its xE whenever that exceeds RESCALE_AT), and computes the row before it divides by row i + 1's factor: so the
    value it must hold at row i is the true one over the product of the factors of rows i + 2 .. Ld.  Where Forward saw nothing to rescale --
    the second copy of a two-copy envelope, whose cells lie under the first copy's leftovers -- Backward's values grow unchecked."""
    base, cum = 0.0, np.zeros(len(lxe))
    thr = math.log(RESCALE_AT)
    for i in range(1, len(lxe)):
        if lxe[i] - base > thr:
            base = lxe[i]
        cum[i] = base
    Ld = len(lxe) - 1
    after = cum[Ld] - cum[np.minimum(np.arange(Ld + 1) + 1, Ld)]
    return float(np.max(lbt - after)) - FLT_MAX_LOG


def whole_overflow(model, dsq):
    """backward_overflow of the unihit span (1, L) of a whole sequence against a Model: positive where an alignment of the sequence
    (ckm_align, the oracle's p7o_align) must be refused.  The sequence must have a finite Forward score."""
    L = len(dsq)
    r = envelope_c(model.cfg(), specials(L, False), dsq)
    if not consistent(r):
        r = envelope_c(model.cfg(WIDE), specials(L, False, WIDE), dsq)
    return backward_overflow(r["lxe"], r["lbt"])


# ---- tolerances ---------------------------------------------------------------------------------------------------------------------
# |got - ref64| <= K (Ld + 1) 2^-24 + 2 ulp32(|ref64|) nats for scores; |got / ref64 - 1| <= K_N2 (Ld + 1) 2^-24 for the null2 odds.
# Each K is 4 x the largest ratio measure_tolerances() observes between the float32 and the float64 evaluation of the recurrences above
# over the whole world, rounded up to a power of two (the factor 4: the kernels sum in another association -- 64-lane blocks, Kogge-Stone
# D chain, xor butterfly -- and use expf-rounded tables, both of the order of the plain float32 run and no larger).
# tests/test_fb_reference_host.py measures again and fails if a ratio exceeds K / 4.
#
# Excused, by an exact condition computed in the reference (backward_overflow() > 0): the envelopes in which a float32 Backward that is
# scaled by Forward's factors must hold a value above float32's largest number.  They are the spans (1, L) and (5, L - 3) of the two-copy
# targets of the models of 192 nodes and more (38 envelopes, each at least 2 nats beyond the limit): Forward's cells of the second copy
# lie under the first copy's leftovers, so Forward rescales nothing there and Backward's values grow by the second copy's whole score.
# The kernels must answer these with ok = 0 (HMMER answers eslERANGE) and every other envelope with ok = 1; the float32 evaluation of the
# reference hangs together (consistent() with F32_CONSISTENT) on exactly the others, which the host test asserts, and only those enter
# the measurement: beyond its range a float32 run measures no rounding.
#
# K_GAP is the constant of the trace's runner-up gap: an envelope's coordinates are undecided when the reference's gap is below
# K_GAP (Ld + 1) 2^-24.  The OA score's own tolerance is not used for this: the float32 error of an OA cell grows with Ld^2 (a sum of Ld
# posteriors, each off by a multiple of Ld rounding errors), so K_OA is set by the longest envelopes and at their lengths its tolerance
# (0.06 at Ld = 1000) exceeds most gaps -- 126 of the 328 envelopes would be undecided.  The gap is a difference of two cells that share
# their predecessors' errors, and it is measured like every other figure here: float32 against float64 evaluation, 4 x, a power of two.
# This excuses fewer envelopes, never more (K_GAP < K_OA).
#
# K_REG is the constant of the region scan's threshold margins, in a unit of its own: a region is undecided when the smallest margin of
# a comparison that shaped it is below K_REG 2^-24.  mocc, btot and etot are posterior probabilities in [0, 1] (the cumulated ones sums of
# them over a region), normalised by Z, and their float32 error does not grow with the length as a score's does: the largest, 207 units of
# 2^-24, is at L = 1152 and not at L = 12288, while at L = 1 against a long model it is 32 units -- in the unit (L + 1) 2^-24 those 32
# would set the constant and leave 39 of 398 regions undecided.  Measured like the others (per residue and cumulated, float32 against
# float64, 4 x, a power of two).
#
# K_PP is the constant of the posterior line of the OA path (pp_path: the posterior of every residue on the path in the state that emits
# it), in K_REG's unit: |got - ref64| <= K_PP 2^-24 per residue.  A posterior lies in [0, 1] and is normalised by Z like mocc.  Measured
# like the others over the decided envelopes (there both evaluations trace the same path, so the same cells are compared): the float32
# error does grow with the envelope, but far slower than its length -- the largest per length class is 4 units at Ld < 32, 25 at
# Ld = 32 .. 127, 67 at Ld = 512 .. 1023 and 177 at Ld = 3084 (M = 3073), about the square root of Ld.  In the unit (Ld + 1) 2^-24 the
# largest ratio, 0.72, is set by an envelope of two residues and would give the constant 4: 9.8e-4 at Ld = 4100, sixteen times what
# the flat unit allows there (1024 x 2^-24 = 6.1e-5), for a figure that is printed to one decimal.  So the flat unit was taken;
# measure_tolerances() reports the other figure as pp_per_length.
#
# K_FWD's largest ratios come from the shortest targets against the long models (4.49 at M = 1024, L = 2): there the score is the log of
# one row's sum over the entry distribution, and float32's occupancy recurrence and its sum over M nodes are what is being rounded.
K_FWD, K_OA, K_BIAS, K_N2, K_GAP, K_REG, K_PP = 32.0, 1024.0, 2.0, 128.0, 8.0, 1024.0, 1024.0
OBSERVED = dict(fwd=4.494, oa=133.9, bias=0.4448, n2=30.09, gap=1.901, reg=206.8, pp=176.9)      # the ratios measure_tolerances() gave when the constants were set
F32_CONSISTENT = 1e-3     # a float32 evaluation whose posteriors miss 1 by more than this left float32's range: it measures no rounding


def ulp32(x):
    return float(np.spacing(np.float32(abs(x)))) if math.isfinite(x) else 0.0


def score_tol(K, Ld, ref):
    return K * (Ld + 1) * EPS32 + 2.0 * ulp32(ref)


def score_ratio(got, ref, Ld):
    """How many (Ld + 1) 2^-24 the difference is, beyond the 2 ulp32 of the result's own rounding; inf when exactly one is -inf or either NaN."""
    got, ref = float(got), float(ref)
    if math.isnan(got) or math.isnan(ref):
        return np.inf
    if math.isinf(got) or math.isinf(ref):
        return 0.0 if got == ref else np.inf
    return max(0.0, abs(got - ref) - 2.0 * ulp32(ref)) / ((Ld + 1) * EPS32)


def pp_ratio(got, ref):
    """How many 2^-24 the posteriors along a path differ at most; inf for a NaN."""
    d = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(ref, dtype=np.float64))
    return float(d.max()) / EPS32 if np.isfinite(d).all() else np.inf


def n2_ratio(got, ref, Ld):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if not (np.isfinite(got).all() and np.isfinite(ref).all()):
        return np.inf
    return float(np.abs(got / ref - 1.0).max()) / ((Ld + 1) * EPS32)


# ---- the world ----------------------------------------------------------------------------------------------------------------------

def launch_classes():
    """[(Q, [model lengths])]: both edges of every Forward register class; the shortest class also takes M = 5 and 9."""
    out, prev = [], 0
    for q in KFB_Q:
        out.append((q, [1, 5, 9, 64] if prev == 0 else [prev + 1, 64 * q]))
        prev = 64 * q
    return out


TARGET_SEED = 83000
RESEED = {4096: 1, 1: 1, 9: 1, 65: 1, 129: 1}             # models whose targets take another seed, chosen so that the reference alone meets the undecided caps
GATED_M, GATED_NODE = 40, 20          # one more model of the first class: MD = 0 at this node, so the OA gates are exercised
WHOLE_NAMES = ("planted", "two", "fragment", "nb_planted", "nb_fragment", "r1", "r17", "star_mid", "deg_allx", "star_only")   # the targets aligned as a whole (ckm_align)


def class_of(M):
    return next(q for q in KFB_Q if 64 * q >= M)


def make_profile(M, gated=False):
    """A synthetic calibrated profile of M nodes with the stats line of tests/test_gpu_scan.py::test_register_class_boundaries."""
    rng = np.random.default_rng(61000 + M + (7 if gated else 0))
    p = synth.random_profile(rng, M, ("FBG%04d" if gated else "FB%04d") % M, "PF%05d.1" % (70000 + M + (5000 if gated else 0)))
    p.stats = (-8.5 - 0.002 * M, 0.71, -9.5 - 0.002 * M, 0.71, -3.8, 0.71)
    if gated:
        p.t[GATED_NODE, 0:3] = [1.0 - p.t[GATED_NODE, 1], p.t[GATED_NODE, 1], 0.0]
    return p


def planted_targets(p, rng):
    """(name, text) of the targets that carry whole domains: envelopes are defined on these."""
    dom = lambda: synth.sample_domain(rng, p)
    recs = [("planted", synth.to_text(np.concatenate([synth.random_residues(rng, 7), dom(), synth.random_residues(rng, 11)]))),
            ("two", synth.to_text(np.concatenate([synth.random_residues(rng, 9), dom(), synth.random_residues(rng, 5), dom(), synth.random_residues(rng, 8)])))]
    if p.M <= 128:
        d = dom()
        recs.append(("noise3100", synth.to_text(np.concatenate([synth.random_residues(rng, 1500), d, synth.random_residues(rng, 3100 - 1500 - len(d))]))))
    return recs


def own_targets(p):
    rng = np.random.default_rng(TARGET_SEED + p.M + 100000 * RESEED.get(p.M, 0))
    recs = [("r%d" % L, synth.to_text(synth.random_residues(rng, L))) for L in RANDOM_LENGTHS]
    recs += planted_targets(p, rng)
    w = max(1, p.M // 3)
    a = int(rng.integers(1, p.M - w + 2))
    recs.append(("fragment", synth.to_text(np.concatenate([synth.random_residues(rng, 6), synth.sample_domain(rng, p, a, a + w - 1), synth.random_residues(rng, 6)]))))
    consensus = synth.to_text(np.argmax(p.mat[1:] / synth.BGF, axis=1))
    half = synth.to_text(synth.random_residues(rng, 20))
    recs += [("consensus_x3", consensus * 3), ("deg_bjzoux", "BJZOUX" * 20), ("deg_allx", "X" * 30), ("star_mid", half + "*" + half[::-1]),
             ("star_only", "*")]                                     # (star_only: the one target whose Forward score is -inf)
    return recs


ENSEMBLE_SEED = TARGET_SEED + 500000                      # the ensemble targets' generator: ENSEMBLE_SEED + M (+ 7 gated) + 100000 ENSEMBLE_RESEED[M]
ENSEMBLE_RESEED = {}                                      # models whose ensemble target takes another seed, so that the oracle alone samples a trace of two segments in every class from 2 up


def ensemble_target(p, gated=False):
    """The text of a model's target for the trace ensemble: 6 random residues, three abutting pieces of the model -- its first 80 nodes, the
    80 around its middle, its last 80 -- and 6 random residues.  About 250 residues at every M, so the region matrix stays small at
    M = 4096, while both ends and the middle of the lane-striped row carry weight."""
    M = p.M
    rng = np.random.default_rng(ENSEMBLE_SEED + M + (7 if gated else 0) + 100000 * ENSEMBLE_RESEED.get(M, 0))
    pieces = [synth.random_residues(rng, 6), synth.sample_domain(rng, p, 1, min(M, 80)), synth.sample_domain(rng, p, max(1, M // 2 - 40), min(M, M // 2 + 40)),
              synth.sample_domain(rng, p, max(1, M - 79), M), synth.random_residues(rng, 6)]
    return synth.to_text(np.concatenate(pieces))


class Pair(object):
    __slots__ = ("M", "gated", "q", "name", "text", "dsq", "L", "fwd", "bias", "null", "nscale", "nscale_close", "regions", "tail", "btotal", "fwd32", "bias32", "occ_err")


class Envelope(object):
    """ref: envelope_c's dictionary in float64 (in WIDE where float64 itself left its range: wide); f32: the same evaluation in float32,
    in_range: whether that one hangs together; overflow, excused: backward_overflow and whether it is positive; undecided: the runner-up gap of the trace is below K_GAP's tolerance
    (the gap is the smallest over every choice of the walk: a decided envelope has a decided whole path, ref["path"] and ref["pp_path"]).
    An element of World.wholes that is no envelope of the world has no f32 (in_range is None), and ref is None where the target has no path."""
    __slots__ = ("M", "gated", "q", "name", "pair", "ienv", "jenv", "Ld", "ref", "wide", "f32", "in_range", "overflow", "excused", "undecided")


class World(object):
    """Every model of every class with its targets, envelopes and the reference's results (built once per process)."""
    _instance = None

    def __init__(self, threads=None):
        from tests import common
        threads = threads or max(1, min(16, os.cpu_count() or 1))
        self.lengths = sorted(set(m for _q, ms in launch_classes() for m in ms))
        self.keys = [(M, False) for M in self.lengths] + [(GATED_M, True)]          # a model is (length, gated)
        self.profs = [make_profile(M, g) for M, g in self.keys]
        self.path = common.hmm_file("fb_classes", self.profs)
        self.text = open(self.path).read()
        self.models = [Model(r) for r in parse_hmm(self.text)]
        self.index = dict((k, i) for i, k in enumerate(self.keys))
        self.recs = {}
        for key, p in zip(self.keys, self.profs):
            self.recs[key] = own_targets(p)
        for n, key in enumerate(self.keys):                                         # two targets of a neighbouring model
            other = self.keys[n - 1] if n else self.keys[1]
            self.recs[key] = self.recs[key] + [("nb_" + nm, tx) for nm, tx in self.recs[other] if nm in ("planted", "fragment")]
        jobs = [(key, nm, tx) for key in self.keys for nm, tx in self.recs[key]]
        order = dict(((key, nm), n) for n, (key, nm, _tx) in enumerate(jobs))
        with ThreadPoolExecutor(max_workers=threads) as ex:                         # (the C loop releases the interpreter lock)
            self.pairs = list(ex.map(self._pair, sorted(jobs, key=lambda j: -j[0][0] * len(j[2]))))
            self.pairs.sort(key=lambda pr: order[((pr.M, pr.gated), pr.name)])
            self.envs = [e for pr in self.pairs for e in self._envelopes_of(pr)]
            # ckm_align's reference: the unihit span (1, L) of every target of WHOLE_NAMES -- the world's own envelope where it has one
            have = dict((id(e.pair), e) for e in self.envs if (e.ienv, e.jenv) == (1, e.pair.L))
            self.wholes = [have.get(id(pr)) or self._span(pr, 1, pr.L) for pr in self.pairs if pr.name in WHOLE_NAMES]
            more = [e for e in self.wholes if id(e.pair) not in have]
            work = [(self._envelope, e) for e in self.envs] + [(self._whole, e) for e in more]
            list(ex.map(lambda fe: fe[0](fe[1]), sorted(work, key=lambda fe: -fe[1].M * fe[1].Ld)))

    def _pair(self, job):
        (M, gated), name, text = job
        model = self.models[self.index[(M, gated)]]
        c, c32 = model.cfg(), model.cfg(np.float32)
        pr = Pair()
        pr.M, pr.gated, pr.q, pr.name, pr.text, pr.dsq = M, gated, class_of(M), name, text, p7.digitize(text)
        L = pr.L = len(pr.dsq)
        pr.fwd, lxe = forward_c(c, specials(L, True), pr.dsq)
        pr.nscale, pr.nscale_close = expected_nscale(lxe)
        pr.bias, pr.null = bias_score(c, pr.dsq), float(null_score(L))
        pr.fwd32, pr.bias32 = float(np.float32(forward_c(c32, specials(L, True, np.float32), pr.dsq)[0])), float(np.float32(bias_score(c32, pr.dsq)))
        pr.regions, pr.tail, pr.btotal, pr.occ_err = [], np.inf, pr.fwd, 0.0
        if math.isfinite(pr.fwd):
            _f, pr.btotal, mocc, bt, et = occupancy_c(c, specials(L, True), pr.dsq)
            pr.regions, pr.tail = regions_of(mocc, bt, et)
            o32 = occupancy_c(c32, specials(L, True, np.float32), pr.dsq)[2:]          # what a threshold is compared with, in float32
            pr.occ_err = float(max([np.abs(a - b).max() for a, b in zip(o32, (mocc, bt, et))] +
                                   [np.abs(np.cumsum(a) - np.cumsum(b)).max() for a, b in zip(o32[1:], (bt, et))]))
        return pr

    @staticmethod
    def _envelopes_of(pr):
        """The envelopes of a planted target: the reference's own single-domain regions, (1, L), (5, L - 3), (i, i) and (i, i + 1)."""
        if pr.name not in ("planted", "two", "noise3100"):
            return []
        mid = pr.L // 2
        spans = sorted(set([(i, j) for i, j, multi, _m in pr.regions if not multi] + [(1, pr.L), (5, pr.L - 3), (mid, mid), (mid, mid + 1)]))
        return [World._span(pr, i, j) for i, j in spans]

    @staticmethod
    def _span(pr, i, j):
        e = Envelope()
        e.M, e.gated, e.q, e.name, e.pair, e.ienv, e.jenv, e.Ld = pr.M, pr.gated, pr.q, pr.name, pr, i, j, j - i + 1
        return e

    def _envelope(self, e, with_f32=True):
        _i, model = self.model_of(e)
        L, dsq = e.pair.L, e.pair.dsq[e.ienv - 1:e.jenv]
        e.ref = envelope_c(model.cfg(), specials(L, False), dsq)
        e.wide = not consistent(e.ref)
        if e.wide:
            e.ref = envelope_c(model.cfg(WIDE), specials(L, False, WIDE), dsq)
        e.f32 = envelope_c(model.cfg(np.float32), specials(L, False, np.float32), dsq) if with_f32 else None
        e.overflow = backward_overflow(e.ref["lxe"], e.ref["lbt"])
        e.excused = e.overflow > 0
        for r in (e.f32, e.ref):
            if r is not None:
                del r["ppX"], r["lxe"], r["lbt"]
        e.in_range = consistent(e.f32, F32_CONSISTENT) if with_f32 else None
        e.undecided = e.ref["gap"] < K_GAP * (e.Ld + 1) * EPS32

    def _whole(self, e):
        """The span (1, L) of a target that is aligned as a whole and is no envelope of the world: the float64 evaluation alone (nothing is
        measured on it), and nothing at all where no path exists (the Forward total is 0: ref is None)."""
        if math.isfinite(e.pair.fwd):
            self._envelope(e, with_f32=False)
        else:
            e.ref, e.wide, e.f32, e.overflow, e.excused, e.in_range, e.undecided = None, False, None, -np.inf, False, None, False

    @classmethod
    def get(cls):
        if cls._instance is None:
            cls._instance = World()
        return cls._instance

    def model_of(self, pr):
        """(index in the HMM file, Model) of a pair's or an envelope's model."""
        i = self.index[(pr.M, pr.gated)]
        return i, self.models[i]


def region_undecided(margin):
    return margin < K_REG * EPS32


def comparable_regions(pr):
    """The region list of a pair whose regions all fail rt3 and are decided (the comparisons after the last one too); else None."""
    if any(multi or region_undecided(margin) for _i, _j, multi, margin in pr.regions) or region_undecided(pr.tail):
        return None
    return [(i, j) for i, j, _multi, _margin in pr.regions]


def region_findings(pr, got, who):
    """The failures of one comparable pair's rows, got = [(env_from, env_to, ndom)], against the reference's regions."""
    tag = (who, pr.M, "gated" if pr.gated else pr.q, pr.name)
    want, bad = comparable_regions(pr), []
    if not all((i, j) in want for i, j, _n in got) or len(set(got)) != len(got):
        bad.append(tag + ("regions", [(i, j) for i, j, _n in got], want))
    if any(n != len(got) for _i, _j, n in got):
        bad.append(tag + ("ndom", [n for _i, _j, n in got], len(got)))
    return bad


def envelope_findings(e, rc_ok, envsc, oasc, null2, coords, who):
    """The failures of one envelope's figures (coords envelope-local) against the reference, as tuples that name it."""
    tag = (who, e.M, "gated" if e.gated else e.q, e.name, e.ienv, e.jenv)
    r = e.ref
    figures = [("envsc", envsc, r["envsc"], score_ratio(envsc, r["envsc"], e.Ld), K_FWD), ("oasc", oasc, r["oasc"], score_ratio(oasc, r["oasc"], e.Ld), K_OA),
               ("null2", list(null2), list(r["null2"]), n2_ratio(null2, r["null2"], e.Ld), K_N2)]
    bad = [tag + (f, got, ref, ratio) for f, got, ref, ratio, K in figures if not ratio <= K]
    if tuple(coords) != r["coords"] and not e.undecided:
        bad.append(tag + ("coords", tuple(coords), r["coords"], r["gap"]))
    if e.excused:                                    # float32 cannot hold its Backward: it must be refused
        return [tag + ("ok", 1, 0, e.overflow)] if rc_ok else []
    return bad if rc_ok else [tag + ("ok", 0, 1, e.overflow)]


def path_findings(e, rc_ok, path, pp, who):
    """(the failures of one envelope's alignment against the reference, the pp ratio or None where nothing was compared): path = int32[M],
    the envelope-local residue of match node k at k - 1, pp = float[Ld + 1].  Refused exactly where excused; where the envelope is decided,
    the path node for node, pp within K_PP 2^-24 and exactly 0 off ali_from..ali_to.  An undecided envelope's path is not compared."""
    tag = (who, e.M, "gated" if e.gated else e.q, e.name, e.ienv, e.jenv)
    if e.excused or not rc_ok:
        return ([] if e.excused != bool(rc_ok) else [tag + ("ok", int(bool(rc_ok)), int(not e.excused), e.overflow)]), None
    if e.undecided:
        return [], None
    r, bad = e.ref, []
    path, pp = np.asarray(path), np.asarray(pp, dtype=np.float64)
    differ = np.nonzero(path != r["path"][1:])[0]
    if len(differ):
        k = int(differ[0])
        bad.append(tag + ("path", "%d nodes differ, the first is node" % len(differ), k + 1, int(path[k]), int(r["path"][k + 1])))
    ratio = pp_ratio(pp, r["pp_path"])
    if not ratio <= K_PP:
        i = int(np.argmax(np.abs(pp - r["pp_path"])))
        bad.append(tag + ("pp", "residue", i, float(pp[i]), float(r["pp_path"][i]), ratio))
    outside = np.ones(e.Ld + 1, dtype=bool)
    outside[r["coords"][2]:r["coords"][3] + 1] = False
    if np.any(pp[outside] != 0):
        bad.append(tag + ("pp off the alignment", int(np.nonzero(outside & (pp != 0))[0][0])))
    return bad, ratio


def measure_tolerances(world):
    """The largest ratio of |float32 evaluation - float64 evaluation| to its unit, per quantity, over every pair and every envelope of the
    world that is not excused (backward_overflow): dict(fwd, oa, bias, n2, gap, reg, pp, pp_per_length, left_out).  fwd covers the whole-sequence
    Forward and envsc; gap is taken where both evaluations trace the same path (the host test asserts that they do wherever the envelope is
    decided); pp, in units of 2^-24, over the decided envelopes (the same path: the same cells are compared), pp_per_length the same figure
    in units of (Ld + 1) 2^-24 -- the unit that was not taken, see K_PP."""
    ins = [e for e in world.envs if not e.excused]
    return dict(fwd=max([score_ratio(pr.fwd32, pr.fwd, pr.L) for pr in world.pairs] + [score_ratio(np.float32(e.f32["envsc"]), e.ref["envsc"], e.Ld) for e in ins]),
                bias=max(score_ratio(pr.bias32, pr.bias, pr.L) for pr in world.pairs),
                oa=max(score_ratio(np.float32(e.f32["oasc"]), e.ref["oasc"], e.Ld) for e in ins),
                n2=max(n2_ratio(e.f32["null2"], e.ref["null2"], e.Ld) for e in ins),
                gap=max(abs(e.f32["gap"] - e.ref["gap"]) / ((e.Ld + 1) * EPS32) for e in ins if e.f32["coords"] == e.ref["coords"] and math.isfinite(e.ref["gap"])),
                reg=max(pr.occ_err for pr in world.pairs) / EPS32, left_out=[e for e in world.envs if e.excused],
                pp=max(pp_ratio(e.f32["pp_path"], e.ref["pp_path"]) for e in ins if e.in_range and not e.undecided),
                pp_per_length=max(pp_ratio(e.f32["pp_path"], e.ref["pp_path"]) / (e.Ld + 1) for e in ins if e.in_range and not e.undecided))


def k_of(ratio):
    """4 x the ratio, rounded up to a power of two."""
    return 2.0 ** math.ceil(math.log2(4.0 * ratio))
