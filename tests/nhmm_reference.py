"""TEST INFRASTRUCTURE: an independent reference of the nucleotide model scan of SSU_Finder (the recurrence in the header comment of
checkm_amd/csrc/nhmm_dev.h), in numpy and plain Python.  It shares nothing with the library, the executor or tests/emu:

  - scores are int64 and never saturate (FLOOR x 2048 is about -2^32); a cell outside the matrix is a score of -2^42, far below every
    sum of table entries, where the header has NEG = -2^29 -- the header's bounds say no live cell can tell the two apart;
  - a cell is the key score * 2^18 + (2^18 - 1 - start): higher score first, at equal score the smaller start.  Adding t * 2^18 adds t
    to the score and keeps the order, so max over keys is best() of the header.  start < 2^18 is asserted;
  - the M and I rows are one vector operation over k; the D row is the closed form
        D(k) = S(k) + max_{1 <= j < k} (M(j) + tMD(j + 1) - S(j + 1)),      S the prefix sum of tDD,
    a running maximum instead of a chain (the path M(j) -> D(j + 1) -> ... -> D(k) costs tMD(j + 1) + S(k) - S(j + 1));
  - tBM, the tiles, the compaction order and the hit rule are restated here from the header's comments.

rows() is one tile; scan() is a whole call and returns the columns of _lib.nhmm_run plus, per reported row, whether two cells M(i, k)
reach the row's maximum with different starts (row_tie)."""
import math

import numpy as np

FLOOR = -(1 << 21)
SHIFT = 18
LOWMASK = (1 << SHIFT) - 1
OUTSIDE = -(1 << 42) << SHIFT          # the key of a cell outside the matrix
ROW_F = ("row_model", "row_seq", "row_strand", "row_pos", "row_start", "row_score")
HIT_F = ("hit_model", "hit_seq", "hit_strand", "hit_from", "hit_to", "hit_score")
_CODE = {"a": 0, "c": 1, "g": 2, "t": 3, "u": 3}


def tbm(M):
    """round(1000 log2(2 / (M (M + 1)))), halves away from zero."""
    x = 1000.0 * math.log2(2.0 / (float(M) * (float(M) + 1.0)))
    return int(math.floor(abs(x) + 0.5)) * (1 if x >= 0 else -1)


def codes(text, strand):
    """The residues x_1 .. x_L of a strand as 0..3 (A C G T/U, either case) or 4; strand 1 is the reverse complement."""
    if isinstance(text, bytes):
        text = text.decode("ascii")
    c = [_CODE.get(ch.lower(), 4) for ch in text]
    return [3 - v if v < 4 else 4 for v in reversed(c)] if strand else c


def rows(emis, trans, text, strand, first, own, last, ties=False):
    """Rows first .. last of one strand are computed from an empty matrix before `first`; returns (pos, start, score) of the rows
    own .. last as int64 arrays, and with ties=True a fourth bool array: two cells M(i, k) hold the row's best score with different starts."""
    e = np.asarray(emis, dtype=np.int64) << SHIFT
    t = np.asarray(trans, dtype=np.int64) << SHIFT
    M = e.shape[1]
    assert e.shape == (4, M) and t.shape == (7, M) and 1 <= first <= own <= last < (1 << SHIFT)
    tMM, tIM, tDM, tMI, tII, tMD, tDD = t
    S = np.cumsum(tDD)                                              # S[k - 1] = S(k)
    lift = tMD[1:] - S[1:]                                          # index j - 1: tMD(j + 1) - S(j + 1), j = 1 .. M - 1
    x = codes(text, strand)
    entry_score = tbm(M) << SHIFT
    pM, pI, pD = (np.full(M + 1, OUTSIDE, dtype=np.int64) for _ in range(3))          # index k, 0 = outside
    pos, start, score, tie = [], [], [], []
    for i in range(first, last + 1):
        entry = entry_score + (LOWMASK - i)
        cM, cI, cD = (np.full(M + 1, OUTSIDE, dtype=np.int64) for _ in range(3))
        into = np.maximum(np.maximum(pM[:-1] + tMM, pI[:-1] + tIM), np.maximum(pD[:-1] + tDM, entry))
        cM[1:] = into + e[x[i - 1]] if x[i - 1] < 4 else into
        cI[1:] = np.maximum(pM[1:] + tMI, pI[1:] + tII)
        if M > 1:
            cD[2:] = S[1:] + np.maximum.accumulate(cM[1:-1] + lift)
        if i >= own:
            best = int(cM[1:].max())
            pos.append(i)
            start.append(LOWMASK - (best & LOWMASK))
            score.append(best >> SHIFT)
            top = cM[1:][(cM[1:] >> SHIFT) == (best >> SHIFT)]
            tie.append(bool((top != best).any()))
        pM, pI, pD = cM, cI, cD
    out = (np.array(pos, dtype=np.int64), np.array(start, dtype=np.int64), np.array(score, dtype=np.int64))
    return out + (np.array(tie, dtype=bool),) if ties else out


def tiles_of(L, stride, overlap):
    """(first, own, last) of every tile of a strand of L rows: a tile owns `stride` rows and starts `overlap` rows before them."""
    return [(own - overlap if own > overlap else 1, own, min(L, own + stride - 1)) for own in range(1, L + 1, stride)]


def hits_of(reported, L, strand):
    """The hit rule on the reported rows [(start, row, score)] of one (model, sequence, strand): one candidate per start, its highest
    score and at equal scores its smallest row; candidates by score descending, then start ascending; one is accepted when its closed
    interval [start, row] meets no accepted one.  Returns [(from, to, score)] on the forward strand, in the order of acceptance."""
    cand = {}
    for s, r, sc in reported:
        if s not in cand or (sc, -r) > (cand[s][1], -cand[s][0]):
            cand[s] = (r, sc)
    kept, out = [], []
    for s, (r, sc) in sorted(cand.items(), key=lambda kv: (-kv[1][1], kv[0])):
        if any(s <= r2 and s2 <= r for s2, r2 in kept):
            continue
        kept.append((s, r))
        out.append((L + 1 - r, L + 1 - s, sc) if strand else (s, r, sc))
    return out


def scan(models, thresholds, stride, overlap, strands, seqs):
    """A whole call.  models: [(emis [4, M], trans [7, M])]; thresholds: one per model; strands: 1 forward, 2 reverse, 3 both; seqs: a
    list of str.  Returns a dict: the ROW_F columns in (model, sequence, strand, tile, row) order for the rows at or above the model's
    threshold, row_tie for the same rows, the HIT_F columns, and the number of tiles."""
    row = {f: [] for f in ROW_F + ("row_tie",)}
    hit = {f: [] for f in HIT_F}
    ntiles = 0
    for m, (e, t) in enumerate(models):
        for q, text in enumerate(seqs):
            for st in (0, 1):
                if not strands & (1 << st):
                    continue
                reported = []
                for first, own, last in tiles_of(len(text), stride, overlap):
                    ntiles += 1
                    for i, s, sc, tie in zip(*rows(e, t, text, st, first, own, last, ties=True)):
                        if sc < thresholds[m]:
                            continue
                        reported.append((int(s), int(i), int(sc)))
                        for f, v in zip(ROW_F + ("row_tie",), (m, q, st, i, s, sc, tie)):
                            row[f].append(v)
                for a, b, sc in hits_of(reported, len(text), st):
                    for f, v in zip(HIT_F, (m, q, st, a, b, sc)):
                        hit[f].append(v)
    out = {f: np.array(v, dtype=bool if f == "row_tie" else np.int64) for f, v in row.items()}
    out.update({f: np.array(v, dtype=np.int64) for f, v in hit.items()})
    out["tiles"] = ntiles
    return out
