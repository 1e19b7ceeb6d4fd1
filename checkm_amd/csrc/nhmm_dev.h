// nhmm_dev.h -- the nucleotide model scan of SSU_Finder, defined once: the score system, the cell, the recurrence, the tile
// geometry, the check of a call, the layout of the device image, the host executor, the compaction order and the hit rule.  Included by
// kernels_nhmm.hip / ckm_nhmm.hip (hipcc), nhmm_host.cpp and the CPU tests (g++).
//
// Scores are int32 milli-bits.  A cell is a pair (score, start), start being the 1-based position of the strand where the path entered
// the model, packed into one int64 as (score << 32) | ~start: a signed 64-bit max then is best(a, b) = the higher score, at equal
// scores the smaller start.  That is a total order, max over it is associative and commutative, and adding a transition to the score
// is monotone in it, so every reduction or scan order of the recurrence below gives the same pair.
//
//   M(i,k) = e(k, x_i) + best( (tBM, i), M(i-1,k-1) + tMM(k), I(i-1,k-1) + tIM(k), D(i-1,k-1) + tDM(k) )
//   I(i,k) = best( M(i-1,k) + tMI(k), I(i-1,k) + tII(k) )
//   D(i,k) = best( M(i,k-1) + tMD(k), D(i,k-1) + tDD(k) )
//   row(i) = best_k M(i,k)                                                            k = 1 .. M, unihit local, exit from a match costs 0
//
// Tables of a model, node k at index k - 1: emis[4][M] (A C G T/U; every other byte emits 0) and trans[7][M] in the order
// MM IM DM (into k: node k - 1's numbers of the file, FLOOR at k = 1) MI II (node k's own) MD DD (into k, FLOOR at k = 1).
// tBM = lround(1000 log2(2 / (M (M + 1)))).
//
// No underflow, by bounds the check enforces instead of a floor per cell: FLOOR <= every entry, transitions <= 0, emissions <= EMAX,
// stride + overlap <= 2^17, M <= 2048.  A cell that exists (i >= 1, k >= 1, reached from an entry) then lies in
// [2 FLOOR + tBM, 2^28]: M(i,k) >= FLOOR + tBM, I and D take one transition from a match.  Cells outside the matrix are NEG = -2^29
// and take at most one row of transitions before an entry beats them; the device's padding nodes emit PADE = -2^29 for every byte and
// stay below -2^28.  So every sum fits int32, every row is exact (not only those >= -2^20), and "'*' = FLOOR" is part of the definition.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>
#include "ckm_internal.h"
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define NH_HD __host__ __device__ __forceinline__
#else
#define NH_HD inline
#endif

namespace ckm {
namespace nhmm {

constexpr uint32_t MAX_M = 2048;                    // the cap on model nodes: 32 nodes per lane of one wavefront
constexpr int32_t FLOOR = -(1 << 21);               // what '*' becomes; the lower bound of every table entry
constexpr int32_t EMAX = 2048;                      // upper bound of an emission (log2(1 / 0.25) = 2 bits)
constexpr int32_t NEG = -(1 << 29);                 // score of a cell outside the matrix
constexpr int32_t PADE = -(1 << 29);                // emission of a padding node of the device image
constexpr int32_t TSAT = -(1 << 30);                // sums of tDD over a run of nodes saturate here (kernels_nhmm.hip): below every live d + T
constexpr int32_t MIN_THRESHOLD = -(1 << 20);       // no reporting threshold below this
constexpr uint32_t MAX_SPAN = 1u << 17;             // stride + overlap
constexpr int NT = 7, NE = 4, NIMG = 12;            // transition rows, emission rows, rows of the device image (5 emission + 7 transition)
enum { T_MM = 0, T_IM = 1, T_DM = 2, T_MI = 3, T_II = 4, T_MD = 5, T_DD = 6 };
using ckm::ARGS_INVALID;
using ckm::ARGS_OK;
using ckm::ARGS_RANGE;

typedef long long cell;
NH_HD cell mk(int32_t score, uint32_t start) { return (cell)(((unsigned long long)(uint32_t)score << 32) | (uint32_t)~start); }
NH_HD int32_t score_of(cell c) { return (int32_t)(c >> 32); }
NH_HD uint32_t start_of(cell c) { return ~(uint32_t)(unsigned long long)c; }
NH_HD cell add(cell c, int32_t t) { return mk(score_of(c) + t, start_of(c)); }
NH_HD cell best(cell a, cell b) { return a > b ? a : b; }
NH_HD cell neg_cell() { return mk(NEG, 0xffffffffu); }

// A C G T/U either case -> 0..3, every other byte 4; the complement of a code
NH_HD int code_of(uint8_t c) {
  switch (c | 0x20) { case 'a': return 0; case 'c': return 1; case 'g': return 2; case 't': case 'u': return 3; default: return 4; }
}
NH_HD int comp_of(int code) { return code < 4 ? 3 - code : 4; }

inline int32_t tbm_of(uint32_t M) { return (int32_t)std::lround(1000.0 * std::log2(2.0 / ((double)M * ((double)M + 1.0)))); }
inline int q_of(uint32_t M) { for (int q : {1, 2, 4, 8, 16, 24, 32}) if ((uint32_t)q * 64 >= M) return q; return 0; }

struct Args {
  uint32_t nmodels; const uint32_t *M; const uint64_t *tab_off; const int32_t *emis, *trans; uint64_t ntab; const int32_t *min_score;
  uint32_t stride, overlap, strands;
  const int32_t *e(uint32_t m) const { return emis + NE * tab_off[m]; }
  const int32_t *t(uint32_t m) const { return trans + NT * tab_off[m]; }
};
struct Seqs { const char *text; const uint64_t *off, *bytes; uint32_t nseq; };

// one tile: rows first .. last of a strand are computed, own .. last reported at out_off of the batch's row buffer
struct Tile { uint32_t model, seq, strand, first, own, last; uint64_t out_off; };
struct TileDev { uint64_t text_off, out_off; uint32_t L, first, own, last, strand, model; int32_t thr; uint32_t pad; };

struct Rows { std::vector<uint32_t> model, seq, strand, pos, start; std::vector<int32_t> score; size_t size() const { return pos.size(); } };
struct Hits { std::vector<uint32_t> model, seq, strand, from, to; std::vector<int32_t> score; size_t size() const { return from.size(); } };
struct Info { uint64_t tiles = 0, launches = 0, cells = 0, batches = 0; };

inline int check(const Args &a, std::string &why) {
  if (!a.nmodels) return ARGS_OK;
  if (!a.M || !a.tab_off || !a.emis || !a.trans || !a.min_score) { why = "NULL argument"; return ARGS_INVALID; }
  if (a.strands < 1 || a.strands > 3) { why = "strands is 1 (forward), 2 (reverse) or 3 (both)"; return ARGS_INVALID; }
  if (!a.stride) { why = "a stride of 0"; return ARGS_INVALID; }
  if (a.stride > MAX_SPAN || a.overlap > MAX_SPAN || a.stride + a.overlap > MAX_SPAN) { why = "stride + overlap beyond 2^17 rows"; return ARGS_RANGE; }
  if (a.tab_off[0]) { why = "tab_off does not start at 0"; return ARGS_INVALID; }
  for (uint32_t m = 0; m < a.nmodels; ++m) {
    if (!a.M[m]) { why = "model " + std::to_string(m) + " has no nodes"; return ARGS_INVALID; }
    if (a.M[m] > MAX_M) { why = "model " + std::to_string(m) + " has " + std::to_string(a.M[m]) + " nodes, the scan holds 2048"; return ARGS_RANGE; }
    if (a.tab_off[m + 1] < a.tab_off[m] || a.tab_off[m + 1] - a.tab_off[m] != a.M[m]) { why = "tab_off does not step by the nodes of model " + std::to_string(m); return ARGS_INVALID; }
    if (a.min_score[m] < MIN_THRESHOLD) { why = "a reporting threshold below -2^20"; return ARGS_RANGE; }
  }
  if (a.tab_off[a.nmodels] != a.ntab) { why = "ntab is not the sum of the nodes"; return ARGS_INVALID; }
  for (uint64_t k = 0; k < NE * a.ntab; ++k)
    if (a.emis[k] < FLOOR || a.emis[k] > EMAX) { why = "an emission outside [-2^21, 2048]"; return ARGS_RANGE; }
  for (uint64_t k = 0; k < NT * a.ntab; ++k)
    if (a.trans[k] < FLOOR || a.trans[k] > 0) { why = "a transition outside [-2^21, 0]"; return ARGS_RANGE; }
  return ARGS_OK;
}

// the first sequence with a byte beyond ASCII or with 2^31 - 1 bytes or more, or -1
inline int64_t first_refused_seq(const Seqs &s, bool &too_long) {
  too_long = false;
  for (uint32_t q = 0; q < s.nseq; ++q) {
    if (s.bytes[q] >= 0x7fffffffull) { too_long = true; return q; }
    const uint8_t *p = (const uint8_t *)s.text + s.off[q];
    for (uint64_t k = 0; k < s.bytes[q]; ++k) if (p[k] & 0x80) return q;
  }
  return -1;
}

// every tile of a call in (model, sequence, strand, tile) order; out_off is set by cut_batch
inline std::vector<Tile> make_tiles(const Args &a, const Seqs &s) {
  std::vector<Tile> v;
  for (uint32_t m = 0; m < a.nmodels; ++m)
    for (uint32_t q = 0; q < s.nseq; ++q)
      for (uint32_t st = 0; st < 2; ++st) {
        if (!(a.strands & (1u << st))) continue;
        const uint32_t L = (uint32_t)s.bytes[q];
        for (uint64_t own = 1; own <= L; own += a.stride) {
          const uint32_t first = own > a.overlap ? (uint32_t)(own - a.overlap) : 1u;
          v.push_back(Tile{m, q, st, first, (uint32_t)own, (uint32_t)std::min<uint64_t>(L, own + a.stride - 1), 0});
        }
      }
  return v;
}

// the tiles [from, to) of one batch: as many as keep the row buffer (8 bytes per reported row) inside the budget, one at least
inline size_t cut_batch(std::vector<Tile> &t, size_t from, uint64_t budget_bytes, uint64_t &rows) {
  rows = 0;
  size_t to = from;
  while (to < t.size()) {
    const uint64_t n = t[to].last - t[to].own + 1;
    if (to > from && (rows + n) * 8 > budget_bytes) break;
    t[to].out_off = rows; rows += n; ++to;
  }
  return to;
}

// ---- the device image of a model: 12 rows (emissions of codes 0..4, then the 7 transitions) of Q * 64 nodes, lane z owning the nodes
// z Q + 1 .. z Q + Q, stored [row][j][lane] so that the 64 lanes of a wavefront read consecutive LDS words
inline std::vector<int32_t> device_image(const Args &a, uint32_t m, int Q) {
  const uint32_t M = a.M[m];
  std::vector<int32_t> img((size_t)NIMG * Q * 64);
  for (int r = 0; r < NIMG; ++r)
    for (int lane = 0; lane < 64; ++lane)
      for (int j = 0; j < Q; ++j) {
        const uint32_t k0 = (uint32_t)lane * Q + j;      // node k0 + 1
        int32_t v;
        if (k0 >= M) v = r < 5 ? PADE : FLOOR;
        else if (r < 4) v = a.e(m)[(size_t)r * M + k0];
        else if (r == 4) v = 0;
        else v = a.t(m)[(size_t)(r - 5) * M + k0];
        img[((size_t)r * Q + j) * 64 + lane] = v;
      }
  return img;
}

// ---- the host executor: the recurrence as written above, row by row; out[i - own] = row(i) for the owned rows
inline void tile_host(const Args &a, const Seqs &s, const Tile &t, cell *out) {
  const uint32_t M = a.M[t.model], L = (uint32_t)s.bytes[t.seq];
  const int32_t *e = a.e(t.model), *tr = a.t(t.model), tBM = tbm_of(M);
  const uint8_t *x = (const uint8_t *)s.text + s.off[t.seq];
  std::vector<cell> pM(M + 1, neg_cell()), pI(M + 1, neg_cell()), pD(M + 1, neg_cell()), cM(M + 1), cI(M + 1), cD(M + 1);
  for (uint32_t i = t.first; i <= t.last; ++i) {
    const int code = t.strand ? comp_of(code_of(x[L - i])) : code_of(x[i - 1]);
    cM[0] = cI[0] = cD[0] = neg_cell();
    cell row = neg_cell();
    for (uint32_t k = 1; k <= M; ++k) {
      const size_t z = k - 1;
      const cell in = best(best(mk(tBM, i), add(pM[k - 1], tr[T_MM * M + z])), best(add(pI[k - 1], tr[T_IM * M + z]), add(pD[k - 1], tr[T_DM * M + z])));
      cM[k] = add(in, code < 4 ? e[(size_t)code * M + z] : 0);
      cI[k] = best(add(pM[k], tr[T_MI * M + z]), add(pI[k], tr[T_II * M + z]));
      cD[k] = best(add(cM[k - 1], tr[T_MD * M + z]), add(cD[k - 1], tr[T_DD * M + z]));
      row = best(row, cM[k]);
    }
    if (i >= t.own) out[i - t.own] = row;
    pM.swap(cM); pI.swap(cI); pD.swap(cD);
  }
}

// the reported rows of a batch's row buffer, in tile order (what the count / scan / fill kernels produce)
inline void compact_host(const Args &a, const std::vector<Tile> &t, size_t from, size_t to, const cell *buf, Rows &r) {
  for (size_t k = from; k < to; ++k)
    for (uint32_t i = t[k].own; i <= t[k].last; ++i) {
      const cell c = buf[t[k].out_off + (i - t[k].own)];
      if (score_of(c) < a.min_score[t[k].model]) continue;
      r.model.push_back(t[k].model); r.seq.push_back(t[k].seq); r.strand.push_back(t[k].strand); r.pos.push_back(i); r.start.push_back(start_of(c)); r.score.push_back(score_of(c));
    }
}

// ---- hits: per (model, sequence, strand) the reported rows are grouped by start; a group's candidate is its highest score, at ties
// the smallest row; candidates by score descending, then start ascending, accepted greedily when their closed interval [start, row]
// meets no accepted one.  Coordinates go out on the forward strand: from <= to.
inline void hits_host(const Seqs &s, const Rows &r, Hits &h) {
  struct Cand { uint32_t start, row; int32_t score; };
  for (size_t a = 0, z; a < r.size(); a = z) {
    for (z = a; z < r.size() && r.model[z] == r.model[a] && r.seq[z] == r.seq[a] && r.strand[z] == r.strand[a];) ++z;
    std::vector<Cand> c;
    for (size_t k = a; k < z; ++k) c.push_back(Cand{r.start[k], r.pos[k], r.score[k]});
    std::sort(c.begin(), c.end(), [](const Cand &p, const Cand &q) { return p.start != q.start ? p.start < q.start : p.score != q.score ? p.score > q.score : p.row < q.row; });
    size_t n = 0;
    for (size_t k = 0; k < c.size(); ++k) if (!k || c[k].start != c[k - 1].start) c[n++] = c[k];
    c.resize(n);
    std::sort(c.begin(), c.end(), [](const Cand &p, const Cand &q) { return p.score != q.score ? p.score > q.score : p.start < q.start; });
    std::vector<Cand> kept;
    for (const Cand &x : c) {
      bool free_ = true;
      for (const Cand &y : kept) if (x.start <= y.row && y.start <= x.row) { free_ = false; break; }
      if (!free_) continue;
      kept.push_back(x);
      const uint32_t L = (uint32_t)s.bytes[r.seq[a]], st = r.strand[a];
      h.model.push_back(r.model[a]); h.seq.push_back(r.seq[a]); h.strand.push_back(st); h.score.push_back(x.score);
      h.from.push_back(st ? L + 1 - x.row : x.start); h.to.push_back(st ? L + 1 - x.start : x.row);
    }
  }
}

inline uint64_t tile_cells(const Args &a, const Tile &t) { return (uint64_t)(t.last - t.first + 1) * a.M[t.model]; }

// the whole call on the host; refused_seq: the sequence a refusal names, or -1
inline int run_host(const Args &a, const Seqs &s, uint64_t budget_bytes, Rows &rows, Hits &hits, Info &info, int64_t &refused_seq, std::string &why) {
  refused_seq = -1;
  const int kind = check(a, why);
  if (kind) return kind;
  bool too_long = false;
  refused_seq = first_refused_seq(s, too_long);
  if (refused_seq >= 0) { why = too_long ? "a sequence of 2^31 - 1 bytes or more" : "a sequence holds a byte beyond ASCII"; return too_long ? ARGS_RANGE : ARGS_INVALID; }
  std::vector<Tile> tiles = make_tiles(a, s);
  info.tiles = tiles.size();
  std::vector<cell> buf;
  for (size_t from = 0, to; from < tiles.size(); from = to) {
    uint64_t nrows = 0;
    to = cut_batch(tiles, from, budget_bytes, nrows);
    buf.assign(nrows, mk(0x5a5a5a5a, 0x5a5a5a5a));
    for (size_t k = from; k < to; ++k) {
      tile_host(a, s, tiles[k], buf.data() + tiles[k].out_off);
      info.cells += tile_cells(a, tiles[k]);
      if (k == from || tiles[k].model != tiles[k - 1].model) ++info.launches;
    }
    compact_host(a, tiles, from, to, buf.data(), rows);
    ++info.batches;
  }
  hits_host(s, rows, hits);
  return ARGS_OK;
}

}  // namespace nhmm
}  // namespace ckm

// what ckm_nhmm_run hands back (include/checkm_hip.h keeps it opaque)
struct ckm_nhmm_result { ckm::nhmm::Rows rows; ckm::nhmm::Hits hits; };
