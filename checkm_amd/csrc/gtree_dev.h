// gtree_dev.h -- the data layout, the arithmetic and the batch cuts of the genome tree (what scripts/genometreeworkflow/inferGenomeTree.py
// and bootstrapTree.py of the reference ask of FastTree: a tree over the rows of the concatenated alignment, and one per bootstrap
// replicate), written once for the kernels (kernels_gtree.hip), for the host executor of the CPU tests (run_host below,
// tests/emu/genometree_emu.cpp) and for the stand-alone check.  DESIGN section 27.
//
// Only +, -, *, / and comparisons on doubles, in the order written here: the library is built with -ffp-contract=off -fno-fast-math, the
// host executor with -ffp-contract=off, and neither calls libm: the logarithm is log_pos below.
//
// Alignment: N rows of L bytes, row i at text + i * L.  A byte is a residue when it is one of the twenty amino-acid letters in either
//   case (PplacerRunner's classes, PAML order); everything else is unknown.  The encoded alignment holds one byte per column,
//   0x80 | class for a residue and 0 for an unknown, in rows of Lp = L rounded up to 16 bytes, the padding unknown: eight columns of two
//   rows are then compared with a handful of 64-bit operations (pair_word).
// Trees of a call: the alignment itself (base = 1) and one per replicate, whose encoded alignment is column cols[r][c] of the alignment's
//   at column c (the resampled alignment the reference writes to disk); or, with `matrix` set, one per given matrix.
// Counts: compared[i][j] = columns where both rows hold a residue, differ[i][j] = those of them where the classes differ; [N][N], the
//   diagonal holding the residues of the row and 0.
// Distances: dist_of below; the diagonal is 0.
// Neighbour joining: the matrix D [N][N] stays symmetric.  `list` holds the active slots in ascending order, n of them.  A round with
//   n > 3 takes the pair of list positions (a, b), a < b, with the smallest Q = ((n - 2) * D[i][j] - R[i]) - R[j], ties to the smallest
//   (a, b) -- which is the smallest (i, j), the list being ascending; writes the merge row (i, j, li, lj); puts the new node into slot i;
//   takes j off the list.  R of the other slots is updated element-wise (update_r); R of the new row, and every R at the start, is
//   sum256 over the list.  The last three slots x < y < z close with the three-point formulas (close3): row N-3 joins x and y, row N-2
//   joins that node (slot x) and z, with z's length split in half: the written root sits on the last join.  N = 2 is one row.
// Merge rows: ij [N-1][2] uint32 slots, len [N-1][2] doubles.  A row's slots name the node last put there (a leaf, at first).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>
#include "ckm_internal.h"
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GT_HD __host__ __device__ __forceinline__
#else
#define GT_HD inline
#endif

namespace ckm {
namespace gtree {

constexpr uint32_t MAX_ROWS = 1u << 14;             // N: a matrix of 2 GB
constexpr uint32_t MAX_COLS = 1u << 20;             // L: the counts stay far inside 32 bits
constexpr uint32_t MAX_TREES = 1u << 16;
constexpr int SUM_LANES = 256;                      // lanes of sum256
constexpr int TILE = 64;                            // rows of a tile of the count kernel
constexpr int CHUNK = 128;                          // bytes of a row a tile holds in LDS at once
constexpr uint32_t NCLASS = 20;
enum { MODEL_KIMURA = 0, MODEL_POISSON = 1, MODEL_P = 2 };
using ckm::ARGS_INVALID;
using ckm::ARGS_OK;
using ckm::ARGS_RANGE;

// 0x80 | class of a residue, 0 of anything else
GT_HD uint8_t encode(uint8_t c) {
  const char *S = "ARNDCQEGHILKMFPSTWYV";
  const uint8_t u = (c >= (uint8_t)'a' && c <= (uint8_t)'z') ? (uint8_t)(c - 32) : c;
  for (uint32_t i = 0; i < NCLASS; ++i) if (u == (uint8_t)S[i]) return (uint8_t)(0x80u | i);
  return 0;
}
GT_HD uint32_t padded(uint32_t L) { return (L + 15u) & ~15u; }

// eight columns of two rows: bit 7 of a byte of `both` where both hold a residue, of `diff` where they also differ
GT_HD void pair_word(uint64_t a, uint64_t b, uint64_t &both, uint64_t &diff) {
  const uint64_t H = 0x8080808080808080ull, Lo = 0x7f7f7f7f7f7f7f7full;
  both = a & b & H;
  diff = (((a ^ b) & Lo) + Lo) & both;
}
GT_HD uint32_t pop64(uint64_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__popcll(x);
#else
  return (uint32_t)__builtin_popcountll(x);
#endif
}

GT_HD uint64_t bits_of(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint64_t)__double_as_longlong(x);
#else
  uint64_t u; memcpy(&u, &x, 8); return u;
#endif
}
GT_HD double double_of(uint64_t u) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __longlong_as_double((long long)u);
#else
  double x; memcpy(&x, &u, 8); return x;
#endif
}

// ln x of a positive, normal, finite x.  x = m * 2^e with m in [sqrt(1/2), sqrt(2)); s = (m - 1) / (m + 1), |s| < 0.1716;
// ln m = 2 s (1 + z/3 + z^2/5 + ... + z^11/23), z = s^2 (the first term left out is below 2^-62 of the sum), by Horner's rule;
// ln x = e * LN2_HI + (ln m + e * LN2_LO), LN2_HI holding the upper 32 bits of ln 2 so that e * LN2_HI is exact.
GT_HD double log_pos(double x) {
  uint64_t u = bits_of(x);
  int64_t e = (int64_t)((u >> 52) & 0x7ff) - 1023;
  u = (u & 0x000fffffffffffffull) | 0x3ff0000000000000ull;
  double m = double_of(u);                                   // [1, 2)
  if (m > 1.4142135623730951) { m = m * 0.5; e += 1; }
  const double f = m - 1.0;
  const double s = f / (2.0 + f);
  const double z = s * s;
  double p = 1.0 / 23.0;
  p = p * z + 1.0 / 21.0;
  p = p * z + 1.0 / 19.0;
  p = p * z + 1.0 / 17.0;
  p = p * z + 1.0 / 15.0;
  p = p * z + 1.0 / 13.0;
  p = p * z + 1.0 / 11.0;
  p = p * z + 1.0 / 9.0;
  p = p * z + 1.0 / 7.0;
  p = p * z + 1.0 / 5.0;
  p = p * z + 1.0 / 3.0;
  p = p * z + 1.0;
  const double lm = (2.0 * s) * p;
  const double de = (double)e;
  return de * 6.93147180369123816490e-01 + (lm + de * 1.90821492927058770002e-10);
}

// the argument of the logarithm (P: none); p = differ / compared
GT_HD double model_arg(double p, int model) {
  if (model == MODEL_KIMURA) return (1.0 - p) - 0.2 * (p * p);
  return 1.0 - p;
}
// A pair nothing was compared in, a non-positive argument and a value above max_dist give max_dist.
GT_HD double dist_of(uint32_t compared, uint32_t differ, int model, double max_dist) {
  if (compared == 0) return max_dist;
  const double p = (double)differ / (double)compared;
  double d = p;
  if (model != MODEL_P) {
    const double arg = model_arg(p, model);
    if (!(arg > 0.0)) return max_dist;
    d = arg >= 2.2250738585072014e-308 ? 0.0 - log_pos(arg) : max_dist;
  }
  return d > max_dist ? max_dist : d;
}

GT_HD double q_of(double nm2, double d, double ri, double rj) { return (nm2 * d - ri) - rj; }
// is (q1, k1) before (q2, k2): the smaller Q, then the smaller index
GT_HD bool before(double q1, uint32_t k1, double q2, uint32_t k2) { return q1 < q2 || (q1 == q2 && k1 < k2); }
// the lengths of a join of n > 2 active nodes: a negative one becomes 0 and its sibling takes the whole distance
GT_HD void join_lengths(double d, double ri, double rj, uint32_t n, double &li, double &lj) {
  li = d * 0.5 + (ri - rj) / (2.0 * (double)(n - 2));
  lj = d - li;
  if (li < 0.0) { li = 0.0; lj = d; }
  else if (lj < 0.0) { lj = 0.0; li = d; }
  if (lj < 0.0) lj = 0.0;                          // (a negative distance of a caller's matrix)
  if (li < 0.0) li = 0.0;
}
GT_HD double new_dist(double dik, double djk, double dij) { return ((dik + djk) - dij) * 0.5; }
GT_HD double update_r(double rk, double dik, double djk, double dn) { return ((rk - dik) - djk) + dn; }
GT_HD double clamp0(double x) { return x < 0.0 ? 0.0 : x; }
// the three-point formulas of x, y, z
GT_HD void close3(double dxy, double dxz, double dyz, double &lx, double &ly, double &lz) {
  lx = clamp0(((dxy + dxz) - dyz) * 0.5);
  ly = clamp0(((dxy + dyz) - dxz) * 0.5);
  lz = clamp0(((dxz + dyz) - dxy) * 0.5);
}

// THE summation order of every R: lane t of 256 adds the terms t, t + 256, ... to 0.0 in ascending order; then the lanes fold:
// for s = 128, 64, ..., 1 lane t < s takes lane t + s's sum onto its own.  The kernels do the fold in LDS.
template <class F> inline double sum256(uint32_t n, F term) {
  double lane[SUM_LANES];
  for (int t = 0; t < SUM_LANES; ++t) {
    double s = 0.0;
    for (uint32_t c = (uint32_t)t; c < n; c += SUM_LANES) s = s + term(c);
    lane[t] = s;
  }
  for (int s = SUM_LANES / 2; s >= 1; s >>= 1)
    for (int t = 0; t < s; ++t) lane[t] = lane[t] + lane[t + s];
  return lane[0];
}

// ---- host side, shared by the library, the host executor and the stand-alone check ---------------------------------------------------------
struct Args {
  uint32_t nrows, ncols; const uint8_t *text; uint64_t ntext_bytes;
  uint32_t nreps; const uint32_t *cols; uint32_t base; int32_t model; double max_dist;
  const double *matrix; uint32_t nmatrices;
};
struct Out { uint32_t *compared, *differ; double *dist; uint32_t *merge_ij; double *merge_len; };

inline bool finite(double x) { return x == x && x >= -1.7976931348623157e308 && x <= 1.7976931348623157e308; }
inline uint32_t trees_of(const Args &a) { return a.matrix ? a.nmatrices : a.base + a.nreps; }

// Why a call is refused.  Nothing is read before its size is known to be in range.
inline int check(const Args &a, std::string &why) {
  auto no = [&](int kind, const std::string &m) { why = m; return kind; };
  if (a.nrows > MAX_ROWS) return no(ARGS_RANGE, "more than " + std::to_string(MAX_ROWS) + " rows");
  if (a.nrows < 2) return no(ARGS_INVALID, "a tree needs at least two rows");
  if (a.matrix) {
    if (a.nmatrices > MAX_TREES) return no(ARGS_RANGE, "more than " + std::to_string(MAX_TREES) + " trees");
    const size_t n = (size_t)a.nmatrices * a.nrows * a.nrows;
    for (size_t k = 0; k < n; ++k) if (!finite(a.matrix[k])) return no(ARGS_INVALID, "a distance is not finite");
    return ARGS_OK;
  }
  if (a.ncols > MAX_COLS) return no(ARGS_RANGE, "more than " + std::to_string(MAX_COLS) + " columns");
  if (a.ncols < 1) return no(ARGS_INVALID, "no column");
  if (a.nreps > MAX_TREES - 1) return no(ARGS_RANGE, "more than " + std::to_string(MAX_TREES - 1) + " replicates");
  if (a.base > 1) return no(ARGS_INVALID, "base is 0 or 1");
  if (a.model != MODEL_KIMURA && a.model != MODEL_POISSON && a.model != MODEL_P) return no(ARGS_INVALID, "unknown distance model");
  if (!(a.max_dist > 0.0) || !finite(a.max_dist)) return no(ARGS_INVALID, "maxDist is not a positive finite number");
  if (!a.text || (a.nreps && !a.cols)) return no(ARGS_INVALID, "NULL argument");
  if (a.ntext_bytes != (uint64_t)a.nrows * a.ncols) return no(ARGS_INVALID, "the text does not hold rows x columns bytes");
  for (uint64_t k = 0; k < a.ntext_bytes; ++k) if (a.text[k] >= 0x80) return no(ARGS_RANGE, "the alignment holds a byte outside ASCII (row " + std::to_string(k / a.ncols) + ")");
  for (uint64_t k = 0; k < (uint64_t)a.nreps * a.ncols; ++k) if (a.cols[k] >= a.ncols) return no(ARGS_INVALID, "a drawn column is beyond the alignment");
  return ARGS_OK;
}

// bytes a tree needs on the device: its encoded alignment, the two counts, the matrix, and per slot R, two lists and the row minima
inline uint64_t tree_bytes(uint32_t N, uint32_t L) { return (uint64_t)N * padded(L) + (uint64_t)N * N * 16 + (uint64_t)N * 64; }
// trees of a batch under the budget: at least one
inline uint32_t batch_trees(uint32_t N, uint32_t L, uint64_t budget_bytes, uint32_t left) {
  const uint64_t t = budget_bytes / tree_bytes(N, L);
  return t < 1 ? 1u : t >= left ? left : (uint32_t)t;
}

// ---- the host executor: the kernels restated as loops over their threads, the same functions ----------------------------------------------
inline void host_encode(const uint8_t *text, uint32_t N, uint32_t L, std::vector<uint8_t> &enc) {
  const uint32_t Lp = padded(L);
  enc.assign((size_t)N * Lp, 0);
  for (uint32_t i = 0; i < N; ++i) for (uint32_t c = 0; c < L; ++c) enc[(size_t)i * Lp + c] = encode(text[(size_t)i * L + c]);
}
inline void host_gather(const std::vector<uint8_t> &enc, const uint32_t *cols, uint32_t N, uint32_t L, std::vector<uint8_t> &out) {
  const uint32_t Lp = padded(L);
  out.assign((size_t)N * Lp, 0);
  for (uint32_t i = 0; i < N; ++i) for (uint32_t c = 0; c < L; ++c) out[(size_t)i * Lp + c] = enc[(size_t)i * Lp + cols[c]];
}
inline void host_counts(const std::vector<uint8_t> &enc, uint32_t N, uint32_t L, uint32_t *cmp, uint32_t *dif) {
  const uint32_t Lp = padded(L);
  for (uint32_t i = 0; i < N; ++i)
    for (uint32_t j = 0; j < N; ++j) {
      uint32_t c = 0, d = 0;
      for (uint32_t k = 0; k < Lp; k += 8) {
        uint64_t a, b, both, diff;
        memcpy(&a, &enc[(size_t)i * Lp + k], 8); memcpy(&b, &enc[(size_t)j * Lp + k], 8);
        pair_word(a, b, both, diff);
        c += pop64(both); d += pop64(diff);
      }
      cmp[(size_t)i * N + j] = c; dif[(size_t)i * N + j] = d;
    }
}
inline void host_dist(const uint32_t *cmp, const uint32_t *dif, uint32_t N, int model, double max_dist, double *D) {
  for (uint32_t i = 0; i < N; ++i)
    for (uint32_t j = 0; j < N; ++j) D[(size_t)i * N + j] = i == j ? 0.0 : dist_of(cmp[(size_t)i * N + j], dif[(size_t)i * N + j], model, max_dist);
}
// D [N][N] is used up
inline void host_join(double *D, uint32_t N, uint32_t *ij, double *len) {
  std::vector<uint32_t> list(N), next(N);
  std::vector<double> R(N);
  for (uint32_t i = 0; i < N; ++i) list[i] = i;
  for (uint32_t i = 0; i < N; ++i) R[i] = sum256(N, [&](uint32_t c) { return c == i ? 0.0 : D[(size_t)i * N + c]; });
  uint32_t n = N, row = 0;
  for (; n > 3; --n, ++row) {
    // gt_rowmin: the best partner of every list position; gt_join: the best position
    double bq = 0.0; uint32_t ba = 0, bb = 0; bool have = false;
    for (uint32_t a = 0; a + 1 < n; ++a) {
      const uint32_t i = list[a];
      double rq = 0.0; uint32_t rb = 0; bool rh = false;
      for (uint32_t b = a + 1; b < n; ++b) {
        const uint32_t k = list[b];
        const double q = q_of((double)(n - 2), D[(size_t)i * N + k], R[i], R[k]);
        if (!rh || before(q, b, rq, rb)) { rq = q; rb = b; rh = true; }
      }
      if (!have || before(rq, a, bq, ba)) { bq = rq; ba = a; bb = rb; have = true; }
    }
    const uint32_t i = list[ba], j = list[bb];
    const double dij = D[(size_t)i * N + j];
    join_lengths(dij, R[i], R[j], n, len[(size_t)row * 2], len[(size_t)row * 2 + 1]);
    ij[(size_t)row * 2] = i; ij[(size_t)row * 2 + 1] = j;
    for (uint32_t c = 0; c + 1 < n; ++c) next[c] = list[c + (c >= bb ? 1u : 0u)];
    std::vector<double> term(n - 1, 0.0);
    for (uint32_t c = 0; c + 1 < n; ++c) {
      const uint32_t k = next[c];
      if (k == i) continue;
      const double dik = D[(size_t)i * N + k], djk = D[(size_t)j * N + k], dn = new_dist(dik, djk, dij);
      R[k] = update_r(R[k], dik, djk, dn);
      D[(size_t)i * N + k] = dn; D[(size_t)k * N + i] = dn;
      term[c] = dn;
    }
    R[i] = sum256(n - 1, [&](uint32_t c) { return term[c]; });
    list.swap(next);
  }
  if (n == 3) {
    const uint32_t x = list[0], y = list[1], z = list[2];
    double lx, ly, lz;
    close3(D[(size_t)x * N + y], D[(size_t)x * N + z], D[(size_t)y * N + z], lx, ly, lz);
    ij[(size_t)row * 2] = x; ij[(size_t)row * 2 + 1] = y; len[(size_t)row * 2] = lx; len[(size_t)row * 2 + 1] = ly; ++row;
    ij[(size_t)row * 2] = x; ij[(size_t)row * 2 + 1] = z; len[(size_t)row * 2] = lz * 0.5; len[(size_t)row * 2 + 1] = lz * 0.5;
  } else {
    const uint32_t x = list[0], y = list[1];
    const double h = clamp0(D[(size_t)x * N + y]) * 0.5;
    ij[0] = x; ij[1] = y; len[0] = h; len[1] = h;
  }
}

// info[0] = batches, info[1] = trees
inline int run_host(const Args &a, uint64_t budget_bytes, const Out &o, uint64_t *info, std::string &why) {
  const int kind = check(a, why);
  if (kind) return kind;
  const uint32_t N = a.nrows, L = a.matrix ? 0 : a.ncols, T = trees_of(a);
  if (info) { info[0] = 0; info[1] = T; }
  std::vector<uint8_t> enc, rep;
  std::vector<uint32_t> cmp, dif;
  std::vector<double> D((size_t)N * N);
  if (!a.matrix) {
    host_encode(a.text, N, L, enc);
    cmp.resize((size_t)N * N); dif.resize((size_t)N * N);
    if (o.compared || o.dist) {
      host_counts(enc, N, L, cmp.data(), dif.data());
      if (o.compared) { memcpy(o.compared, cmp.data(), cmp.size() * 4); memcpy(o.differ, dif.data(), dif.size() * 4); }
      if (o.dist) host_dist(cmp.data(), dif.data(), N, a.model, a.max_dist, o.dist);
    }
  }
  if (!o.merge_ij) return ARGS_OK;
  for (uint32_t t0 = 0; t0 < T;) {
    const uint32_t nt = batch_trees(N, L, budget_bytes, T - t0);
    for (uint32_t t = t0; t < t0 + nt; ++t) {
      if (a.matrix) memcpy(D.data(), a.matrix + (size_t)t * N * N, (size_t)N * N * 8);
      else {
        const bool is_base = a.base && t == 0;
        if (!is_base) host_gather(enc, a.cols + (size_t)(t - a.base) * L, N, L, rep);
        host_counts(is_base ? enc : rep, N, L, cmp.data(), dif.data());
        host_dist(cmp.data(), dif.data(), N, a.model, a.max_dist, D.data());
      }
      host_join(D.data(), N, o.merge_ij + (size_t)t * (N - 1) * 2, o.merge_len + (size_t)t * (N - 1) * 2);
    }
    if (info) info[0] += 1;
    t0 += nt;
  }
  return ARGS_OK;
}

}  // namespace gtree
}  // namespace ckm
