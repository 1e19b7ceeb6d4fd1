// place_dev.h -- the data layout, the arithmetic and the chunk cuts of the phylogenetic placement (what checkm/pplacer.py asks of pplacer:
// the edge of the reference tree every bin attaches to), written once for the kernels (kernels_place.hip), for the host executor of
// the CPU tests (run_host below, tests/emu/placement_emu.cpp) and for the stand-alone check.  DESIGN section 23.
//
// Only +, *, /, comparisons and exact scaling (frexp / ldexp) on doubles: no exp and no log.  Every exp(lambda_k * rate * t) arrives in a
// table the caller made.  The library is built with -ffp-contract=off -fno-fast-math, the host executor with -ffp-contract=off.
//
// Tree: nodes 0 .. N-1 with children lists in CSR (child_off[N + 1], child[..]); the root is the one node nobody lists.  Edge v is the
// edge above node v; the root has none.  Leaves (no children) own the alignment rows, in ascending node order.
// Model: P(t)[i][j] = max(0, sum_k (U[i][k] * e_k) * Uinv[k][j]), e_k = exp(lambda_k * rate * t) from the tables:
//   exp_len [N][R][20]         the edge's length l            exp_half[N][R][20]   l / 2
//   exp_dist[N][F][2][R][20]   f * l and (1 - f) * l          exp_pend[1 + G][R][20]   startPend, then the pendant grid
// Partials (device and host alike): part[node][rate][state][site of the chunk] doubles, scaled per (node, site) so that the largest
// entry lies in [0.5, 1), with the int32 exponent taken out in pexp[node][site].
//   D[v]  the distal partial of edge v: the subtree below v, at v          X[v]  the proximal partial: everything else, at v's parent
// Scaled numbers: (m, e) = m * 2^e with m in [0.5, 1), or (0, 0).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>
#include "ckm_internal.h"
#include "wave_const.h"
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PL_HD __host__ __device__ __forceinline__
#else
#define PL_HD inline
#endif

namespace ckm {
namespace place {

using ckm::WAVE;
constexpr int NS = 20;                              // states
constexpr int NQ = 21;                              // query codes: the twenty states and "unknown" (all ones)
constexpr int PM = NS * NS;                         // entries of a transition matrix
constexpr uint32_t SCAN_SITES = 256;                // sites of an edge table a workgroup of the scan holds in LDS: 21 x 256 x 8 B = 43 KB
constexpr int SCAN_WAVES = 4;
constexpr uint32_t SCAN_QUERIES = 256;              // queries of one workgroup of the scan
constexpr uint32_t MAX_RATES = 8, MAX_FRAC = 32, MAX_PEND = 32;
constexpr uint32_t MAX_NODES = 1u << 22, MAX_SITES = 1u << 22, MAX_QUERIES = 1u << 22, MAX_PITCHES = 1u << 12;
constexpr char STATES[] = "ARNDCQEGHILKMFPSTWYV";  // PAML order

struct Sc { double m; int64_t e; };

PL_HD Sc norm(double x) {
  Sc r; r.m = 0.0; r.e = 0;
  if (!(x > 0.0)) return r;
  int ex = 0;
  r.m = __builtin_frexp(x, &ex);
  r.e = ex;
  return r;
}
PL_HD double scale_down(double x, int ex) { return __builtin_ldexp(x, -ex); }
// a is strictly the larger
PL_HD bool gt(Sc a, Sc b) {
  if (a.m == 0.0) return false;
  if (b.m == 0.0) return true;
  if (a.e != b.e) return a.e > b.e;
  return a.m > b.m;
}
PL_HD Sc mul(Sc a, Sc b) {
  Sc p = norm(a.m * b.m);
  if (p.m != 0.0) p.e += a.e + b.e;
  return p;
}
PL_HD Sc one() { Sc r; r.m = 0.5; r.e = 1; return r; }

PL_HD uint8_t code_of(uint8_t c) {
  for (int i = 0; i < NS; ++i) if (c == (uint8_t)STATES[i]) return (uint8_t)i;
  return (uint8_t)NS;
}

// one entry of P(t)
PL_HD double pmat_entry(const double *U, const double *Ui, const double *ex, int i, int j) {
  double s = (U[i * NS] * ex[0]) * Ui[j];
  for (int k = 1; k < NS; ++k) s = s + (U[i * NS + k] * ex[k]) * Ui[k * NS + j];
  return s < 0.0 ? 0.0 : s;
}

// sum_j P[i][j] * v[j]
PL_HD double row_dot(const double *P, int i, const double *v) {
  double s = P[i * NS] * v[0];
  for (int j = 1; j < NS; ++j) s = s + P[i * NS + j] * v[j];
  return s;
}

// Addressing of a chunk's partials: part + ((node * R + r) * NS + i) * C + s
PL_HD size_t pidx(uint32_t node, uint32_t R, uint32_t r, int i, uint32_t C, uint32_t s) { return (((size_t)node * R + r) * NS + (size_t)i) * C + s; }

PL_HD void load_vec(const double *part, uint32_t node, uint32_t R, uint32_t r, uint32_t C, uint32_t s, double *v) {
  for (int j = 0; j < NS; ++j) v[j] = part[pidx(node, R, r, j, C, s)];
}

// the (node, site) scale: every entry of the node's partial at the site divided by 2^ex, ex the exponent of the largest; returns ex
PL_HD int rescale(double *part, uint32_t node, uint32_t R, uint32_t C, uint32_t s, double mx) {
  const Sc n = norm(mx);
  const int ex = n.m == 0.0 ? 0 : (int)n.e;
  if (ex != 0)
    for (uint32_t r = 0; r < R; ++r)
      for (int i = 0; i < NS; ++i) { const size_t at = pidx(node, R, r, i, C, s); part[at] = scale_down(part[at], ex); }
  return ex;
}

// leaf v, site s of the chunk: one-hot for the twenty letters, all ones for everything else
PL_HD void leaf_site(double *D, int32_t *dexp, uint32_t v, uint32_t R, uint32_t C, uint32_t s, uint8_t code) {
  for (uint32_t r = 0; r < R; ++r)
    for (int i = 0; i < NS; ++i) D[pidx(v, R, r, i, C, s)] = (code == NS || code == i) ? 1.0 : 0.0;
  dexp[(size_t)v * C + s] = 0;
}

// internal node v, site s: the product over its children, in list order, of the messages sum_j P_c[i][j] D[c][j]
PL_HD void up_site(double *D, int32_t *dexp, uint32_t v, const uint64_t *child_off, const uint32_t *child, const double *Plen, uint32_t R, uint32_t C, uint32_t s) {
  double mx = 0.0;
  int32_t esum = 0;
  for (uint64_t k = child_off[v]; k < child_off[v + 1]; ++k) esum += dexp[(size_t)child[k] * C + s];
  for (uint32_t r = 0; r < R; ++r) {
    for (uint64_t k = child_off[v]; k < child_off[v + 1]; ++k) {
      const uint32_t c = child[k];
      double dv[NS];
      load_vec(D, c, R, r, C, s, dv);
      const double *P = Plen + ((size_t)c * R + r) * PM;
      for (int i = 0; i < NS; ++i) {
        const size_t at = pidx(v, R, r, i, C, s);
        const double msg = row_dot(P, i, dv);
        D[at] = k == child_off[v] ? msg : D[at] * msg;
      }
    }
    for (int i = 0; i < NS; ++i) { const double x = D[pidx(v, R, r, i, C, s)]; if (x > mx) mx = x; }
  }
  dexp[(size_t)v * C + s] = esum + rescale(D, v, R, C, s, mx);
}

// edge e below parent p, site s: what arrives at p from above (nothing at the root), times the messages of e's siblings in list order
PL_HD void down_site(double *X, int32_t *xexp, const double *D, const int32_t *dexp, uint32_t e, uint32_t p, bool p_is_root, const uint64_t *child_off, const uint32_t *child,
                     const double *Plen, uint32_t R, uint32_t C, uint32_t s) {
  double mx = 0.0;
  int32_t esum = p_is_root ? 0 : xexp[(size_t)p * C + s];
  for (uint64_t k = child_off[p]; k < child_off[p + 1]; ++k) if (child[k] != e) esum += dexp[(size_t)child[k] * C + s];
  for (uint32_t r = 0; r < R; ++r) {
    bool first = true;
    if (!p_is_root) {
      double xv[NS];
      load_vec(X, p, R, r, C, s, xv);
      const double *P = Plen + ((size_t)p * R + r) * PM;
      for (int i = 0; i < NS; ++i) X[pidx(e, R, r, i, C, s)] = row_dot(P, i, xv);
      first = false;
    }
    for (uint64_t k = child_off[p]; k < child_off[p + 1]; ++k) {
      const uint32_t c = child[k];
      if (c == e) continue;
      double dv[NS];
      load_vec(D, c, R, r, C, s, dv);
      const double *P = Plen + ((size_t)c * R + r) * PM;
      for (int i = 0; i < NS; ++i) {
        const size_t at = pidx(e, R, r, i, C, s);
        const double msg = row_dot(P, i, dv);
        X[at] = first ? msg : X[at] * msg;
      }
      first = false;
    }
    for (int i = 0; i < NS; ++i) { const double x = X[pidx(e, R, r, i, C, s)]; if (x > mx) mx = x; }
  }
  xexp[(size_t)e * C + s] = esum + rescale(X, e, R, C, s, mx);
}

// The attachment point on edge e for one rate: ab[i] = (pi_i * sum_j Pd[i][j] D[e][j]) * sum_j Pp[i][j] X[e][j]
PL_HD void attach_rate(const double *D, const double *X, uint32_t e, uint32_t R, uint32_t r, uint32_t C, uint32_t s, const double *Pd, const double *Pp, const double *pi, double *ab) {
  double dv[NS], xv[NS];
  load_vec(D, e, R, r, C, s, dv);
  load_vec(X, e, R, r, C, s, xv);
  for (int i = 0; i < NS; ++i) ab[i] = (pi[i] * row_dot(Pd, i, dv)) * row_dot(Pp, i, xv);
}
// a tip in state q < 20 on a pendant edge with matrix Pt, seen from the attachment point
PL_HD double tip_inner(const double *ab, const double *Pt, int q) {
  double s = ab[0] * Pt[q];
  for (int i = 1; i < NS; ++i) s = s + ab[i] * Pt[i * NS + q];
  return s;
}

// The likelihood of the reference tree alone at site s, formed once, at the root: what a tip of unknown state leaves of the site on EVERY
// edge and at every point of the grid (the pulley principle), so that unknown sites never move a ranking and an all-gap query ties on
// all edges bit for bit.  rootv[s] * 2^rootexp[s].
PL_HD void root_site(double *rootv, int32_t *rootexp, const double *D, const int32_t *dexp, uint32_t root, const double *pi, const double *weights, uint32_t R, uint32_t C, uint32_t s) {
  double v = 0.0;
  for (uint32_t r = 0; r < R; ++r) {
    double in = pi[0] * D[pidx(root, R, r, 0, C, s)];
    for (int i = 1; i < NS; ++i) in = in + pi[i] * D[pidx(root, R, r, i, C, s)];
    v = r == 0 ? weights[r] * in : v + weights[r] * in;
  }
  rootv[s] = v;
  rootexp[s] = dexp[(size_t)root * C + s];
}

// the scan's table of edge e at site s: T[q][s] for the twenty states, attachment at the midpoint, pendant startPend (exp_pend's first
// entry), all with the exponent texp[e][s]; T[20][s], the unknown tip, is the root's value with the root's exponent
PL_HD void table_site(double *T, int32_t *texp, const double *D, const int32_t *dexp, const double *X, const int32_t *xexp, uint32_t e, const double *Phalf, const double *Ppend,
                      const double *pi, const double *weights, const double *rootv, uint32_t R, uint32_t C, uint32_t s) {
  T[((size_t)e * NQ + NS) * C + s] = rootv[s];
  for (uint32_t r = 0; r < R; ++r) {
    double ab[NS];
    const double *Ph = Phalf + ((size_t)e * R + r) * PM;
    attach_rate(D, X, e, R, r, C, s, Ph, Ph, pi, ab);
    for (int q = 0; q < NS; ++q) {
      const double t = weights[r] * tip_inner(ab, Ppend + (size_t)r * PM, q);
      const size_t at = ((size_t)e * NQ + q) * C + s;
      T[at] = r == 0 ? t : T[at] + t;
    }
  }
  texp[(size_t)e * C + s] = dexp[(size_t)e * C + s] + xexp[(size_t)e * C + s];
}

// A lane's factor of a block of sixty-four sites: the site's value with the site's exponent; a lane past the sites holds one.
PL_HD Sc lane_factor(bool live, double value, int32_t ex) {
  if (!live) return one();
  Sc f = norm(value);
  if (f.m != 0.0) f.e += ex;
  return f;
}
// The cross-lane tree of a block: partners 1, 2, 4, 8, 16, 32; mantissas multiply unnormalised (64 factors in [0.5, 1) stay above
// 2^-64), exponents add, one normalisation at the end.  The host form of what the kernels do with shuffles.
inline Sc block_product(const Sc *lane) {
  double m[WAVE], m2[WAVE];
  int64_t e[WAVE], e2[WAVE];
  for (int l = 0; l < WAVE; ++l) { m[l] = lane[l].m; e[l] = lane[l].e; }
  for (int d = 1; d < WAVE; d <<= 1) {
    for (int l = 0; l < WAVE; ++l) { m2[l] = m[l] * m[l ^ d]; e2[l] = e[l] + e[l ^ d]; }
    for (int l = 0; l < WAVE; ++l) { m[l] = m2[l]; e[l] = e2[l]; }
  }
  Sc p = norm(m[0]);
  if (p.m != 0.0) p.e += e[0];
  return p;
}

// what the kernels take: device pointers of one call (ckm_place.hip fills it)
struct PlaceDev {
  const uint64_t *child_off; const uint32_t *child; const int32_t *parent, *leaf_row; uint32_t root, N, R, S, NQy, F, G, K, Keff, E;
  const uint8_t *rowcode, *qcode;                  // [rows][S], [queries][S]: 0 .. 20
  const double *weights, *pi, *Plen, *Phalf, *Pdist, *Ppend;
  const uint32_t *edges;                           // all nodes but the root, ascending
  double *D, *X, *T; int32_t *dexp, *xexp, *texp;  // one chunk
  double *rootv; int32_t *rootexp;                 // [site of the chunk]
  double *acc_m; long long *acc_e;                 // [edge node][query]
  double *racc_m; long long *racc_e;               // [query][Keff][F][G]
  int32_t *top_edge; double *scan_m; long long *scan_e; double *ref_m; long long *ref_e; int32_t *ref_f, *ref_g;      // [query][K]
};

// ---- host side, shared by the library, the host executor and the stand-alone check ---------------------------------------------------------
using ckm::ARGS_INVALID;
using ckm::ARGS_OK;
using ckm::ARGS_RANGE;

struct Args {
  uint32_t nnodes; const uint64_t *child_off; const uint32_t *child; uint64_t nchild; const double *length;
  uint32_t nsites, nrows; const uint64_t *row_off; const uint8_t *rows; uint64_t nrow_bytes;
  uint32_t nqueries; const uint64_t *q_off; const uint8_t *queries; uint64_t nquery_bytes;
  uint32_t nrates; const double *weights, *U, *Uinv, *pi, *exp_len, *exp_half;
  uint32_t nfrac; const double *exp_dist;
  uint32_t npend; const double *exp_pend;
  uint32_t max_pitches;
};
struct Out { int32_t *top_edge; double *scan_m; int64_t *scan_e; double *ref_m; int64_t *ref_e; int32_t *ref_f, *ref_g; };

// The level schedule of a checked tree: nodes by height for the upward sweep (the leaves first), edges by depth for the downward one.
struct Schedule {
  uint32_t root = 0, nleaves = 0;
  std::vector<int32_t> parent, leaf_row;            // leaf_row[v]: the alignment row of leaf v, -1 for an internal node
  std::vector<uint32_t> up_nodes, up_off, down_nodes, down_off, edges;      // up_off / down_off: the levels; edges: all nodes but the root, ascending
};

inline bool finite_nonneg(const double *p, size_t n) {
  for (size_t k = 0; k < n; ++k) if (!(p[k] >= 0.0) || !(p[k] <= 1.7976931348623157e308)) return false;
  return true;
}

// Why a call is refused; fills the schedule of one that is not.  Nothing is indexed before the offsets into it are known to be in order.
inline int check(const Args &a, Schedule &sch, std::string &why) {
  auto no = [&](int kind, const std::string &m) { why = m; return kind; };
  if (a.nrates > MAX_RATES) return no(ARGS_RANGE, "more than 8 rate categories");
  if (a.nrates < 1) return no(ARGS_INVALID, "no rate category");
  if (a.nnodes > MAX_NODES || a.nsites > MAX_SITES || a.nqueries > MAX_QUERIES) return no(ARGS_RANGE, "more than 2^22 nodes, sites or queries");
  if (a.nfrac < 1 || a.npend < 1) return no(ARGS_INVALID, "an empty grid");
  if (a.nfrac > MAX_FRAC || a.npend > MAX_PEND) return no(ARGS_RANGE, "more than 32 distal fractions or pendant lengths");
  if (a.max_pitches < 1) return no(ARGS_INVALID, "maxPitches below 1");
  if (a.max_pitches > MAX_PITCHES) return no(ARGS_RANGE, "maxPitches above 4096");
  if (a.nnodes < 3) return no(ARGS_INVALID, "a tree of fewer than two leaves");
  if (a.nsites < 1) return no(ARGS_INVALID, "no site");
  if (!a.child_off || !a.child || !a.length || !a.row_off || !a.rows || !a.q_off || !a.weights || !a.U || !a.Uinv || !a.pi || !a.exp_len || !a.exp_half || !a.exp_dist ||
      !a.exp_pend || (a.nqueries && !a.queries))
    return no(ARGS_INVALID, "NULL argument");
  const uint32_t N = a.nnodes, R = a.nrates;
  if (a.child_off[0] != 0) return no(ARGS_INVALID, "child_off does not start at 0");
  for (uint32_t v = 0; v < N; ++v) {
    if (a.child_off[v + 1] < a.child_off[v]) return no(ARGS_INVALID, "child_off falls at node " + std::to_string(v));
    if (a.child_off[v + 1] > a.nchild) return no(ARGS_INVALID, "child_off beyond the children at node " + std::to_string(v));
    if (a.child_off[v + 1] - a.child_off[v] == 1) return no(ARGS_INVALID, "node " + std::to_string(v) + " has one child");
  }
  if (a.child_off[N] != (uint64_t)N - 1) return no(ARGS_INVALID, "the children lists do not hold every node but one once");
  sch = Schedule();
  sch.parent.assign(N, -1);
  for (uint32_t v = 0; v < N; ++v)
    for (uint64_t k = a.child_off[v]; k < a.child_off[v + 1]; ++k) {
      const uint32_t c = a.child[k];
      if (c >= N || c == v) return no(ARGS_INVALID, "child " + std::to_string(c) + " of node " + std::to_string(v) + " is no node");
      if (sch.parent[c] >= 0) return no(ARGS_INVALID, "node " + std::to_string(c) + " is listed as a child twice");
      sch.parent[c] = (int32_t)v;
    }
  uint32_t nroots = 0;
  for (uint32_t v = 0; v < N; ++v) if (sch.parent[v] < 0) { sch.root = v; ++nroots; }
  if (nroots != 1) return no(ARGS_INVALID, "the tree has " + std::to_string(nroots) + " roots");
  { const uint64_t deg = a.child_off[sch.root + 1] - a.child_off[sch.root];
    if (deg != 2 && deg != 3) return no(ARGS_INVALID, "the root has " + std::to_string(deg) + " children"); }
  // depth first from the root: every node reached (no cycle beside the tree), depths and heights
  std::vector<uint32_t> depth(N, 0), height(N, 0), order;
  order.reserve(N);
  order.push_back(sch.root);
  for (size_t h = 0; h < order.size(); ++h) {
    const uint32_t v = order[h];
    for (uint64_t k = a.child_off[v]; k < a.child_off[v + 1]; ++k) { depth[a.child[k]] = depth[v] + 1; order.push_back(a.child[k]); }
  }
  if (order.size() != N) return no(ARGS_INVALID, "the children lists hold a cycle");
  for (size_t h = N; h-- > 0;) {
    const uint32_t v = order[h];
    if (sch.parent[v] >= 0) height[sch.parent[v]] = std::max(height[sch.parent[v]], height[v] + 1);
  }
  for (uint32_t v = 0; v < N; ++v)
    if (v != sch.root && !(a.length[v] >= 0.0 && a.length[v] <= 1.7976931348623157e308)) return no(ARGS_INVALID, "the length of edge " + std::to_string(v) + " is negative or not finite");
  // alignment rows: one per leaf, each of nsites characters
  sch.leaf_row.assign(N, -1);
  for (uint32_t v = 0; v < N; ++v) if (a.child_off[v + 1] == a.child_off[v]) sch.leaf_row[v] = (int32_t)sch.nleaves++;
  if (a.nrows != sch.nleaves) return no(ARGS_INVALID, "the alignment has " + std::to_string(a.nrows) + " rows for " + std::to_string(sch.nleaves) + " leaves");
  if (a.row_off[0] != 0) return no(ARGS_INVALID, "row_off does not start at 0");
  for (uint32_t k = 0; k < a.nrows; ++k) {
    if (a.row_off[k + 1] < a.row_off[k] || a.row_off[k + 1] > a.nrow_bytes) return no(ARGS_INVALID, "row_off out of order at row " + std::to_string(k));
    if (a.row_off[k + 1] - a.row_off[k] != a.nsites) return no(ARGS_INVALID, "alignment row " + std::to_string(k) + " does not have " + std::to_string(a.nsites) + " sites");
  }
  if (a.q_off[0] != 0) return no(ARGS_INVALID, "q_off does not start at 0");
  for (uint32_t k = 0; k < a.nqueries; ++k) {
    if (a.q_off[k + 1] < a.q_off[k] || a.q_off[k + 1] > a.nquery_bytes) return no(ARGS_INVALID, "q_off out of order at query " + std::to_string(k));
    if (a.q_off[k + 1] - a.q_off[k] != a.nsites) return no(ARGS_INVALID, "query " + std::to_string(k) + " does not have " + std::to_string(a.nsites) + " sites");
  }
  if (!finite_nonneg(a.weights, R) || !finite_nonneg(a.pi, NS) || !finite_nonneg(a.exp_len, (size_t)N * R * NS) || !finite_nonneg(a.exp_half, (size_t)N * R * NS) ||
      !finite_nonneg(a.exp_dist, (size_t)N * a.nfrac * 2 * R * NS) || !finite_nonneg(a.exp_pend, ((size_t)a.npend + 1) * R * NS))
    return no(ARGS_INVALID, "a weight, a frequency or a table entry is negative or not finite");
  for (int k = 0; k < PM; ++k) if (!(a.U[k] == a.U[k]) || !(a.Uinv[k] == a.Uinv[k]) || std::fabs(a.U[k]) > 1e300 || std::fabs(a.Uinv[k]) > 1e300) return no(ARGS_INVALID, "an eigenvector entry is not finite");
  // levels
  uint32_t maxh = height[sch.root], maxd = 0;
  for (uint32_t v = 0; v < N; ++v) maxd = std::max(maxd, depth[v]);
  sch.up_off.assign((size_t)maxh + 2, 0); sch.down_off.assign((size_t)maxd + 1, 0);
  for (uint32_t v = 0; v < N; ++v) { sch.up_off[height[v] + 1]++; if (v != sch.root) sch.down_off[depth[v]]++; }
  for (size_t k = 1; k < sch.up_off.size(); ++k) sch.up_off[k] += sch.up_off[k - 1];
  for (size_t k = 1; k < sch.down_off.size(); ++k) sch.down_off[k] += sch.down_off[k - 1];      // down_off[d - 1] .. down_off[d]: the edges at depth d
  sch.up_nodes.resize(N); sch.down_nodes.resize(N - 1);
  { std::vector<uint32_t> ua(sch.up_off.begin(), sch.up_off.end() - 1), da(maxd, 0);
    for (uint32_t d = 1; d < maxd; ++d) da[d] = sch.down_off[d];
    for (uint32_t v = 0; v < N; ++v) { sch.up_nodes[ua[height[v]]++] = v; if (v != sch.root) sch.down_nodes[da[depth[v] - 1]++] = v; } }
  for (uint32_t v = 0; v < N; ++v) if (v != sch.root) sch.edges.push_back(v);
  return ARGS_OK;
}

// bytes a site of a chunk needs on the device: two partials with their exponents, and the edge tables with theirs
inline uint64_t site_bytes(uint32_t N, uint32_t R) { return (uint64_t)N * (2ull * R * NS * 8 + 8) + (uint64_t)N * (NQ * 8 + 4); }
// sites of a chunk under the budget: a multiple of 64, at least 64; all sites when they fit
inline uint32_t chunk_sites(uint32_t nsites, uint32_t N, uint32_t R, uint64_t budget_bytes) {
  uint64_t c = budget_bytes / site_bytes(N, R) / WAVE * WAVE;
  if (c < (uint64_t)WAVE) c = WAVE;
  return c >= nsites ? nsites : (uint32_t)c;
}

// the K best of n scaled numbers, larger first, ties to the lower index: entry k of the result, given the previous pick (prev < 0: none)
inline int32_t next_best(const Sc *v, const uint32_t *ids, uint32_t n, int32_t prev_pos) {
  int32_t best = -1;
  for (uint32_t k = 0; k < n; ++k) {
    if (prev_pos >= 0 && !(gt(v[prev_pos], v[k]) || (!gt(v[k], v[prev_pos]) && ids[k] > ids[prev_pos]))) continue;      // not after the previous pick
    if (best < 0 || gt(v[k], v[best])) best = (int32_t)k;
  }
  return best;
}

// ---- the host executor: the kernels restated as loops over their threads, the same functions, the same chunk loop ----------------------------
struct HostTables { std::vector<double> Plen, Phalf, Ppend; };
inline void host_tables(const Args &a, HostTables &t) {
  const uint32_t N = a.nnodes, R = a.nrates;
  t.Plen.resize((size_t)N * R * PM); t.Phalf.resize((size_t)N * R * PM); t.Ppend.resize(((size_t)a.npend + 1) * R * PM);
  for (size_t m = 0; m < (size_t)N * R; ++m)
    for (int i = 0; i < NS; ++i)
      for (int j = 0; j < NS; ++j) {
        t.Plen[m * PM + i * NS + j] = pmat_entry(a.U, a.Uinv, a.exp_len + m * NS, i, j);
        t.Phalf[m * PM + i * NS + j] = pmat_entry(a.U, a.Uinv, a.exp_half + m * NS, i, j);
      }
  for (size_t m = 0; m < ((size_t)a.npend + 1) * R; ++m)
    for (int i = 0; i < NS; ++i)
      for (int j = 0; j < NS; ++j) t.Ppend[m * PM + i * NS + j] = pmat_entry(a.U, a.Uinv, a.exp_pend + m * NS, i, j);
}

struct HostChunk { std::vector<double> D, X, T, rootv; std::vector<int32_t> dexp, xexp, texp, rootexp; uint32_t C = 0; };
inline void host_sweeps(const Args &a, const Schedule &sch, const HostTables &t, uint32_t s0, uint32_t C, bool tables, HostChunk &h) {
  const uint32_t N = a.nnodes, R = a.nrates;
  const double nan = std::nan("");
  h.C = C;
  h.D.assign((size_t)N * R * NS * C, nan); h.X.assign((size_t)N * R * NS * C, nan); h.dexp.assign((size_t)N * C, 0x7fffffff); h.xexp.assign((size_t)N * C, 0x7fffffff);
  for (size_t lv = 0; lv + 1 < sch.up_off.size(); ++lv)
    for (uint32_t k = sch.up_off[lv]; k < sch.up_off[lv + 1]; ++k) {
      const uint32_t v = sch.up_nodes[k];
      for (uint32_t s = 0; s < C; ++s)
        if (sch.leaf_row[v] >= 0) leaf_site(h.D.data(), h.dexp.data(), v, R, C, s, code_of(a.rows[a.row_off[sch.leaf_row[v]] + s0 + s]));
        else up_site(h.D.data(), h.dexp.data(), v, a.child_off, a.child, t.Plen.data(), R, C, s);
    }
  h.rootv.assign(C, nan); h.rootexp.assign(C, 0x7fffffff);
  for (uint32_t s = 0; s < C; ++s) root_site(h.rootv.data(), h.rootexp.data(), h.D.data(), h.dexp.data(), sch.root, a.pi, a.weights, R, C, s);
  for (size_t lv = 0; lv + 1 < sch.down_off.size(); ++lv)
    for (uint32_t k = sch.down_off[lv]; k < sch.down_off[lv + 1]; ++k) {
      const uint32_t v = sch.down_nodes[k], p = (uint32_t)sch.parent[v];
      for (uint32_t s = 0; s < C; ++s) down_site(h.X.data(), h.xexp.data(), h.D.data(), h.dexp.data(), v, p, p == sch.root, a.child_off, a.child, t.Plen.data(), R, C, s);
    }
  if (!tables) return;
  h.T.assign((size_t)N * NQ * C, nan); h.texp.assign((size_t)N * C, 0x7fffffff);
  for (uint32_t e : sch.edges)
    for (uint32_t s = 0; s < C; ++s) table_site(h.T.data(), h.texp.data(), h.D.data(), h.dexp.data(), h.X.data(), h.xexp.data(), e, t.Phalf.data(), t.Ppend.data(), a.pi, a.weights, h.rootv.data(), R, C, s);
}

// info[0] = chunks, info[1] = sites of a chunk
inline int run_host(const Args &a, uint64_t budget_bytes, const Out &o, uint64_t *info, std::string &why) {
  Schedule sch;
  const int kind = check(a, sch, why);
  if (kind) return kind;
  const uint32_t N = a.nnodes, R = a.nrates, S = a.nsites, NQy = a.nqueries, K = a.max_pitches, E = N - 1, F = a.nfrac, G = a.npend;
  const uint32_t Keff = std::min(K, E), C = chunk_sites(S, N, R, budget_bytes);
  if (info) { info[0] = (S + C - 1) / C; info[1] = C; }
  for (size_t k = 0; k < (size_t)NQy * K; ++k) { o.top_edge[k] = -1; o.scan_m[k] = o.ref_m[k] = 0.0; o.scan_e[k] = o.ref_e[k] = 0; o.ref_f[k] = o.ref_g[k] = -1; }
  if (!NQy) return ARGS_OK;
  HostTables t;
  host_tables(a, t);
  std::vector<uint8_t> qcode((size_t)NQy * S);
  for (uint32_t q = 0; q < NQy; ++q) for (uint32_t s = 0; s < S; ++s) qcode[(size_t)q * S + s] = code_of(a.queries[a.q_off[q] + s]);
  HostChunk h;
  // scan
  std::vector<Sc> acc((size_t)N * NQy, one());
  for (uint32_t s0 = 0; s0 < S; s0 += C) {
    const uint32_t c = std::min(C, S - s0);
    host_sweeps(a, sch, t, s0, c, true, h);
    for (uint32_t e : sch.edges)
      for (uint32_t q = 0; q < NQy; ++q) {
        Sc run = acc[(size_t)e * NQy + q];
        for (uint32_t b = 0; b < c; b += WAVE) {
          Sc lane[WAVE];
          for (uint32_t l = 0; l < (uint32_t)WAVE; ++l) {
            const uint32_t s = b + l;
            const int code = s < c ? qcode[(size_t)q * S + s0 + s] : 0;
            lane[l] = s < c ? lane_factor(true, h.T[((size_t)e * NQ + code) * c + s], code == NS ? h.rootexp[s] : h.texp[(size_t)e * c + s]) : lane_factor(false, 0.0, 0);
          }
          run = mul(run, block_product(lane));
        }
        acc[(size_t)e * NQy + q] = run;
      }
  }
  // the best Keff edges of every query
  std::vector<Sc> col(E);
  for (uint32_t q = 0; q < NQy; ++q) {
    for (uint32_t k = 0; k < E; ++k) col[k] = acc[(size_t)sch.edges[k] * NQy + q];
    int32_t prev = -1;
    for (uint32_t k = 0; k < Keff; ++k) {
      prev = next_best(col.data(), sch.edges.data(), E, prev);
      o.top_edge[(size_t)q * K + k] = (int32_t)sch.edges[prev]; o.scan_m[(size_t)q * K + k] = col[prev].m; o.scan_e[(size_t)q * K + k] = col[prev].e;
    }
  }
  // refine: every kept (query, edge) on the grid
  std::vector<Sc> racc((size_t)NQy * Keff * F * G, one());
  std::vector<double> Pd((size_t)R * PM), Pp((size_t)R * PM), val((size_t)G * WAVE);
  for (uint32_t s0 = 0; s0 < S; s0 += C) {
    const uint32_t c = std::min(C, S - s0);
    if (C < S || h.C != c) host_sweeps(a, sch, t, s0, c, false, h);
    for (uint32_t q = 0; q < NQy; ++q)
      for (uint32_t k = 0; k < Keff; ++k) {
        const uint32_t e = (uint32_t)o.top_edge[(size_t)q * K + k];
        for (uint32_t f = 0; f < F; ++f) {
          for (uint32_t r = 0; r < R; ++r)
            for (int i = 0; i < NS; ++i)
              for (int j = 0; j < NS; ++j) {
                Pd[(size_t)r * PM + i * NS + j] = pmat_entry(a.U, a.Uinv, a.exp_dist + ((((size_t)e * F + f) * 2 + 0) * R + r) * NS, i, j);
                Pp[(size_t)r * PM + i * NS + j] = pmat_entry(a.U, a.Uinv, a.exp_dist + ((((size_t)e * F + f) * 2 + 1) * R + r) * NS, i, j);
              }
          for (uint32_t b = 0; b < c; b += WAVE) {
            for (uint32_t l = 0; l < (uint32_t)WAVE; ++l) {
              const uint32_t s = b + l;
              if (s >= c) continue;
              const int code = qcode[(size_t)q * S + s0 + s];
              if (code == NS) { for (uint32_t g = 0; g < G; ++g) val[(size_t)g * WAVE + l] = h.rootv[s]; continue; }
              for (uint32_t r = 0; r < R; ++r) {
                double ab[NS];
                attach_rate(h.D.data(), h.X.data(), e, R, r, c, s, Pd.data() + (size_t)r * PM, Pp.data() + (size_t)r * PM, a.pi, ab);
                for (uint32_t g = 0; g < G; ++g) {
                  const double tv = a.weights[r] * tip_inner(ab, t.Ppend.data() + ((size_t)(g + 1) * R + r) * PM, code);
                  val[(size_t)g * WAVE + l] = r == 0 ? tv : val[(size_t)g * WAVE + l] + tv;
                }
              }
            }
            for (uint32_t g = 0; g < G; ++g) {
              Sc lane[WAVE];
              for (uint32_t l = 0; l < (uint32_t)WAVE; ++l) {
                const uint32_t s = b + l;
                lane[l] = s < c ? lane_factor(true, val[(size_t)g * WAVE + l], qcode[(size_t)q * S + s0 + s] == NS ? h.rootexp[s] : h.dexp[(size_t)e * c + s] + h.xexp[(size_t)e * c + s])
                                : lane_factor(false, 0.0, 0);
              }
              Sc &ra = racc[(((size_t)q * Keff + k) * F + f) * G + g];
              ra = mul(ra, block_product(lane));
            }
          }
        }
      }
  }
  for (uint32_t q = 0; q < NQy; ++q)
    for (uint32_t k = 0; k < Keff; ++k) {
      const Sc *ra = &racc[((size_t)q * Keff + k) * F * G];
      uint32_t best = 0;
      for (uint32_t fg = 1; fg < F * G; ++fg) if (gt(ra[fg], ra[best])) best = fg;
      const size_t at = (size_t)q * K + k;
      o.ref_m[at] = ra[best].m; o.ref_e[at] = ra[best].e; o.ref_f[at] = (int32_t)(best / G); o.ref_g[at] = (int32_t)(best % G);
    }
  return ARGS_OK;
}

}  // namespace place
}  // namespace ckm
