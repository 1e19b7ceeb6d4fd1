// genetree_dev.h -- the data layout, the arithmetic and the round cuts of the gene-tree tests (what scripts/genometreeworkflow/
// paralogTest.py and consistencyTest.py of the reference ask of dendropy, tree by tree), written once for the kernels
// (kernels_genetree.hip), for the host executor (run_host below, genetree_host.cpp) and for the stand-alone check.  DESIGN section 28.
//
// Forest: T trees.  The leaves of a tree are numbered in the order they are written, so the subtree of a node is the leaf range
//   [first, last) and a count below a node is a difference of two prefix sums.
//   Per tree t: nodes node_off[t] .. node_off[t+1], in pre-order as written (a parent stands before its children, node 0 is the root);
//     per node first, last (leaf positions in the tree), parent (node in the tree, NONE for the root), length (the edge above it; the
//     root's is 0 when the text gives none) and internal (1: it has children).  Multifurcations and single-child nodes are allowed.
//   Per leaf, leaf_off[t] .. leaf_off[t+1] in tree order: genome (dense per tree), species (dense per tree, NONE: not counted) and,
//     rank-major over the whole forest (leaf_class[r * nleaves + leaf], r = 0 domain, 1 phylum, 2 class), the class of the leaf, dense
//     per tree and rank by first appearance.
//   Per (tree, rank): classes class_off[3t+r] .. class_off[3t+r+1], per class its total in the tree.
//   Per tree: groups group_off[t] .. group_off[t+1], one per genome with more than one leaf in the tree; per group its same-genome leaf
//     pairs gpair_off[g] .. gpair_off[g+1], pair_a < pair_b leaf positions in the tree.
// Outputs: consistency [classes] doubles, pair_flag [pairs] bytes, group_node [groups] (node in the tree, NONE when no pair of the group
//   is flagged) and group_mixed [groups] bytes.
// Arithmetic: integer sums, then ONE IEEE division per quotient (quot1, quot2); a maximum of correctly rounded quotients does not depend
//   on the order of its reduction.  Path lengths are summed in the fixed orders of pair_flag below; no libm, no contraction.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>
#include "ckm_internal.h"
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GN_HD __host__ __device__ __forceinline__
#else
#define GN_HD inline
#endif

namespace ckm {
namespace genetree {

constexpr uint32_t MAX_LEAVES = 1u << 14;           // per tree: the prefix sums of a class fit 16 bits of LDS each
constexpr uint32_t MAX_NODES = 1u << 15;            // per tree
constexpr uint32_t MAX_CLASSES = 65535;             // per tree and rank
constexpr uint32_t MAX_TREES = 1u << 20;
constexpr uint32_t NONE = 0xffffffffu;
constexpr int RANKS = 3;
using ckm::ARGS_INVALID;
using ckm::ARGS_OK;
using ckm::ARGS_RANGE;

struct Args {
  uint32_t ntrees;
  const uint32_t *node_off, *leaf_off, *class_off, *group_off, *gpair_off;
  const uint32_t *first, *last, *parent;   const double *length;   const uint8_t *internal;
  const uint32_t *leaf_genome, *leaf_species, *leaf_class;
  const uint32_t *class_total;
  const uint32_t *pair_a, *pair_b;
};
struct Out { double *consistency; uint8_t *pair_flag; uint32_t *group_node; uint8_t *group_mixed; };

// One tree as the per-item functions see it: pointers at the tree's first node, leaf, class of rank 0 and pair.
struct Tree {
  uint32_t nnodes, nleaves;
  const uint32_t *first, *last, *parent;   const double *length;   const uint8_t *internal;
  const uint32_t *leaf_node;               // leaf position -> node
  const uint32_t *species;
};

// The device arrays of one round, trees t0 .. t1.  The offset arrays are the call's (they index the whole forest); every other array
// begins at the round's first node, leaf, class, pair or group, whose indices in the forest are node0 .. group0.
struct Round {
  uint32_t t0, t1, node0, leaf0, class0, pair0, group0, nleaves, nclasses, npairs, ngroups;
  const uint32_t *node_off, *leaf_off, *class_off, *group_off, *gpair_off;
  const uint32_t *first, *last, *parent;   const double *length;   const uint8_t *internal;
  const uint32_t *leaf_node, *species, *leaf_class /* [3][nleaves] */, *class_total, *pair_a, *pair_b;
  double *consistency;   uint8_t *pair_flag;   uint32_t *group_node;   uint8_t *group_mixed;
};

// consistencyTest.py:154-165 -- k of the class's T leaves are among the n leaves below the node, N leaves in the tree
GN_HD double quot1(uint32_t k, uint32_t n, uint32_t T) { return (double)k / (double)(T + (n - k)); }
GN_HD double quot2(uint32_t k, uint32_t n, uint32_t T, uint32_t N) { return (double)(T - k) / (double)(T + ((N - n) - (T - k))); }
GN_HD double node_quot(uint32_t k, uint32_t n, uint32_t T, uint32_t N) {
  const double c1 = quot1(k, n, T), c2 = quot2(k, n, T, N);
  return c2 > c1 ? c2 : c1;
}

// distance_from_root of the golden tool's stand-in: the node's own length first, then every ancestor's up to and including the root's
GN_HD double root_distance(const Tree &t, uint32_t v) {
  double d = t.length[v];
  for (uint32_t p = t.parent[v]; p != NONE; p = t.parent[p]) d = d + t.length[p];
  return d;
}
// paralogTest.py:44-65 for the leaves at positions a < b: the common ancestor is the lowest ancestor of a whose range holds b (the deepest
// node over both); one running sum up the first side to it, then the second side added onto the same sum; two root distances when it is
// the root.  The flag: distance > 0.
GN_HD uint8_t pair_flag(const Tree &t, uint32_t a, uint32_t b) {
  const uint32_t va = t.leaf_node[a], vb = t.leaf_node[b];
  uint32_t m = t.parent[va];
  while (t.last[m] <= b) m = t.parent[m];
  double dist;
  if (t.parent[m] == NONE) {
    dist = root_distance(t, va) + root_distance(t, vb);
  } else {
    dist = t.length[va];
    for (uint32_t p = t.parent[va]; p != m; p = t.parent[p]) dist = dist + t.length[p];
    dist = dist + t.length[vb];
    for (uint32_t p = t.parent[vb]; p != m; p = t.parent[p]) dist = dist + t.length[p];
  }
  return dist > 0.0 ? 1 : 0;
}
// whether node v (internal) covers the leaf positions lo .. hi
GN_HD bool covers(const Tree &t, uint32_t v, uint32_t lo, uint32_t hi) { return t.internal[v] && t.first[v] <= lo && t.last[v] > hi; }

// bytes a tree keeps resident in a round: its nodes, leaves, classes, pairs and groups with their outputs
GN_HD uint64_t tree_bytes(uint64_t nodes, uint64_t leaves, uint64_t classes, uint64_t pairs, uint64_t groups) {
  return nodes * 21 + leaves * 24 + classes * 12 + pairs * 9 + groups * 9 + 64;
}
inline uint64_t tree_bytes_of(const Args &a, uint32_t t) {
  const uint32_t g0 = a.group_off[t], g1 = a.group_off[t + 1];
  return tree_bytes(a.node_off[t + 1] - a.node_off[t], a.leaf_off[t + 1] - a.leaf_off[t], a.class_off[3 * t + 3] - a.class_off[3 * t], a.gpair_off[g1] - a.gpair_off[g0], g1 - g0);
}
// the round that begins at tree t0: trees t0 .. the returned one; at least one tree, then as many as fit the budget
inline uint32_t round_end(const Args &a, uint32_t t0, uint64_t budget) {
  uint64_t used = tree_bytes_of(a, t0);
  uint32_t t = t0 + 1;
  while (t < a.ntrees && used + tree_bytes_of(a, t) <= budget) used += tree_bytes_of(a, t++);
  return t;
}

// Why a call would be refused.  Everything the walks above rely on is established here: offsets ascend, a parent precedes its child,
// the children of a node tile its range in order, the k-th leaf node is position k, the root covers the tree, the class totals are the
// counts of the leaves, the pairs name leaves of one genome.
inline int check(const Args &a, std::string &why) {
  auto bad = [&](int kind, const std::string &w) { why = w; return kind; };
  if (!a.node_off || !a.leaf_off || !a.class_off || !a.group_off || !a.gpair_off) return bad(ARGS_INVALID, "NULL argument");
  if (a.ntrees > MAX_TREES) return bad(ARGS_RANGE, "more than 2^20 trees in a call");
  if (a.node_off[0] || a.leaf_off[0] || a.class_off[0] || a.group_off[0] || a.gpair_off[0]) return bad(ARGS_INVALID, "an offset array does not begin at 0");
  const uint32_t T = a.ntrees;
  for (uint32_t t = 0; t < T; ++t) {
    if (a.node_off[t + 1] < a.node_off[t] || a.leaf_off[t + 1] < a.leaf_off[t] || a.group_off[t + 1] < a.group_off[t]) return bad(ARGS_INVALID, "offsets of tree " + std::to_string(t) + " descend");
    for (int r = 0; r < RANKS; ++r) if (a.class_off[3 * t + r + 1] < a.class_off[3 * t + r]) return bad(ARGS_INVALID, "class offsets of tree " + std::to_string(t) + " descend");
  }
  const uint64_t NN = a.node_off[T], NL = a.leaf_off[T], NC = a.class_off[3 * (uint64_t)T], NG = a.group_off[T];
  for (uint64_t g = 0; g < NG; ++g) if (a.gpair_off[g + 1] < a.gpair_off[g]) return bad(ARGS_INVALID, "pair offsets descend");
  const uint64_t NP = a.gpair_off[NG];
  if ((NN && (!a.first || !a.last || !a.parent || !a.length || !a.internal)) || (NL && (!a.leaf_genome || !a.leaf_species || !a.leaf_class)) || (NC && !a.class_total) ||
      (NP && (!a.pair_a || !a.pair_b)))
    return bad(ARGS_INVALID, "NULL argument");
  std::vector<uint32_t> next, count;
  for (uint32_t t = 0; t < T; ++t) {
    const std::string name = "tree " + std::to_string(t);
    const uint32_t n0 = a.node_off[t], nn = a.node_off[t + 1] - n0, l0 = a.leaf_off[t], nl = a.leaf_off[t + 1] - l0;
    if (nl > MAX_LEAVES) return bad(ARGS_RANGE, name + " has more than 2^14 leaves");
    if (nn > MAX_NODES) return bad(ARGS_RANGE, name + " has more than 2^15 nodes");
    for (int r = 0; r < RANKS; ++r) if (a.class_off[3 * t + r + 1] - a.class_off[3 * t + r] > MAX_CLASSES) return bad(ARGS_RANGE, name + " has more than 65535 classes at a rank");
    if (!nn || !nl) return bad(ARGS_INVALID, name + " is empty");
    const uint32_t *first = a.first + n0, *last = a.last + n0, *parent = a.parent + n0;
    next.assign(nn, 0);
    uint32_t leaves = 0;
    for (uint32_t v = 0; v < nn; ++v) {
      const double len = a.length[n0 + v];
      if (!(len - len == 0.0)) return bad(ARGS_INVALID, name + " has an edge length that is not finite");
      if (first[v] >= last[v] || last[v] > nl) return bad(ARGS_INVALID, name + " has a node whose leaf range is outside the tree");
      if (v == 0) {
        if (parent[v] != NONE || first[v] != 0 || last[v] != nl) return bad(ARGS_INVALID, name + ": the first node is not a root over every leaf");
      } else {
        const uint32_t p = parent[v];
        if (p >= v) return bad(ARGS_INVALID, name + " has a parent that does not precede its child");
        if (!a.internal[n0 + p] || first[v] != next[p] || last[v] > last[p]) return bad(ARGS_INVALID, name + ": the children of a node do not tile its leaf range");
        next[p] = last[v];
      }
      next[v] = first[v];
      if (!a.internal[n0 + v]) {
        if (first[v] != leaves || last[v] != leaves + 1) return bad(ARGS_INVALID, name + ": a leaf node is not at its position");
        ++leaves;
      }
    }
    for (uint32_t v = 0; v < nn; ++v) if (a.internal[n0 + v] && next[v] != last[v]) return bad(ARGS_INVALID, name + ": the children of a node do not tile its leaf range");
    if (leaves != nl) return bad(ARGS_INVALID, name + ": leaf nodes and leaves differ in number");
    for (int r = 0; r < RANKS; ++r) {
      const uint32_t c0 = a.class_off[3 * t + r], nc = a.class_off[3 * t + r + 1] - c0;
      count.assign(nc, 0);
      for (uint32_t k = 0; k < nl; ++k) {
        const uint32_t c = a.leaf_class[(uint64_t)r * NL + l0 + k];
        if (c >= nc) return bad(ARGS_INVALID, name + " has a class index beyond its class count");
        ++count[c];
      }
      for (uint32_t c = 0; c < nc; ++c) if (count[c] != a.class_total[c0 + c] || !count[c]) return bad(ARGS_INVALID, name + ": a class total is not the count of its leaves");
    }
    for (uint32_t g = a.group_off[t]; g < a.group_off[t + 1]; ++g)
      for (uint32_t k = a.gpair_off[g]; k < a.gpair_off[g + 1]; ++k) {
        if (a.pair_a[k] >= a.pair_b[k] || a.pair_b[k] >= nl) return bad(ARGS_INVALID, name + " has a pair that names a leaf beyond the tree or is not ascending");
        if (a.leaf_genome[l0 + a.pair_a[k]] != a.leaf_genome[l0 + a.pair_b[k]]) return bad(ARGS_INVALID, name + " has a pair of two genomes");
      }
  }
  return ARGS_OK;
}

// leaf position -> node, for the trees t0 .. t1 (the non-internal nodes in order), at leaf_node[leaf - leaf_off[t0]]
inline void leaf_nodes_of(const Args &a, uint32_t t0, uint32_t t1, std::vector<uint32_t> &leaf_node) {
  leaf_node.resize(a.leaf_off[t1] - a.leaf_off[t0]);
  uint32_t at = 0;
  for (uint32_t t = t0; t < t1; ++t)
    for (uint32_t v = a.node_off[t]; v < a.node_off[t + 1]; ++v)
      if (!a.internal[v]) leaf_node[at++] = v - a.node_off[t];
}

// The host executor: the same rounds, the same per-item functions, loops where the device has lanes.  counts: rounds, trees.
inline int run_host(const Args &a, uint64_t budget, const Out &o, uint64_t counts[2], std::string &why) {
  const int kind = check(a, why);
  if (kind != ARGS_OK) return kind;
  const uint64_t NL = a.leaf_off[a.ntrees];
  std::vector<uint32_t> leaf_node, pre;
  counts[0] = 0; counts[1] = a.ntrees;
  for (uint32_t t0 = 0; t0 < a.ntrees;) {
    const uint32_t t1 = round_end(a, t0, budget);
    leaf_nodes_of(a, t0, t1, leaf_node);
    for (uint32_t t = t0; t < t1; ++t) {
      const uint32_t n0 = a.node_off[t], l0 = a.leaf_off[t];
      const Tree tr{a.node_off[t + 1] - n0, a.leaf_off[t + 1] - l0, a.first + n0, a.last + n0, a.parent + n0, a.length + n0, a.internal + n0, leaf_node.data() + (l0 - a.leaf_off[t0]),
                    a.leaf_species + l0};
      for (int r = 0; r < RANKS; ++r)
        for (uint32_t c = a.class_off[3 * t + r]; c < a.class_off[3 * t + r + 1]; ++c) {
          const uint32_t cls = c - a.class_off[3 * t + r], T = a.class_total[c];
          pre.assign(tr.nleaves + 1, 0);
          for (uint32_t k = 0; k < tr.nleaves; ++k) pre[k + 1] = pre[k] + (a.leaf_class[(uint64_t)r * NL + l0 + k] == cls ? 1u : 0u);
          double best = 0.0;
          for (uint32_t v = 0; v < tr.nnodes; ++v)
            if (tr.internal[v]) {
              const double q = node_quot(pre[tr.last[v]] - pre[tr.first[v]], tr.last[v] - tr.first[v], T, tr.nleaves);
              if (q > best) best = q;
            }
          o.consistency[c] = best;
        }
      for (uint32_t g = a.group_off[t]; g < a.group_off[t + 1]; ++g) {
        uint32_t lo = NONE, hi = 0;
        for (uint32_t k = a.gpair_off[g]; k < a.gpair_off[g + 1]; ++k) {
          const uint8_t f = pair_flag(tr, a.pair_a[k], a.pair_b[k]);
          o.pair_flag[k] = f;
          if (f) { if (a.pair_a[k] < lo) lo = a.pair_a[k]; if (a.pair_b[k] > hi) hi = a.pair_b[k]; }
        }
        uint32_t node = NONE; uint8_t mixed = 0;
        if (lo != NONE) {
          for (uint32_t v = 0; v < tr.nnodes; ++v) if (covers(tr, v, lo, hi)) node = v;      // the last in pre-order: the deepest
          uint32_t smin = NONE, smax = 0;
          for (uint32_t k = tr.first[node]; k < tr.last[node]; ++k) {
            const uint32_t s = tr.species[k];
            if (s != NONE) { if (s < smin) smin = s; if (s > smax) smax = s; }
          }
          mixed = (smin != NONE && smin != smax) ? 1 : 0;
        }
        o.group_node[g] = node;
        o.group_mixed[g] = mixed;
      }
    }
    counts[0] += 1;
    t0 = t1;
  }
  return ARGS_OK;
}

}  // namespace genetree
}  // namespace ckm
