// kernels_genetree.hip -- the gene-tree tests on the device (what paralogTest.py and consistencyTest.py of the reference's
// scripts/genometreeworkflow ask of dendropy).  gfx950 only.  The layout and the arithmetic are genetree_dev.h, shared with the host
// executor; the quotients are one IEEE double division each and the path sums run in the header's order (the library's
// -ffp-contract=off -fno-fast-math).  Every launch covers the trees of a round; every output word has one writer; no atomics, no
// waiting between blocks.
//
//   gn_consistency  a workgroup of 256 per (tree, rank, class).  The class's 0/1 indicator over the leaves is scanned into LDS, 256
//                   leaves a step: a ballot per wavefront, the lane's bits below it, the counts of the wavefronts before it, the
//                   carry of the steps before.  A lane per internal node then reads two prefix values and forms both quotients; the
//                   maximum goes across the wavefront by a butterfly and across the four wavefronts through LDS.
//   gn_flags        a lane per same-genome pair: pair_flag (the walk up both sides).
//   gn_conspecific  a wavefront per (tree, group): min / max of the flagged leaf positions over the group's pairs, the deepest node
//                   whose range covers them over the tree's nodes, min / max of the counted species over that node's leaves.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "genetree_dev.h"
#include "wave_const.h"

namespace ckm {
using namespace genetree;

// the last j in [lo, hi) with off[j] <= x (off ascends, off[lo] <= x)
__device__ __forceinline__ uint32_t span_of(const uint32_t *__restrict__ off, uint32_t lo, uint32_t hi, uint32_t x) {
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (off[mid] <= x) lo = mid; else hi = mid;
  }
  return lo;
}
__device__ __forceinline__ Tree tree_of(const Round &R, uint32_t t) {
  const uint32_t n0 = R.node_off[t] - R.node0, l0 = R.leaf_off[t] - R.leaf0;
  return Tree{R.node_off[t + 1] - R.node_off[t], R.leaf_off[t + 1] - R.leaf_off[t], R.first + n0, R.last + n0, R.parent + n0, R.length + n0, R.internal + n0, R.leaf_node + l0, R.species + l0};
}
__device__ __forceinline__ uint32_t wave_min(uint32_t x) {
  for (int off = WAVE / 2; off; off >>= 1) { const uint32_t y = (uint32_t)__shfl_xor((int)x, off); x = y < x ? y : x; }
  return x;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t x) {
  for (int off = WAVE / 2; off; off >>= 1) { const uint32_t y = (uint32_t)__shfl_xor((int)x, off); x = y > x ? y : x; }
  return x;
}

__global__ __launch_bounds__(256) void gn_consistency(const Round R) {
  __shared__ uint16_t pre[MAX_LEAVES + 1];
  __shared__ uint32_t wcount[4];
  __shared__ double wbest[4];
  const uint32_t tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid / WAVE;
  const uint32_t c = R.class0 + blockIdx.x;                                       // (the grid is the round's classes)
  const uint32_t j = span_of(R.class_off, 3 * R.t0, 3 * R.t1, c);                // spans without a class are passed over: the last one that begins at or before c
  const uint32_t t = j / 3, r = j % 3, cls = c - R.class_off[j];
  const uint32_t n0 = R.node_off[t] - R.node0, nn = R.node_off[t + 1] - R.node_off[t], nl = R.leaf_off[t + 1] - R.leaf_off[t];
  const uint32_t *__restrict__ leaf_cls = R.leaf_class + (uint64_t)r * R.nleaves + (R.leaf_off[t] - R.leaf0);
  const uint32_t T = R.class_total[c - R.class0];
  if (tid == 0) pre[0] = 0;
  uint32_t carry = 0;
  for (uint32_t base = 0; base < nl; base += 256) {
    const uint32_t k = base + tid;
    const bool bit = k < nl && leaf_cls[k] == cls;
    const unsigned long long m = __ballot(bit);
    if (lane == 0) wcount[w] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t before = carry, all = 0;
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) { before += i < w ? wcount[i] : 0u; all += wcount[i]; }
    if (k < nl) pre[k + 1] = (uint16_t)(before + (uint32_t)__popcll(m & (~0ull >> (WAVE - 1 - lane))));
    carry += all;
    __syncthreads();                                                              // (wcount is written again in the next step; pre is read below)
  }
  double best = 0.0;
  for (uint32_t v = tid; v < nn; v += 256)
    if (R.internal[n0 + v]) {
      const uint32_t f = R.first[n0 + v], l = R.last[n0 + v];
      const double q = node_quot((uint32_t)pre[l] - (uint32_t)pre[f], l - f, T, nl);
      best = q > best ? q : best;
    }
  for (int off = WAVE / 2; off; off >>= 1) { const double y = __shfl_xor(best, off); best = y > best ? y : best; }
  if (lane == 0) wbest[w] = best;
  __syncthreads();
  if (tid == 0) {
    for (int i = 1; i < 4; ++i) best = wbest[i] > best ? wbest[i] : best;
    R.consistency[c - R.class0] = best;
  }
}

__global__ __launch_bounds__(256) void gn_flags(const Round R) {
  const uint32_t at = blockIdx.x * 256 + threadIdx.x;
  if (at >= R.npairs) return;
  const uint32_t k = R.pair0 + at;
  // the tree whose groups hold pair k: the last t with gpair_off[group_off[t]] <= k
  uint32_t lo = R.t0, hi = R.t1;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (R.gpair_off[R.group_off[mid]] <= k) lo = mid; else hi = mid;
  }
  R.pair_flag[at] = pair_flag(tree_of(R, lo), R.pair_a[at], R.pair_b[at]);
}

__global__ __launch_bounds__(256) void gn_conspecific(const Round R) {
  const uint32_t lane = threadIdx.x & (WAVE - 1), at = blockIdx.x * 4 + threadIdx.x / WAVE;
  if (at >= R.ngroups) return;                                                    // (a whole wavefront leaves; the kernel has no barrier)
  const uint32_t g = R.group0 + at;
  const Tree tr = tree_of(R, span_of(R.group_off, R.t0, R.t1, g));
  uint32_t lo = NONE, hi = 0;
  for (uint32_t k = R.gpair_off[g] + lane; k < R.gpair_off[g + 1]; k += WAVE)
    if (R.pair_flag[k - R.pair0]) {
      const uint32_t a = R.pair_a[k - R.pair0], b = R.pair_b[k - R.pair0];
      lo = a < lo ? a : lo;
      hi = b > hi ? b : hi;
    }
  lo = wave_min(lo);
  hi = wave_max(hi);
  uint32_t node = NONE, mixed = 0;
  if (lo != NONE) {
    node = 0;                                                                     // the root covers every leaf; a node further down has a larger index
    for (uint32_t v = lane; v < tr.nnodes; v += WAVE) if (covers(tr, v, lo, hi)) node = v;
    node = wave_max(node);
    uint32_t smin = NONE, smax = 0;
    for (uint32_t k = tr.first[node] + lane; k < tr.last[node]; k += WAVE) {
      const uint32_t s = tr.species[k];
      if (s != NONE) { smin = s < smin ? s : smin; smax = s > smax ? s : smax; }
    }
    smin = wave_min(smin);
    smax = wave_max(smax);
    mixed = (smin != NONE && smin != smax) ? 1u : 0u;
  }
  if (lane == 0) { R.group_node[at] = node; R.group_mixed[at] = (uint8_t)mixed; }
}

uint32_t launch_gn_round(hipStream_t st, const Round &R, int what) {
  if (what == 0 && R.nclasses) { hipLaunchKernelGGL(gn_consistency, dim3(R.nclasses), dim3(256), 0, st, R); return 1; }
  if (what == 1 && R.npairs) { hipLaunchKernelGGL(gn_flags, dim3((R.npairs + 255) / 256), dim3(256), 0, st, R); return 1; }
  if (what == 2 && R.ngroups) { hipLaunchKernelGGL(gn_conspecific, dim3((R.ngroups + 3) / 4), dim3(256), 0, st, R); return 1; }
  return 0;
}

}  // namespace ckm
