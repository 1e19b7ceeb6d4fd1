// kernels_gtree.hip -- the genome tree on the device (what inferGenomeTree.py and bootstrapTree.py of the reference's
// scripts/genometreeworkflow ask of FastTree): pair counts over the rows of an alignment, corrected distances, neighbour joining.
// gfx950 only.  The layout and the arithmetic are gtree_dev.h, shared with the host executor of the CPU tests; the float operations are
// IEEE double in the header's order (the library's -ffp-contract=off -fno-fast-math).  Every launch covers the trees of a batch
// (blockIdx.y, or the outer index of a flat grid); every output word has one writer; no atomics, no waiting between blocks.
//
//   gt_encode   a thread per byte of the padded encoded alignment: 0x80 | class, or 0.
//   gt_gather   a thread per byte of a replicate's encoded alignment: column cols[r][c] of the call's.
//   gt_counts   a workgroup of 256 per pair of 64-row tiles bi <= bj.  CHUNK bytes of the 128 rows go to LDS (rows 8 bytes apart from
//               a multiple of the chunk, so that the sixteen rows a wavefront reads fall into different banks); a thread owns 4 x 4 pairs
//               and takes eight columns of a pair with pair_word and two population counts.  Rows past N are read as unknown.
//   gt_dist     a thread per matrix entry: dist_of.
//   gt_rsum     a workgroup per slot: R at the start, by sum256.
//   gt_rowmin   a wavefront per list position a < n - 1: the best partner b > a, lanes striding b in ascending order, then a butterfly.
//   gt_join     a workgroup per tree: the best position, the merge row, then thread t takes the new list's positions t, t + 256, ...:
//               the new distance, R of that slot, the new list, and its lane's share of the new row's R; the fold of sum256 in LDS.
//   gt_close    a thread per tree: the last two rows.
// The join loop is a chain of gt_rowmin / gt_join launches on the call's stream: the host knows n of every round without looking.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "gtree_dev.h"
#include "wave_const.h"

namespace ckm {
using namespace gtree;

__global__ __launch_bounds__(256) void gt_encode(const uint8_t *__restrict__ text, uint32_t N, uint32_t L, uint32_t Lp, uint8_t *__restrict__ enc) {
  const uint64_t at = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (at >= (uint64_t)N * Lp) return;
  const uint32_t i = (uint32_t)(at / Lp), c = (uint32_t)(at % Lp);
  enc[at] = c < L ? encode(text[(uint64_t)i * L + c]) : (uint8_t)0;
}

// replicate blockIdx.y of the batch: cols [trees][L], out [trees][N * Lp]
__global__ __launch_bounds__(256) void gt_gather(const uint8_t *__restrict__ enc, const uint32_t *__restrict__ cols, uint32_t N, uint32_t L, uint32_t Lp, uint8_t *__restrict__ out) {
  const uint64_t at = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (at >= (uint64_t)N * Lp) return;
  const uint32_t i = (uint32_t)(at / Lp), c = (uint32_t)(at % Lp);
  const uint32_t *col = cols + (uint64_t)blockIdx.y * L;
  out[(uint64_t)blockIdx.y * N * Lp + at] = c < L ? enc[(uint64_t)i * Lp + col[c]] : (uint8_t)0;
}

constexpr int ROW_WORDS = CHUNK / 8 + 1;      // 17 words: a row's chunk and 8 bytes of padding

// enc [trees][N * Lp] (tree_stride 0: one alignment for every tree); cmp, dif [trees][N * N]
__global__ __launch_bounds__(256) void gt_counts(const uint8_t *__restrict__ enc, uint64_t tree_stride, uint32_t N, uint32_t Lp, uint32_t ntiles, uint32_t *__restrict__ cmp,
                                                 uint32_t *__restrict__ dif) {
  __shared__ uint64_t sa[TILE * ROW_WORDS], sb[TILE * ROW_WORDS];
  uint32_t p = blockIdx.x, bi = 0;
  while (p >= ntiles - bi) { p -= ntiles - bi; ++bi; }
  const uint32_t bj = bi + p;
  const uint8_t *e = enc + (uint64_t)blockIdx.y * tree_stride;
  const uint32_t tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  uint32_t c[4][4] = {}, d[4][4] = {};
  for (uint32_t k0 = 0; k0 < Lp; k0 += CHUNK) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t idx = threadIdx.x + 256u * q, row = idx >> 4, w = idx & 15;
      const uint32_t ra = bi * TILE + row, rb = bj * TILE + row, col = k0 + w * 8;
      uint64_t va = 0, vb = 0;
      if (col < Lp) {                              // (Lp is a multiple of 16: a word lies inside the row or past it)
        if (ra < N) va = *reinterpret_cast<const uint64_t *>(e + (uint64_t)ra * Lp + col);
        if (rb < N) vb = *reinterpret_cast<const uint64_t *>(e + (uint64_t)rb * Lp + col);
      }
      sa[row * ROW_WORDS + w] = va;
      sb[row * ROW_WORDS + w] = vb;
    }
    __syncthreads();
#pragma unroll 4
    for (int w = 0; w < CHUNK / 8; ++w) {
      uint64_t a[4], b[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) { a[r] = sa[(ty + 16 * r) * ROW_WORDS + w]; b[r] = sb[(tx + 16 * r) * ROW_WORDS + w]; }
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          uint64_t both, diff;
          pair_word(a[r], b[s], both, diff);
          c[r][s] += pop64(both);
          d[r][s] += pop64(diff);
        }
    }
    __syncthreads();
  }
  uint32_t *oc = cmp + (uint64_t)blockIdx.y * N * N, *od = dif + (uint64_t)blockIdx.y * N * N;
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const uint32_t i = bi * TILE + ty + 16 * r, j = bj * TILE + tx + 16 * s;
      if (i >= N || j >= N) continue;
      oc[(uint64_t)i * N + j] = c[r][s]; od[(uint64_t)i * N + j] = d[r][s];
      if (bi != bj) { oc[(uint64_t)j * N + i] = c[r][s]; od[(uint64_t)j * N + i] = d[r][s]; }
    }
}

// n_entries = trees * N * N
__global__ __launch_bounds__(256) void gt_dist(const uint32_t *__restrict__ cmp, const uint32_t *__restrict__ dif, uint32_t N, uint64_t n_entries, int model, double max_dist,
                                               double *__restrict__ D) {
  const uint64_t at = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (at >= n_entries) return;
  const uint64_t in_tree = at % ((uint64_t)N * N);
  const uint32_t i = (uint32_t)(in_tree / N), j = (uint32_t)(in_tree % N);
  D[at] = i == j ? 0.0 : dist_of(cmp[at], dif[at], model, max_dist);
}

// the fold of sum256 over the 256 lanes' sums; every thread returns the total
__device__ __forceinline__ double fold256(double mine, double *lane) {
  lane[threadIdx.x] = mine;
  __syncthreads();
#pragma unroll
  for (int s = SUM_LANES / 2; s >= 1; s >>= 1) {
    if ((int)threadIdx.x < s) lane[threadIdx.x] = lane[threadIdx.x] + lane[threadIdx.x + s];
    __syncthreads();
  }
  const double total = lane[0];
  __syncthreads();
  return total;
}

// slot blockIdx.x of tree blockIdx.y: R, and the first list
__global__ __launch_bounds__(SUM_LANES) void gt_rsum(const double *__restrict__ D, uint32_t N, double *__restrict__ R, uint32_t *__restrict__ list) {
  __shared__ double lane[SUM_LANES];
  const uint32_t i = blockIdx.x;
  const double *row = D + ((uint64_t)blockIdx.y * N + i) * N;
  double s = 0.0;
  for (uint32_t c = threadIdx.x; c < N; c += SUM_LANES) s = s + (c == i ? 0.0 : row[c]);
  const double total = fold256(s, lane);
  if (threadIdx.x == 0) { R[(uint64_t)blockIdx.y * N + i] = total; list[(uint64_t)blockIdx.y * N + i] = i; }
}

// list position a = blockIdx.x of tree blockIdx.y, n active: row_q[a], row_b[a]
__global__ __launch_bounds__(WAVE) void gt_rowmin(const double *__restrict__ D, const double *__restrict__ R, const uint32_t *__restrict__ list, uint32_t N, uint32_t n,
                                                  double *__restrict__ row_q, uint32_t *__restrict__ row_b) {
  const uint64_t t = blockIdx.y;
  const uint32_t a = blockIdx.x;
  const uint32_t *ls = list + t * N;
  const double *r = R + t * N;
  const uint32_t i = ls[a];
  const double *row = D + (t * N + i) * N;
  const double ri = r[i], nm2 = (double)(n - 2);
  double bq = 0.0; uint32_t bb = 0xffffffffu;      // (no partner yet)
  for (uint32_t b = a + 1 + threadIdx.x; b < n; b += WAVE) {
    const uint32_t k = ls[b];
    const double q = q_of(nm2, row[k], ri, r[k]);
    if (bb == 0xffffffffu || before(q, b, bq, bb)) { bq = q; bb = b; }
  }
#pragma unroll
  for (int m = 1; m < WAVE; m <<= 1) {
    const double oq = __shfl_xor(bq, m, WAVE);
    const uint32_t ob = __shfl_xor(bb, m, WAVE);
    if (ob != 0xffffffffu && (bb == 0xffffffffu || before(oq, ob, bq, bb))) { bq = oq; bb = ob; }
  }
  if (threadIdx.x == 0) { row_q[t * N + a] = bq; row_b[t * N + a] = bb; }
}

// tree blockIdx.x, n > 3 active, merge row `row`: list -> next
__global__ __launch_bounds__(SUM_LANES) void gt_join(double *__restrict__ D, double *__restrict__ R, const uint32_t *__restrict__ list, uint32_t *__restrict__ next, uint32_t N, uint32_t n,
                                                     const double *__restrict__ row_q, const uint32_t *__restrict__ row_b, uint32_t row, uint32_t *__restrict__ merge_ij,
                                                     double *__restrict__ merge_len) {
  __shared__ double lane[SUM_LANES];
  __shared__ uint32_t lane_a[SUM_LANES];
  const uint64_t t = blockIdx.x;
  const uint32_t *ls = list + t * N;
  uint32_t *nx = next + t * N;
  double *r = R + t * N, *d = D + t * N * N;
  // the best position: (q, a)
  double bq = 0.0; uint32_t ba = 0xffffffffu;
  for (uint32_t a = threadIdx.x; a + 1 < n; a += SUM_LANES) {
    const double q = row_q[t * N + a];
    if (ba == 0xffffffffu || before(q, a, bq, ba)) { bq = q; ba = a; }
  }
  lane[threadIdx.x] = bq; lane_a[threadIdx.x] = ba;
  __syncthreads();
  for (int s = SUM_LANES / 2; s >= 1; s >>= 1) {
    if ((int)threadIdx.x < s) {
      const double oq = lane[threadIdx.x + s]; const uint32_t oa = lane_a[threadIdx.x + s];
      if (oa != 0xffffffffu && (lane_a[threadIdx.x] == 0xffffffffu || before(oq, oa, lane[threadIdx.x], lane_a[threadIdx.x]))) { lane[threadIdx.x] = oq; lane_a[threadIdx.x] = oa; }
    }
    __syncthreads();
  }
  const uint32_t pa = lane_a[0];
  __syncthreads();                                 // (lane[] is used again below)
  const uint32_t pb = row_b[t * N + pa];
  const uint32_t i = ls[pa], j = ls[pb];
  const double dij = d[(uint64_t)i * N + j];
  if (threadIdx.x == 0) {
    double li, lj;
    join_lengths(dij, r[i], r[j], n, li, lj);
    const uint64_t at = (t * (N - 1) + row) * 2;
    merge_ij[at] = i; merge_ij[at + 1] = j; merge_len[at] = li; merge_len[at + 1] = lj;
  }
  __syncthreads();                                 // r[i] has been read before it is written below
  double s = 0.0;
  for (uint32_t c = threadIdx.x; c + 1 < n; c += SUM_LANES) {
    const uint32_t k = ls[c + (c >= pb ? 1u : 0u)];
    nx[c] = k;
    double term = 0.0;
    if (k != i) {
      const double dik = d[(uint64_t)i * N + k], djk = d[(uint64_t)j * N + k];
      term = new_dist(dik, djk, dij);
      r[k] = update_r(r[k], dik, djk, term);
      d[(uint64_t)i * N + k] = term; d[(uint64_t)k * N + i] = term;
    }
    s = s + term;
  }
  const double total = fold256(s, lane);
  if (threadIdx.x == 0) r[i] = total;
}

// tree blockIdx.x * 64 + threadIdx.x: the last rows, n = 3 or (N = 2) 2 active
__global__ __launch_bounds__(WAVE) void gt_close(const double *__restrict__ D, const uint32_t *__restrict__ list, uint32_t N, uint32_t n, uint32_t trees, uint32_t *__restrict__ merge_ij,
                                                 double *__restrict__ merge_len) {
  const uint64_t t = (uint64_t)blockIdx.x * WAVE + threadIdx.x;
  if (t >= trees) return;
  const uint32_t *ls = list + t * N;
  const double *d = D + t * N * N;
  uint32_t *ij = merge_ij + t * (N - 1) * 2;
  double *len = merge_len + t * (N - 1) * 2;
  if (n == 3) {
    const uint32_t x = ls[0], y = ls[1], z = ls[2], row = N - 3;
    double lx, ly, lz;
    close3(d[(uint64_t)x * N + y], d[(uint64_t)x * N + z], d[(uint64_t)y * N + z], lx, ly, lz);
    ij[row * 2] = x; ij[row * 2 + 1] = y; len[row * 2] = lx; len[row * 2 + 1] = ly;
    ij[row * 2 + 2] = x; ij[row * 2 + 3] = z; len[row * 2 + 2] = lz * 0.5; len[row * 2 + 3] = lz * 0.5;
  } else {
    const uint32_t x = ls[0], y = ls[1];
    const double h = clamp0(d[(uint64_t)x * N + y]) * 0.5;
    ij[0] = x; ij[1] = y; len[0] = h; len[1] = h;
  }
}

// ---- launchers (ckm_gtree.hip) ---------------------------------------------------------------------------------------------------------------
void launch_gt_encode(hipStream_t st, const uint8_t *text, uint32_t N, uint32_t L, uint8_t *enc) {
  const uint32_t Lp = padded(L);
  const uint64_t n = (uint64_t)N * Lp;
  hipLaunchKernelGGL(gt_encode, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, text, N, L, Lp, enc);
}
void launch_gt_gather(hipStream_t st, const uint8_t *enc, const uint32_t *cols, uint32_t N, uint32_t L, uint32_t trees, uint8_t *out) {
  if (!trees) return;
  const uint32_t Lp = padded(L);
  const uint64_t n = (uint64_t)N * Lp;
  hipLaunchKernelGGL(gt_gather, dim3((uint32_t)((n + 255) / 256), trees), dim3(256), 0, st, enc, cols, N, L, Lp, out);
}
void launch_gt_counts(hipStream_t st, const uint8_t *enc, uint64_t tree_stride, uint32_t N, uint32_t L, uint32_t trees, uint32_t *cmp, uint32_t *dif) {
  if (!trees) return;
  const uint32_t nt = (N + TILE - 1) / TILE;
  hipLaunchKernelGGL(gt_counts, dim3(nt * (nt + 1) / 2, trees), dim3(256), 0, st, enc, tree_stride, N, padded(L), nt, cmp, dif);
}
void launch_gt_dist(hipStream_t st, const uint32_t *cmp, const uint32_t *dif, uint32_t N, uint32_t trees, int model, double max_dist, double *D) {
  if (!trees) return;
  const uint64_t n = (uint64_t)trees * N * N;
  hipLaunchKernelGGL(gt_dist, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, cmp, dif, N, n, model, max_dist, D);
}
// the whole join of `trees` matrices; returns the launches made
uint64_t launch_gt_join(hipStream_t st, double *D, uint32_t N, uint32_t trees, double *R, uint32_t *list_a, uint32_t *list_b, double *row_q, uint32_t *row_b, uint32_t *merge_ij,
                        double *merge_len) {
  if (!trees) return 0;
  uint64_t launches = 1;
  hipLaunchKernelGGL(gt_rsum, dim3(N, trees), dim3(SUM_LANES), 0, st, D, N, R, list_a);
  uint32_t *cur = list_a, *nxt = list_b;
  uint32_t row = 0;
  for (uint32_t n = N; n > 3; --n, ++row) {
    hipLaunchKernelGGL(gt_rowmin, dim3(n - 1, trees), dim3(WAVE), 0, st, D, R, cur, N, n, row_q, row_b);
    hipLaunchKernelGGL(gt_join, dim3(trees), dim3(SUM_LANES), 0, st, D, R, cur, nxt, N, n, row_q, row_b, row, merge_ij, merge_len);
    std::swap(cur, nxt);
    launches += 2;
  }
  hipLaunchKernelGGL(gt_close, dim3((trees + WAVE - 1) / WAVE), dim3(WAVE), 0, st, D, cur, N, N >= 3 ? 3u : 2u, trees, merge_ij, merge_len);
  return launches + 1;
}

}  // namespace ckm
