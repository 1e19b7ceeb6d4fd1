// kernels_nearid.hip -- the near-identity pass on the device (what __nearlyIdentical of the reference's scripts/genometreeworkflow/
// createSmallTree.py asks of a Python loop over all pairs of rows).  gfx950 only.  The layout and the arithmetic are nearid_dev.h, shared
// with the host executor of the CPU tests; integers only.  Every output word has one writer; no atomics, no waiting between blocks.
//
//   ni_tiles    a workgroup of 256 per pair of 64-row tiles bi <= bj of a band of row tiles.  CHUNK columns of the 128 rows go to LDS
//               (gt_counts' arrangement: rows 8 bytes apart from a multiple of the chunk, so that the sixteen rows a wavefront reads fall
//               into different banks), masked to the row length; a thread owns 4 x 4 pairs and takes eight columns of a pair with one
//               XOR, diff_bits and one population count.  After a chunk the workgroup leaves the loop when every pair of the tile that
//               counts has reached its row's limit: the output is a bit, so this is exact.  A wave ballot per (r, s) gathers sixteen
//               columns of four rows; the lane with tx == 0 ors its row's four ballots into the 64-bit word of (row, column tile) and
//               stores it.  Rows and columns past n_rows and, in a diagonal tile, columns j <= i give 0 bits.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "nearid_dev.h"

namespace ckm {
using namespace nearid;

constexpr int NI_ROW_WORDS = CHUNK / 8 + 1;      // 17 words: a row's chunk and 8 bytes of padding

// text [N][stride], limit [N]; near [rows of the band from row tile b0][W]
__global__ __launch_bounds__(256) void ni_tiles(const uint8_t *__restrict__ text, const uint32_t *__restrict__ limit, uint32_t N, uint32_t L, uint32_t stride, uint32_t ntiles,
                                                uint32_t b0, uint32_t W, uint64_t *__restrict__ near) {
  __shared__ uint64_t sa[TILE * NI_ROW_WORDS], sb[TILE * NI_ROW_WORDS];
  uint32_t p = blockIdx.x, bi = b0;
  while (p >= ntiles - bi) { p -= ntiles - bi; ++bi; }
  const uint32_t bj = bi + p;
  const uint32_t tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  uint32_t d[4][4] = {}, lim[4];
  bool counts[4][4];                               // the pair is inside the matrix and above the diagonal
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const uint32_t i = bi * TILE + ty + 16 * r;
    lim[r] = i < N ? limit[i] : 0u;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const uint32_t j = bj * TILE + tx + 16 * s;
      counts[r][s] = i < N && j < N && j > i;
    }
  }
  for (uint32_t k0 = 0; k0 < L; k0 += CHUNK) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t idx = threadIdx.x + 256u * q, row = idx >> 4, w = idx & 15;
      const uint32_t ra = bi * TILE + row, rb = bj * TILE + row, col = k0 + w * 8;
      uint64_t va = 0, vb = 0;
      if (col < L) {                               // (stride is a multiple of 16 and >= L: the word lies inside the row's stride)
        const uint64_t m = word_mask(col, L);
        if (ra < N) va = *reinterpret_cast<const uint64_t *>(text + (uint64_t)ra * stride + col) & m;
        if (rb < N) vb = *reinterpret_cast<const uint64_t *>(text + (uint64_t)rb * stride + col) & m;
      }
      sa[row * NI_ROW_WORDS + w] = va;
      sb[row * NI_ROW_WORDS + w] = vb;
    }
    __syncthreads();
    const uint32_t left = L - k0, nw = left >= CHUNK ? CHUNK / 8 : (left + 7) / 8;
#pragma unroll 4
    for (uint32_t w = 0; w < nw; ++w) {
      uint64_t a[4], b[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) { a[r] = sa[(ty + 16 * r) * NI_ROW_WORDS + w]; b[r] = sb[(tx + 16 * r) * NI_ROW_WORDS + w]; }
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int s = 0; s < 4; ++s) d[r][s] += pop64(diff_bits(a[r] ^ b[s]));
    }
    int settled = 1;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int s = 0; s < 4; ++s) settled &= (!counts[r][s] || d[r][s] >= lim[r]) ? 1 : 0;
    if (__syncthreads_and(settled)) break;         // (the same answer in every thread; also the barrier before the next chunk is staged)
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    uint64_t word = 0;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const uint64_t lanes = __ballot(counts[r][s] && d[r][s] < lim[r]);      // lane = tx + 16 * (ty & 3)
      word |= ((lanes >> (16 * (ty & 3))) & 0xffffull) << (16 * s);
    }
    const uint32_t i = bi * TILE + ty + 16 * r;
    if (tx == 0 && i < N) near[(uint64_t)(i - b0 * TILE) * W + bj] = word;
  }
}

// ---- launcher (ckm_nearid.hip) ---------------------------------------------------------------------------------------------------------------
// the tiles of the row tiles b0 .. b1 against every column tile at or right of them; returns the workgroups launched
uint64_t launch_ni_band(hipStream_t st, const uint8_t *text, const uint32_t *limit, uint32_t N, uint32_t L, uint32_t stride, uint32_t b0, uint32_t b1, uint64_t *near) {
  const uint32_t nt = tiles_of(N);
  uint64_t blocks = 0;
  for (uint32_t b = b0; b < b1; ++b) blocks += nt - b;
  if (!blocks) return 0;
  hipLaunchKernelGGL(ni_tiles, dim3((uint32_t)blocks), dim3(256), 0, st, text, limit, N, L, stride, nt, b0, words_of(N), near);
  return blocks;
}

}  // namespace ckm
