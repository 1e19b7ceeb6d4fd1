// kernels_unbinned.hip -- the selective base count of `checkm unbinned` (checkm/unbinned.py:66-77, checkm/util/seqUtils.py:279-286): of
// every contig Unbinned.run keeps, A, C, G, T+U after upper-casing and the code points; nothing of the others.  gfx950 only.
//
//   unbinned_count_kernel  one wavefront per tile of a kept sequence (four per block), 1 KiB per step, every lane one aligned 128-bit
//                          load.  The per-word logic is ub::lane_counts (unbinned_dev.h), shared with the host executor of the CPU
//                          tests: word-parallel byte compares, one population count per counter and chunk.  The five counters are summed
//                          over the wave once per tile and lanes 0 .. 4 store the tile's row: one writer per row, no atomics.
//   unbinned_sum_kernel    one thread per kept sequence: its tile rows summed into uint64.
// Integers only: the result does not depend on the tile size, the batches or the launch geometry.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "unbinned_dev.h"

namespace ckm {
using namespace ub;

__global__ __launch_bounds__(256) void unbinned_count_kernel(const uint8_t *__restrict__ text, const Tile *__restrict__ tiles, uint32_t ntiles, uint32_t *__restrict__ rows) {
  const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x >> 6;
  const uint32_t t = blockIdx.x * 4 + wv;
  if (t >= ntiles) return;
  const Tile T = tiles[t];
  uint32_t acc[NCOUNT] = {0, 0, 0, 0, 0};
  // a chunk that starts inside the tile ends inside the tile's 16-byte padding, which the batch buffer holds
  for (uint32_t off = (uint32_t)lane * LANE_BYTES; off < T.len; off += WAVE_BYTES) {
    const uint4 v = *reinterpret_cast<const uint4 *>(text + T.start + off);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    const uint32_t rem = T.len - off;
    lane_counts(w, rem >= (uint32_t)LANE_BYTES ? LANE_BYTES : (int)rem, acc);
  }
#pragma unroll
  for (int k = 0; k < NCOUNT; ++k) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) acc[k] += __shfl_xor(acc[k], s);
  }
  uint32_t mine = acc[0];
#pragma unroll
  for (int k = 1; k < NCOUNT; ++k) mine = lane == k ? acc[k] : mine;
  if (lane < NCOUNT) rows[(uint64_t)t * NCOUNT + lane] = mine;
}

__global__ __launch_bounds__(256) void unbinned_sum_kernel(const uint32_t *__restrict__ rows, const uint64_t *__restrict__ first_tile, uint32_t nkept, uint64_t *__restrict__ out) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nkept) return;
  sum_rows(rows, first_tile[k], first_tile[k + 1], out + (uint64_t)k * NCOUNT);
}

void launch_unbinned_count(hipStream_t st, const uint8_t *text, const Tile *tiles, uint32_t ntiles, uint32_t *rows) {
  if (ntiles) hipLaunchKernelGGL(unbinned_count_kernel, dim3((ntiles + 3) / 4), dim3(256), 0, st, text, tiles, ntiles, rows);
}
void launch_unbinned_sum(hipStream_t st, const uint32_t *rows, const uint64_t *first_tile, uint32_t nkept, uint64_t *out) {
  if (nkept) hipLaunchKernelGGL(unbinned_sum_kernel, dim3((nkept + 255) / 256), dim3(256), 0, st, rows, first_tile, nkept, out);
}

}  // namespace ckm
