// kernels_refdist.hip -- counts of randomly placed, overlapping windows of a genome scaffold from prefix counts at block checkpoints:
// the sampling behind CheckM's gc_dist, cd_dist and td_dist tables.  gfx950 only.  The geometry is rd::block_piece /
// rd::window_geom (refdist_dev.h), the per-byte logic sw::lane_step (seqwin_dev.h), both shared with the host executor of the CPU tests.
// The distance of a TD window to the genome's signature is seqwin_td_kernel (kernels_seqwin.hip) run on the count rows written here.
//
//   refdist_block_kernel   a wavefront per block of the scaffold (four per workgroup).  The wave walks 16-byte-ALIGNED spans from the
//                          chunk that holds the block's first byte (a block starts at any byte: `block` need not be a multiple of 16):
//                          one aligned 128-bit load per lane, the bytes outside the block masked, the three bytes a 4-mer needs behind
//                          a chunk taken from the next lane's word.  A 4-mer belongs to the block where it STARTS.  GC / CD: two
//                          counters summed over the wave; TD: a histogram of the wave's own in LDS.  The block's row is a plain store.
//   refdist_scan_kernel    a wavefront per column: pc::row_scan (pairs_wave.h) down the column, an exclusive scan over the blocks;
//                          row nblocks receives the totals of the scaffold.
//   refdist_window_kernel  a wavefront per window: P[b1] - P[b0] over its whole blocks plus its edges (fewer than two blocks of text),
//                          read as the block kernel reads a block.  GC / CD: two uint32 per window; TD: the window's 136 counts.
// No global atomics anywhere: every row has one writer.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "pairs_wave.h"
#include "refdist_dev.h"
#include "tetra_wave.h"

namespace ckm {
using namespace sw;

__global__ __launch_bounds__(256) void refdist_block_kernel(const uint8_t *__restrict__ text, uint64_t L, uint32_t block, uint32_t nblocks, int td,
                                                             const uint8_t *__restrict__ canon, uint32_t *__restrict__ rows) {
  __shared__ uint32_t hist[4][NKMER];
  __shared__ uint8_t lcanon[256];
  const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x >> 6;
  const uint32_t b = blockIdx.x * 4 + wv;
  if (td) hist_stage(canon, lcanon, hist[wv], lane);        // GC / CD count no 4-mers: nothing to stage
  __syncthreads();
  const bool active = b < nblocks;
  uint32_t acc[4] = {0, 0, 0, 0};
  if (active) wave_piece(text, rd::block_piece(b, block, L), lane, td != 0, lcanon, hist[wv], acc);
  __syncthreads();
  if (!active) return;
  if (td) {
    uint32_t *row = rows + (uint64_t)b * NKMER;
    hist_flush(lane, [=](int k) { row[k] = hist[wv][k]; });
  } else {
    const uint32_t gc = wave_sum(acc[1] + acc[2]), at = wave_sum(acc[0] + acc[3]);
    if (lane == 0) { rows[(uint64_t)b * 2] = gc; rows[(uint64_t)b * 2 + 1] = at; }
  }
}

// rows [nblocks + 1][ncol]: rows 0 .. nblocks - 1 hold the blocks' counts going in, their exclusive prefix going out; row nblocks the totals
__global__ __launch_bounds__(256) void refdist_scan_kernel(uint32_t *__restrict__ rows, uint32_t nblocks, uint32_t ncol) {
  const int lane = threadIdx.x & (WAVE - 1);
  const uint32_t col = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (col >= ncol) return;
  const uint32_t total = pc::row_scan(rows + col, ncol, 0u, nblocks, lane);      // at most the scaffold's length, below 2^31
  if (lane == 0) rows[(uint64_t)nblocks * ncol + col] = total;
}

// windows win0 .. win0 + nwin - 1 of the call; tet holds the rows of this launch only (row 0 = window win0)
__global__ __launch_bounds__(256) void refdist_window_kernel(const uint8_t *__restrict__ text, uint32_t block, int stat, const uint32_t *__restrict__ starts,
                                                              const uint32_t *__restrict__ sizes, uint64_t win0, uint32_t nwin, const uint8_t *__restrict__ canon,
                                                              const uint32_t *__restrict__ rows, uint32_t *__restrict__ cnt, uint32_t *__restrict__ tet) {
  __shared__ uint32_t hist[4][NKMER];
  __shared__ uint8_t lcanon[256];
  const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x >> 6;
  const uint32_t x = blockIdx.x * 4 + wv;
  const bool active = x < nwin, td = stat == rd::STAT_TD;
  if (td) hist_stage(canon, lcanon, hist[wv], lane);
  __syncthreads();
  uint32_t acc[4] = {0, 0, 0, 0};
  rd::WindowGeom g = {};
  if (active) {
    g = rd::window_geom(starts[win0 + x], sizes[win0 + x], stat, block);
    wave_piece(text, g.edge[0], lane, td, lcanon, hist[wv], acc);
    wave_piece(text, g.edge[1], lane, td, lcanon, hist[wv], acc);
  }
  __syncthreads();
  if (!active) return;
  if (td) {
    const uint32_t *p0 = rows + g.b0 * NKMER, *p1 = rows + g.b1 * NKMER;
    uint32_t *row = tet + (uint64_t)x * NKMER;
    hist_flush(lane, [=](int k) { row[k] = hist[wv][k] + (g.whole ? p1[k] - p0[k] : 0u); });
  } else {
    uint32_t gc = wave_sum(acc[1] + acc[2]), at = wave_sum(acc[0] + acc[3]);
    if (lane == 0) {
      if (g.whole) { gc += rows[g.b1 * 2] - rows[g.b0 * 2]; at += rows[g.b1 * 2 + 1] - rows[g.b0 * 2 + 1]; }
      cnt[(win0 + x) * 2] = gc; cnt[(win0 + x) * 2 + 1] = at;
    }
  }
}

void launch_refdist_blocks(hipStream_t st, const uint8_t *text, uint64_t L, uint32_t block, uint32_t nblocks, int td, const uint8_t *canon, uint32_t *rows) {
  if (nblocks) hipLaunchKernelGGL(refdist_block_kernel, dim3((nblocks + 3) / 4), dim3(256), 0, st, text, L, block, nblocks, td, canon, rows);
}
void launch_refdist_scan(hipStream_t st, uint32_t *rows, uint32_t nblocks, uint32_t ncol) {
  hipLaunchKernelGGL(refdist_scan_kernel, dim3((ncol + 3) / 4), dim3(256), 0, st, rows, nblocks, ncol);
}
void launch_refdist_windows(hipStream_t st, const uint8_t *text, uint32_t block, int stat, const uint32_t *starts, const uint32_t *sizes, uint64_t win0, uint32_t nwin,
                            const uint8_t *canon, const uint32_t *rows, uint32_t *cnt, uint32_t *tet) {
  if (nwin) hipLaunchKernelGGL(refdist_window_kernel, dim3((nwin + 3) / 4), dim3(256), 0, st, text, block, stat, starts, sizes, win0, nwin, canon, rows, cnt, tet);
}

}  // namespace ckm
