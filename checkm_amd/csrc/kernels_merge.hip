// kernels_merge.hip -- the all-pairs comparison of `checkm merge` (checkm/merger.py:64-106).  gfx950 only.  The arithmetic is merge_dev.h,
// shared with the host executor of the CPU tests; every result is float64 and equals the reference's bit for bit (the library's
// -ffp-contract=off -fno-fast-math: nothing here may be fused or replaced by a reciprocal).
//
// A bin is a row of member bits over the common marker genes (nwords 64-bit words, a run-time value) and three numbers.  The pairs
// (i, j), i < j, are cut into tiles of 64 rows x 64 columns; a tile below the diagonal exits at once.
//
//   merge_bins_kernel   a thread per bin: popcount of its row, completeness and contamination of the bin by itself.
//   merge_tile_kernel   a block of four wavefronts per tile, a lane per column j.  The rows of both sides are staged in LDS sixteen words
//                       at a time (the J side transposed: lane j reads word k at [k][j], no bank conflict; the I side is read by a whole
//                       wavefront at one address: a broadcast) and reused by the sixteen rows a wavefront walks; the union counts of
//                       those sixteen rows live in registers.  Then a row at a time: the two tests of the reference, a 64-bit ballot,
//                       and the count or the fill step of pairs_wave.h (count_store; lanes_below and pair_slot): the output is in (i, j) order and no atomic decides a position.
//   merge_scan_kernel   a wavefront per row: pc::row_scan over the row's tile counts (tiles left of the diagonal count as nothing and
//                       are never read), the row's total out.  The prefix over the rows is the host's (it needs the totals to cut the
//                       output into batches).
#include <hip/hip_runtime.h>
#include <cstdint>
#include "merge_dev.h"
#include "pairs_wave.h"

namespace ckm {
using namespace mg;

__global__ __launch_bounds__(256) void merge_bins_kernel(MergeBins B) {
  const uint32_t b = blockIdx.x * 256u + threadIdx.x;
  if (b >= B.nbins) return;
  const uint64_t *row = B.bits + (uint64_t)b * B.nwords;
  int32_t members = 0;
  for (uint32_t k = 0; k < B.nwords; ++k) members += popc64(row[k]);
  double comp, cont;
  bin_stats(members, B.hit_sum[b], B.n_markers[b], comp, cont);
  B.comp[b] = comp; B.cont[b] = cont;
}

template <bool FILL>
__global__ __launch_bounds__(256) void merge_tile_kernel(MergeBins B, Thresholds thr, uint32_t row_lo, uint32_t row_hi, uint32_t tile_i0, uint32_t ntiles_j,
                                                          uint32_t count_row0, uint32_t *__restrict__ tile_count, MergeOut out) {
  const uint32_t tj = blockIdx.x, ti = tile_i0 + blockIdx.y;
  if (tj < ti) return;                                         // wholly below the diagonal
  __shared__ uint64_t sJ[WORD_CHUNK * TILE_J], sI[TILE_I * WORD_CHUNK];
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
  const uint32_t i0 = ti * TILE_I, j0 = tj * TILE_J;
  int32_t u[ROWS_PER_WAVE];
#pragma unroll
  for (int r = 0; r < ROWS_PER_WAVE; ++r) u[r] = 0;
  for (uint32_t w0 = 0; w0 < B.nwords; w0 += WORD_CHUNK) {
    const uint32_t wc = B.nwords - w0 < (uint32_t)WORD_CHUNK ? B.nwords - w0 : (uint32_t)WORD_CHUNK;
    __syncthreads();                                           // the readers of the chunk before
    for (uint32_t x = threadIdx.x; x < (uint32_t)TILE_J * wc; x += 256u) {
      const uint32_t r = x / wc, k = x % wc;
      sJ[k * TILE_J + r] = j0 + r < B.nbins ? B.bits[(uint64_t)(j0 + r) * B.nwords + w0 + k] : 0;
      sI[r * WORD_CHUNK + k] = i0 + r < B.nbins ? B.bits[(uint64_t)(i0 + r) * B.nwords + w0 + k] : 0;
    }
    __syncthreads();
    for (uint32_t k = 0; k < wc; ++k) {
      const uint64_t bj = sJ[k * TILE_J + lane];
#pragma unroll
      for (int r = 0; r < ROWS_PER_WAVE; ++r) u[r] += union_word(sI[(wave * ROWS_PER_WAVE + r) * WORD_CHUNK + k], bj);
    }
  }
  const uint32_t j = j0 + lane;
  const bool jv = j < B.nbins;
  BinSide J = {0, 1, 0.0, 0.0};
  if (jv) J = BinSide{B.hit_sum[j], B.n_markers[j], B.comp[j], B.cont[j]};
#pragma unroll
  for (int r = 0; r < ROWS_PER_WAVE; ++r) {
    const uint32_t i = i0 + (uint32_t)(wave * ROWS_PER_WAVE + r);            // the same for every lane of the wavefront
    if (i < row_lo || i >= row_hi || i >= B.nbins) continue;
    const BinSide I = {B.hit_sum[i], B.n_markers[i], B.comp[i], B.cont[i]};
    PairCols pc;
    const bool keep = jv && j > i && pair_eval(u[r], I, J, thr, pc);
    const uint64_t ballot = __ballot(keep);
    const uint64_t at = (uint64_t)(i - count_row0) * ntiles_j + tj;
    if (!FILL) {
      pc::count_store(ballot, lane, tile_count, at);
    } else if (keep) {
      const int below = pc::lanes_below(ballot);
      const uint64_t slot = pair_slot(out.row_base[i - count_row0], tile_count[at], below, out.batch_base);
      if (slot < out.cap) {
        out.pi[slot] = i; out.pj[slot] = j;
#pragma unroll
        for (int c = 0; c < NCOL; ++c) out.cols[(uint64_t)c * out.cap + slot] = pc.v[c];
      }
    }
  }
}

__global__ __launch_bounds__(256) void merge_scan_kernel(uint32_t row0, uint32_t nrows, uint32_t ntiles_j, uint32_t *__restrict__ tile_count, uint32_t *__restrict__ row_total) {
  const int lane = threadIdx.x & (WAVE - 1);
  const uint32_t k = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (k >= nrows) return;
  const uint32_t total = pc::row_scan(tile_count + (uint64_t)k * ntiles_j, 1u, (row0 + k) / (uint32_t)TILE_I, ntiles_j, lane);
  if (lane == 0) row_total[k] = total;
}

void launch_merge_bins(hipStream_t st, const MergeBins &B) {
  if (B.nbins) hipLaunchKernelGGL(merge_bins_kernel, dim3((B.nbins + 255) / 256), dim3(256), 0, st, B);
}
// rows [row_lo, row_hi) of the count pass that starts at row count_row0 (a multiple of TILE_I)
void launch_merge_tiles(hipStream_t st, bool fill, const MergeBins &B, const Thresholds &thr, uint32_t row_lo, uint32_t row_hi, uint32_t count_row0,
                        uint32_t *tile_count, const MergeOut &out) {
  if (row_lo >= row_hi) return;
  const uint32_t ntj = (B.nbins + TILE_J - 1) / TILE_J, t0 = row_lo / TILE_I, t1 = (row_hi - 1) / TILE_I + 1;
  const dim3 grid(ntj, t1 - t0);
  if (fill) hipLaunchKernelGGL(merge_tile_kernel<true>, grid, dim3(256), 0, st, B, thr, row_lo, row_hi, t0, ntj, count_row0, tile_count, out);
  else hipLaunchKernelGGL(merge_tile_kernel<false>, grid, dim3(256), 0, st, B, thr, row_lo, row_hi, t0, ntj, count_row0, tile_count, out);
}
void launch_merge_scan(hipStream_t st, uint32_t row0, uint32_t nrows, uint32_t ntiles_j, uint32_t *tile_count, uint32_t *row_total) {
  if (nrows) hipLaunchKernelGGL(merge_scan_kernel, dim3((nrows + 3) / 4), dim3(256), 0, st, row0, nrows, ntiles_j, tile_count, row_total);
}

}  // namespace ckm
