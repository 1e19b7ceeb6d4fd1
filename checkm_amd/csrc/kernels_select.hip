// kernels_select.hip -- the marker-set selection's draws on the device (scripts/simInferBestMarkerSet.py of the reference, :94-110: per
// replicate two random.uniform, MarkerSetBuilder.sampleGenome, then containedMarkerGenes and MarkerSet.genomeCheck for every set of the
// chain).  gfx950 only.  The layout, the generator and the draw are select_dev.h, shared with the host executor of the CPU tests; the
// float operations are IEEE double in the reference's order (the library's -ffp-contract=off -fno-fast-math).
//
//   select_kernel   a block of four wavefronts per draw (genome, replicate); one launch covers the draws of a round.
//                   1. Every lane forms the draw's plan (one Philox call: nComp, nCont, trueComp, trueCont).
//                   2. Contig i's word goes to sMult[i].  The nComp-th smallest pair (w_i, i) is found by counting passes over 8 bits
//                      of the pair, most significant first: a 256-bin histogram in LDS (ds_add_u32), then EVERY wavefront scans the
//                      bins (four per lane, a shuffle scan, a ballot for the bin that holds the rank), so no lane works alone and no
//                      broadcast is needed.  The two passes over the contig index run only where the threshold word is shared.
//                   3. sMult[i] becomes 1 or 0; the contamination draws add to it with ds_add_u32 (integer sums: any order).
//                   4. A lane owns a marker and adds sMult[p / contigLen] over its copies: no search.  The U counts stay in LDS
//                      (STAGE_COUNTS of them; more go to the block's scratch row in global memory), then score_sets of sim_score.h.
//                   No atomics on global memory; every output word has one writer.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "select_dev.h"
#include "sim_score.h"

namespace ckm {
using namespace sel;

// The bin that holds rank k (1-based) of the histogram: every lane of every wavefront returns the same.  before: entries in lower bins.
__device__ __forceinline__ uint32_t bin_of_rank(const uint32_t *hist, uint32_t k, uint32_t &before, uint32_t &inside) {
  const int lane = threadIdx.x & (WAVE - 1);
  static_assert(BINS == 4 * WAVE, "four bins per lane");
  const uint32_t h0 = hist[4 * lane], h1 = hist[4 * lane + 1], h2 = hist[4 * lane + 2], h3 = hist[4 * lane + 3];
  const uint32_t mine = h0 + h1 + h2 + h3;
  uint32_t incl = mine;
#pragma unroll
  for (int d = 1; d < WAVE; d <<= 1) {
    const uint32_t up = __shfl_up(incl, d, WAVE);
    if (lane >= d) incl += up;
  }
  const uint32_t excl = incl - mine;
  const unsigned long long owner = __ballot(excl < k && k <= incl);
  const int src = owner ? __ffsll((long long)owner) - 1 : 0;      // 1 <= k <= entries: exactly one lane
  uint32_t b = 4 * lane, lo = excl, in = h0;
  if (k > lo + h0) { lo += h0; b += 1; in = h1;
    if (k > lo + h1) { lo += h1; b += 1; in = h2;
      if (k > lo + h2) { lo += h2; b += 1; in = h3; } } }
  before = __shfl(lo, src, WAVE);
  inside = __shfl(in, src, WAVE);
  return __shfl(b, src, WAVE);
}

// draw d0 + blockIdx.x of the call; truth [blocks][2]; out [blocks][S][4]; scratch [blocks][U] only when U > STAGE_COUNTS; rows (or NULL)
// holds the round's multiplicity rows, the first of them being entry row_base of the call's
__global__ __launch_bounds__(THREADS) void select_kernel(SelectDev T, uint32_t d0, uint64_t row_base, double *__restrict__ truth, double *__restrict__ out,
                                                          uint32_t *__restrict__ scratch, uint16_t *__restrict__ rows) {
  extern __shared__ __attribute__((aligned(16))) uint32_t sMult[];      // [the call's largest C]
  __shared__ uint32_t sCounts[STAGE_COUNTS];
  __shared__ uint32_t sHist[BINS];
  const uint32_t d = d0 + blockIdx.x, g = d / T.R, r = d % T.R;
  const uint32_t C = T.ncontigs[g];
  const Plan plan = plan_of(T.P, T.genome_len[g], C, g, r);

  // the completeness words
  for (uint32_t q = threadIdx.x; q < (C + 3) / 4; q += THREADS) {
    const Words w = words_of(T.P.seed, STREAM_COMP, g, r, q);
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k)
      if (4 * q + k < C) sMult[4 * q + k] = w.w[k];
  }
  // the threshold pair: the nComp-th smallest
  uint64_t threshold = 0;
  bool any = plan.ncomp > 0;
  if (any) {
    uint32_t k = plan.ncomp;
    for (int p = 0; p < PASSES; ++p) {
      const int shift = pass_shift(p);
      const uint64_t above = pass_above(p);
      for (uint32_t b = threadIdx.x; b < BINS; b += THREADS) sHist[b] = 0;
      __syncthreads();                                          // the words (first pass), the cleared bins
      for (uint32_t i = threadIdx.x; i < C; i += THREADS) {
        const uint64_t pair = pair_of(sMult[i], i);
        if ((pair & above) == threshold) atomicAdd(&sHist[(uint32_t)(pair >> shift) & (BINS - 1)], 1u);
      }
      __syncthreads();
      uint32_t before, inside;
      const uint32_t b = bin_of_rank(sHist, k, before, inside);
      __syncthreads();                                          // every wavefront has read the bins
      threshold |= (uint64_t)b << shift;
      k -= before;
      if (p == 3 && inside == 1) { threshold |= 0xffffffffull; break; }      // one contig has this word: its index decides nothing
    }
  } else {
    __syncthreads();
  }
  for (uint32_t i = threadIdx.x; i < C; i += THREADS) sMult[i] = any && pair_of(sMult[i], i) <= threshold ? 1u : 0u;
  __syncthreads();
  // the contamination draws
  for (uint32_t q = threadIdx.x; q < (plan.ncont + 3) / 4; q += THREADS) {
    const Words w = words_of(T.P.seed, STREAM_CONT, g, r, q);
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k)
      if (4 * q + k < plan.ncont) atomicAdd(&sMult[landing(w.w[k], C)], 1u);
  }
  __syncthreads();
  if (rows) {
    uint16_t *row = rows + (T.row_off[g] + (uint64_t)r * C - row_base);
    for (uint32_t i = threadIdx.x; i < C; i += THREADS) row[i] = row_entry(sMult[i]);
  }
  // the marker counts
  uint32_t *counts = T.U <= STAGE_COUNTS ? sCounts : scratch + (uint64_t)blockIdx.x * T.U;
  const uint32_t *koff = T.key_off + (uint64_t)g * T.U;
  for (uint32_t m = threadIdx.x; m < T.U; m += THREADS) counts[m] = marker_mult(T.key, koff[m], koff[m + 1], sMult, C, T.P.contig_len);
  __syncthreads();                                              // the counts, in LDS or in the block's own scratch row

  if (threadIdx.x == 0) { truth[(uint64_t)blockIdx.x * 2] = plan.true_comp; truth[(uint64_t)blockIdx.x * 2 + 1] = plan.true_cont; }
  sim::score_sets(T.sets, counts, out + (uint64_t)blockIdx.x * T.sets.S * 4);
}

void launch_select(hipStream_t st, const SelectDev &T, uint32_t max_contigs, uint32_t d0, uint32_t nd, uint64_t row_base, double *truth, double *out, uint32_t *scratch,
                   uint16_t *rows) {
  if (!nd) return;
  const size_t bytes = (size_t)max_contigs * 4;
  if (bytes > 32768) (void)hipFuncSetAttribute((const void *)select_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  hipLaunchKernelGGL(select_kernel, dim3(nd), dim3(THREADS), bytes, st, T, d0, row_base, truth, out, scratch, rows);
}

}  // namespace ckm
