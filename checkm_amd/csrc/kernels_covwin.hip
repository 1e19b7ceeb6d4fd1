// kernels_covwin.hip -- the device pass of CoverageWindows (`checkm gc_bias_plot`) over a batch of BAM records, and the scan that turns
// its accumulators into window sums.  gfx950 only.  What a record is, the chain and the scatter: covwin_dev.h, shared with the host
// executor of the CPU tests.
//
//   covwin_kernel      a lane per record, the mapping of coverage_kernel.  The nine per-reference counters (reads, classes 1..7 by THIS
//                      chain, the numerator = bases covered after clipping to the reference) are reduced over runs of equal refID
//                      inside the wavefront as there.  A mapped read then costs O(1) memory operations whatever alen / w is: the bases
//                      in its first window go to direct[k0], combined over runs of equal global slot inside the wavefront (a sorted
//                      BAM puts neighbouring reads into the same window: run-head ballot, segmented shuffle sum, the head issues one
//                      atomic); the three rarer adds -- direct[k1], +w at diff[k0 + 1], -w at diff[k1] -- are plain 64-bit atomics.
//                      Integer sums: neither the order of the records nor the batches change a value.
//   covwin_block_sums  \  sum[k] = direct[k] + inclusive_prefix(diff)[k] over ALL slots (every reference's diff nets to zero), in three
//   covwin_scan_sums    > passes: the diff total of each workgroup's SCAN_BLOCK slots; an exclusive scan of those totals by one
//   covwin_add         /  workgroup that carries across its tiles; the workgroup scan plus its carry, written over `direct`.
// Nothing here has been measured; nothing more elaborate is built until it has.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "covwin_dev.h"
#include "pairs_wave.h"

namespace ckm {
using namespace cw;

// the first lane of the next run, for a lane of a run whose heads are `heads`
__device__ __forceinline__ int run_end(uint64_t heads, int lane) {
  const uint64_t above = lane == WAVE - 1 ? 0 : heads & ~(((uint64_t)2 << lane) - 1);
  return above ? __ffsll((unsigned long long)above) - 1 : WAVE;
}

// sum of v over the lanes [lane, end) of the lane's run
__device__ __forceinline__ long long run_sum(long long v, int lane, int end) {
#pragma unroll
  for (int d = 1; d < WAVE; d <<= 1) {
    const long long up = __shfl_down(v, d, WAVE);
    if (lane + d < end) v += up;
  }
  return v;
}

__global__ __launch_bounds__(256) void covwin_kernel(const uint8_t *__restrict__ data, const uint32_t *__restrict__ offsets, uint32_t nrec, uint64_t first_ordinal, Params P,
                                                      const int64_t *__restrict__ ref_len, const int64_t *__restrict__ ref_first, unsigned long long *__restrict__ counters,
                                                      unsigned long long *__restrict__ direct, unsigned long long *__restrict__ diff, unsigned long long *__restrict__ err_slot) {
  const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
  const int lane = threadIdx.x & (WAVE - 1);
  RecOut o = {-1, -1, 0, 0, 0};
  if (idx < nrec) {                                            // (no early return: every lane takes part in the ballots below)
    classify(data + offsets[idx], P, o);
    if (o.err) { atomicMin(err_slot, (unsigned long long)((first_ordinal + idx) * 8u + o.err)); o.ref = -1; }
  }
  const int32_t ref = o.ref;
  const bool counted = ref >= 0;
  Scatter sc = {0, 0, 0, 0, 0};
  uint32_t g0 = NO_SLOT;                                       // the global slot of the read's first window
  if (counted && o.cls == 7) {
    sc = scatter(o.pos, o.alen, ref_len[ref], P.window);
    if (sc.span) g0 = (uint32_t)ref_first[ref] + sc.k0;
  }
  // the nine counters over runs of equal refID
  {
    const int32_t below = __shfl_up(ref, 1, WAVE);
    const bool head = lane == 0 || below != ref;
    const int end = run_end(__ballot(head), lane);
    const uint64_t run = (end == WAVE ? ~(uint64_t)0 : (((uint64_t)1 << end) - 1)) & ~(((uint64_t)1 << lane) - 1);
    unsigned long long add[NSLOT];
    add[SLOT_READS] = (unsigned long long)__popcll(__ballot(counted) & run);
#pragma unroll
    for (int c = 1; c < NCLASS; ++c) add[c] = (unsigned long long)__popcll(__ballot(counted && o.cls == c) & run);
    add[SLOT_NUMER] = (unsigned long long)run_sum((long long)sc.span, lane, end);
    if (head && counted) {
      unsigned long long *row = counters + (uint64_t)ref * NSLOT;
#pragma unroll
      for (int k = 0; k < NSLOT; ++k) if (add[k]) atomicAdd(row + k, add[k]);
    }
  }
  // direct[k0] over runs of equal global slot
  {
    const uint32_t below = __shfl_up(g0, 1, WAVE);
    const bool head = lane == 0 || below != g0;
    const int end = run_end(__ballot(head), lane);
    const long long sum = run_sum((long long)sc.head, lane, end);          // (sc.head is 0 where g0 is NO_SLOT)
    if (head && g0 != NO_SLOT) atomicAdd(direct + g0, (unsigned long long)sum);
  }
  if (g0 != NO_SLOT && sc.k1 > sc.k0) {                        // k1 <= (L - 1) / w: g1 is a slot of this reference
    const uint32_t g1 = g0 + (sc.k1 - sc.k0);
    atomicAdd(direct + g1, (unsigned long long)sc.tail);
    if (sc.k1 > sc.k0 + 1) {
      atomicAdd(diff + g0 + 1, (unsigned long long)P.window);
      atomicAdd(diff + g1, (unsigned long long)(-(long long)P.window));
    }
  }
}

// inclusive scan of v over the workgroup's SCAN_THREADS threads; *total = the workgroup's sum.  lds: SCAN_THREADS / WAVE values.
__device__ __forceinline__ long long block_scan(long long v, long long *lds, long long *total) {
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  v = wave_inclusive(v, lane);
  __syncthreads();                                             // (the previous use of lds has been read)
  if (lane == WAVE - 1) lds[wave] = v;
  __syncthreads();
  long long before = 0, all = 0;
#pragma unroll
  for (int k = 0; k < SCAN_THREADS / WAVE; ++k) { const long long t = lds[k]; all += t; if (k < wave) before += t; }
  *total = all;
  return v + before;
}

__global__ __launch_bounds__(SCAN_THREADS) void covwin_block_sums(const long long *__restrict__ diff, uint32_t n, long long *__restrict__ sums) {
  __shared__ long long lds[SCAN_THREADS / WAVE];
  const uint64_t base = (uint64_t)blockIdx.x * SCAN_BLOCK + (uint64_t)threadIdx.x * SCAN_ITEMS;
  long long v = 0;
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; ++k) if (base + k < n) v += diff[base + k];
  long long total;
  (void)block_scan(v, lds, &total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// sums[b] := the sum of sums[0 .. b), by ONE workgroup that walks the array in tiles and carries
__global__ __launch_bounds__(SCAN_THREADS) void covwin_scan_sums(long long *__restrict__ sums, uint32_t nb) {
  __shared__ long long lds[SCAN_THREADS / WAVE];
  long long carry = 0;
  for (uint32_t t0 = 0; t0 < nb; t0 += SCAN_THREADS) {          // (uniform trip count: every thread reaches the barriers)
    const uint32_t i = t0 + threadIdx.x;
    const long long v = i < nb ? sums[i] : 0;
    long long total;
    const long long incl = block_scan(v, lds, &total);
    if (i < nb) sums[i] = carry + incl - v;
    carry += total;
  }
}

__global__ __launch_bounds__(SCAN_THREADS) void covwin_add(long long *__restrict__ direct, const long long *__restrict__ diff, const long long *__restrict__ sums, uint32_t n) {
  __shared__ long long lds[SCAN_THREADS / WAVE];
  const uint64_t base = (uint64_t)blockIdx.x * SCAN_BLOCK + (uint64_t)threadIdx.x * SCAN_ITEMS;
  long long pre[SCAN_ITEMS], v = 0;
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; ++k) { if (base + k < n) v += diff[base + k]; pre[k] = v; }
  long long total;
  const long long before = block_scan(v, lds, &total) - v + sums[blockIdx.x];
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; ++k) if (base + k < n) direct[base + k] += before + pre[k];
}

void launch_covwin(hipStream_t st, const uint8_t *data, const uint32_t *offsets, uint32_t nrec, uint64_t first_ordinal, const Params &P, const int64_t *ref_len,
                   const int64_t *ref_first, unsigned long long *counters, unsigned long long *direct, unsigned long long *diff, unsigned long long *err_slot) {
  if (nrec) hipLaunchKernelGGL(covwin_kernel, dim3((nrec + 255) / 256), dim3(256), 0, st, data, offsets, nrec, first_ordinal, P, ref_len, ref_first, counters, direct, diff, err_slot);
}

// direct[k] += inclusive_prefix(diff)[k] for k < n; sums: (n + SCAN_BLOCK - 1) / SCAN_BLOCK values of scratch
void launch_covwin_scan(hipStream_t st, unsigned long long *direct, const unsigned long long *diff, unsigned long long *sums, uint32_t n) {
  if (!n) return;
  const uint32_t nb = (uint32_t)(((uint64_t)n + SCAN_BLOCK - 1) / SCAN_BLOCK);
  hipLaunchKernelGGL(covwin_block_sums, dim3(nb), dim3(SCAN_THREADS), 0, st, reinterpret_cast<const long long *>(diff), n, reinterpret_cast<long long *>(sums));
  hipLaunchKernelGGL(covwin_scan_sums, dim3(1), dim3(SCAN_THREADS), 0, st, reinterpret_cast<long long *>(sums), nb);
  hipLaunchKernelGGL(covwin_add, dim3(nb), dim3(SCAN_THREADS), 0, st, reinterpret_cast<long long *>(direct), reinterpret_cast<const long long *>(diff), reinterpret_cast<const long long *>(sums), n);
}

}  // namespace ckm
