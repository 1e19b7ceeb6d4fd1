// kernels_coverage.hip -- the device pass of `checkm coverage` over a batch of BAM records.  gfx950 only.  What a record is and how it
// is classified: coverage_dev.h, shared with the host executor of the CPU tests.
//
//   coverage_kernel   a lane per record.  The lane assembles the record's fields from bytes (records start at any address), walks the
//                     CIGAR and, when the chain gets that far, the auxiliary fields to the first NM.  A sorted BAM puts the same refID in
//                     consecutive records, so the wavefront reduces before it touches memory: a lane whose refID differs from the lane
//                     below it heads a run; one ballot per class and a population count over the run's lanes give the head the class
//                     counters, a segmented shuffle sum gives it the numerator; the head issues one global atomic add per non-zero
//                     value.  An unsorted file only costs more atomics: the sums are integers, so neither the order of the records
//                     nor where a run meets a wavefront or batch boundary changes a counter.
//                     A record the walk cannot finish puts (ordinal * 8 + reason) into the error slot by atomic minimum.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "coverage_dev.h"

namespace ckm {
using namespace cv;

__global__ __launch_bounds__(256) void coverage_kernel(const uint8_t *__restrict__ data, const uint32_t *__restrict__ offsets, uint32_t nrec, uint64_t first_ordinal,
                                                        Params P, unsigned long long *__restrict__ counters, unsigned long long *__restrict__ err_slot) {
  const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
  const int lane = threadIdx.x & (WAVE - 1);
  RecOut o = {-1, -1, 0, 0};
  if (idx < nrec) {                                            // (no early return: every lane takes part in the ballots below)
    classify(data + offsets[idx], P, o);
    if (o.err) { atomicMin(err_slot, (unsigned long long)((first_ordinal + idx) * 8u + o.err)); o.ref = -1; }
  }
  const int32_t ref = o.ref;
  const int32_t below = __shfl_up(ref, 1, WAVE);
  const bool head = lane == 0 || below != ref;
  const uint64_t heads = __ballot(head);
  const uint64_t above = lane == WAVE - 1 ? 0 : heads & ~(((uint64_t)2 << lane) - 1);
  const int end = above ? __ffsll((unsigned long long)above) - 1 : WAVE;                   // the first lane of the next run
  const uint64_t run = (end == WAVE ? ~(uint64_t)0 : (((uint64_t)1 << end) - 1)) & ~(((uint64_t)1 << lane) - 1);
  const bool counted = ref >= 0;
  unsigned long long add[NSLOT];
  add[SLOT_READS] = (unsigned long long)__popcll(__ballot(counted) & run);
#pragma unroll
  for (int c = 1; c < NCLASS; ++c) add[c] = (unsigned long long)__popcll(__ballot(counted && o.cls == c) & run);
  long long sum = counted && o.cls == 7 ? (long long)o.alen : 0;
#pragma unroll
  for (int d = 1; d < WAVE; d <<= 1) {
    const long long up = __shfl_down(sum, d, WAVE);
    if (lane + d < end) sum += up;
  }
  add[SLOT_NUMER] = (unsigned long long)sum;
  if (head && counted) {
    unsigned long long *row = counters + (uint64_t)ref * NSLOT;
#pragma unroll
    for (int k = 0; k < NSLOT; ++k) if (add[k]) atomicAdd(row + k, add[k]);
  }
}

void launch_coverage(hipStream_t st, const uint8_t *data, const uint32_t *offsets, uint32_t nrec, uint64_t first_ordinal, const Params &P,
                     unsigned long long *counters, unsigned long long *err_slot) {
  if (nrec) hipLaunchKernelGGL(coverage_kernel, dim3((nrec + 255) / 256), dim3(256), 0, st, data, offsets, nrec, first_ordinal, P, counters, err_slot);
}

}  // namespace ckm
