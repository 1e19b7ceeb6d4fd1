// kernels_sim.hip -- the marker-set simulation on the device (scripts/simulation.py of the reference, worker :97-142: per draw of contigs
// MarkerSetBuilder.containedMarkerGenes, markerSetBuilder.py:353-369, then MarkerSet.genomeCheck, checkm/markerSets.py:206-238, in both
// modes for every marker set).  gfx950 only.  The layout and the arithmetic are sim_dev.h, shared with the host executor of the CPU
// tests; the float operations are IEEE double divisions, multiplications and additions in the reference's order (the library's
// -ffp-contract=off -fno-fast-math).
//
//   sim_kernel   a block of four wavefronts per replicate; one launch covers the replicates of a round.
//                1. The replicate's sorted starts are staged in LDS (STAGE_STARTS of them; a longer list stays in global memory and is
//                   searched there by the same code).
//                2. A lane owns a marker and walks its copies: two binary searches per copy.  The U counts stay in LDS (STAGE_COUNTS of
//                   them; more go to the block's scratch row in global memory).  The searches of neighbouring lanes land on unrelated
//                   banks: their conflicts are the price of a search and are not laid out away.
//                3. A wavefront owns a marker set and scores it from the counts (score_sets of sim_score.h, shared with
//                   kernels_simscaf.hip): the quotients of the co-located sets summed in list order, the integers by butterfly.
//                No atomics; every output word has one writer.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "sim_dev.h"
#include "sim_score.h"

namespace ckm {
using namespace sim;

// replicate r0 + blockIdx.x of the call; starts holds the round's starts, the first of them being entry start_base of the call's list;
// scratch [blocks][U] only when U > STAGE_COUNTS; out [blocks][S][4]
__global__ __launch_bounds__(THREADS) void sim_kernel(SimDev T, uint32_t r0, const uint64_t *__restrict__ rs_off, uint64_t start_base, const int32_t *__restrict__ starts,
                                                       const int32_t *__restrict__ contig_len, uint32_t *__restrict__ scratch, double *__restrict__ out) {
  __shared__ int32_t sStarts[STAGE_STARTS];
  __shared__ uint32_t sCounts[STAGE_COUNTS];
  const uint32_t r = r0 + blockIdx.x;
  const uint64_t o = rs_off[r];
  const uint32_t n = (uint32_t)(rs_off[r + 1] - o);
  const int32_t *mine = starts + (o - start_base);
  const bool staged = n <= STAGE_STARTS;
  if (staged)
    for (uint32_t k = threadIdx.x; k < n; k += THREADS) sStarts[k] = mine[k];
  __syncthreads();
  const int32_t *s = staged ? sStarts : mine;
  uint32_t *counts = T.U <= STAGE_COUNTS ? sCounts : scratch + (uint64_t)blockIdx.x * T.U;
  const int32_t len = contig_len[r];
  for (uint32_t m = threadIdx.x; m < T.U; m += THREADS) counts[m] = marker_count(T.key, T.key_off[m], T.key_off[m + 1], s, n, len);
  __syncthreads();                                              // the counts, in LDS or in the block's own scratch row
  score_sets(T.sets, counts, out + (uint64_t)blockIdx.x * T.sets.S * 4);
}

void launch_sim(hipStream_t st, const SimDev &T, uint32_t r0, uint32_t nr, const uint64_t *rs_off, uint64_t start_base, const int32_t *starts, const int32_t *contig_len,
                uint32_t *scratch, double *out) {
  if (!nr || !T.sets.S) return;
  hipLaunchKernelGGL(sim_kernel, dim3(nr), dim3(THREADS), 0, st, T, r0, rs_off, start_base, starts, contig_len, scratch, out);
}

}  // namespace ckm
