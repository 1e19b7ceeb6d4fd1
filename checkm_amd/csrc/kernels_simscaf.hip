// kernels_simscaf.hip -- the scaffold simulation on the device (scripts/simulationScaffoldsRandom.py and simulationScaffoldsByLength.py of
// the reference, workers :137-162: per draw of scaffolds MarkerSetBuilder.markerGenesOnScaffolds, markerSetBuilder.py:371-378, for the test
// genome and for the contaminant, then MarkerSet.genomeCheck, checkm/markerSets.py:206-238, in both modes for every marker set).  gfx950
// only.  The layout and the arithmetic are simscaf_dev.h, shared with the host executor of the CPU tests; the float operations are IEEE
// double divisions, multiplications and additions in the reference's order (the library's -ffp-contract=off -fno-fast-math).
//
//   simscaf_kernel   a block of four wavefronts per replicate; one launch covers the replicates of a round.
//                    1. The two bit rows of the replicate -- kept scaffolds of the test genome, sampled scaffolds of the contaminant -- are
//                       staged in LDS (STAGE_BITS scaffolds each; a longer row stays in global memory and is read there by the same code).
//                    2. A lane owns a marker and walks its copies in both genomes: a bit test per copy.  The U counts stay in LDS
//                       (STAGE_COUNTS of them; more go to the block's scratch row in global memory).
//                    3. A wavefront owns a marker set and scores it from the counts (score_sets of sim_score.h, shared with
//                       kernels_sim.hip).
//                    No atomics; every output word has one writer.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "simscaf_dev.h"
#include "sim_score.h"

namespace ckm {
using namespace simscaf;

// replicate r0 + blockIdx.x of the call; bits holds the round's rows, the first of them being word bit_base of the call's list;
// scratch [blocks][U] only when U > STAGE_COUNTS; out [blocks][S][4]
__global__ __launch_bounds__(THREADS) void simscaf_kernel(SimScafDev T, uint32_t r0, const uint32_t *__restrict__ test, const uint32_t *__restrict__ cont,
                                                           const uint64_t *__restrict__ bit_off, uint64_t bit_base, const uint32_t *__restrict__ bits,
                                                           uint32_t *__restrict__ scratch, double *__restrict__ out) {
  __shared__ uint32_t sTest[STAGE_WORDS];
  __shared__ uint32_t sCont[STAGE_WORDS];
  __shared__ uint32_t sCounts[STAGE_COUNTS];
  const uint32_t r = r0 + blockIdx.x;
  const uint32_t g = test[r], h = cont[r];
  const uint32_t wt = row_words(T.nscaf[g]), wc = h == NONE ? 0u : row_words(T.nscaf[h]);
  const uint32_t *mine = bits + (bit_off[r] - bit_base);
  const bool staged_t = wt <= STAGE_WORDS, staged_c = wc <= STAGE_WORDS;
  if (staged_t)
    for (uint32_t k = threadIdx.x; k < wt; k += THREADS) sTest[k] = mine[k];
  if (staged_c)
    for (uint32_t k = threadIdx.x; k < wc; k += THREADS) sCont[k] = mine[wt + k];
  __syncthreads();
  const uint32_t *trow = staged_t ? sTest : mine, *crow = staged_c ? sCont : mine + wt;
  uint32_t *counts = T.U <= STAGE_COUNTS ? sCounts : scratch + (uint64_t)blockIdx.x * T.U;
  const uint64_t tcell = (uint64_t)g * T.U, ccell = h == NONE ? 0ull : (uint64_t)h * T.U;
  for (uint32_t m = threadIdx.x; m < T.U; m += THREADS) {
    uint32_t c = row_count(T.sc, T.sc_off[tcell + m], T.sc_off[tcell + m + 1], trow);
    if (h != NONE) c += row_count(T.sc, T.sc_off[ccell + m], T.sc_off[ccell + m + 1], crow);
    counts[m] = c;
  }
  __syncthreads();                                              // the counts, in LDS or in the block's own scratch row
  sim::score_sets(T.sets, counts, out + (uint64_t)blockIdx.x * T.sets.S * 4);
}

void launch_simscaf(hipStream_t st, const SimScafDev &T, uint32_t r0, uint32_t nr, const uint32_t *test, const uint32_t *cont, const uint64_t *bit_off, uint64_t bit_base,
                    const uint32_t *bits, uint32_t *scratch, double *out) {
  if (!nr || !T.sets.S) return;
  hipLaunchKernelGGL(simscaf_kernel, dim3(nr), dim3(THREADS), 0, st, T, r0, test, cont, bit_off, bit_base, bits, scratch, out);
}

}  // namespace ckm
