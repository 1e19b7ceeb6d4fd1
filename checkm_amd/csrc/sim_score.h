// sim_score.h -- the last step of the two simulation kernels (kernels_sim.hip, kernels_simscaf.hip): MarkerSet.genomeCheck in both modes
// (checkm/markerSets.py:206-238) for every marker set of a call, from the block's marker counts.  Device code only; the layout and the
// arithmetic are marker_sets.h's.
//
// A wavefront owns a marker set: sixty-four co-located sets at a time, a lane forms the two quotients of its set, then every lane adds the
// sixty-four terms in list order (a broadcast read of lane l's registers), so lane 0 holds the reference's sums.  The integer sums of the
// individual mode go through a butterfly over the wavefront.  No atomics; every output word has one writer.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "sim_dev.h"

namespace ckm {
namespace sim {

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
  for (int d = WAVE / 2; d > 0; d >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, d, WAVE);
  return v;
}

// counts: the block's marker counts, complete and visible to every wavefront of the block; out_row [S][4], the block's own
__device__ __forceinline__ void score_sets(const msets::SetsDev &M, const uint32_t *counts, double *out_row) {
  const int lane = threadIdx.x & (WAVE - 1);
  for (uint32_t ms = threadIdx.x >> 6; ms < M.S; ms += WAVES) {
    const uint32_t c0 = M.ms_off[ms], c1 = M.ms_off[ms + 1];
    msets::Individual ind = {0u, 0ull};
    double comp = 0.0, cont = 0.0;
    for (uint32_t base = c0; base < c1; base += WAVE) {
      const uint32_t c = base + (uint32_t)lane;
      double tc = 0.0, tn = 0.0;
      if (c < c1) msets::set_terms(M.cs_marker, M.cs_off[c], M.cs_off[c + 1], counts, tc, tn, ind);
      const int here = c1 - base < (uint32_t)WAVE ? (int)(c1 - base) : WAVE;
      for (int l = 0; l < here; ++l) {                          // list order; the same in every lane
        comp += __shfl(tc, l, WAVE);
        cont += __shfl(tn, l, WAVE);
      }
    }
    ind.present = (uint32_t)wave_sum(ind.present);
    ind.multi = wave_sum(ind.multi);
    if (lane == 0) msets::finish(ind, M.num_markers[ms], comp, cont, c1 - c0, out_row + (uint64_t)ms * 4);
  }
}

}  // namespace sim
}  // namespace ckm
