// score_sets_emu.h -- TEST INFRASTRUCTURE: score_sets of checkm_amd/csrc/sim_score.h restated as loops over its wavefronts and lanes, for
// the host executors of the three passes that score marker sets (simulation_emu.cpp, simscaf_emu.cpp, selection_emu.cpp).  The arithmetic
// is marker_sets.h's own; every table is read through .at(), and the output row is the caller's, poisoned before the call.
#pragma once
#include <cstdint>
#include <vector>
#include "../../checkm_amd/csrc/marker_sets.h"
#include "../../checkm_amd/csrc/sim_dev.h"

namespace ckm {

// block b of a launch: counts are the block's marker counts, out [blocks][S][4]
inline void score_sets_emu(const msets::Packed &M, uint32_t S, const uint32_t *counts, uint32_t b, std::vector<double> &out) {
  for (uint32_t wave = 0; wave < (uint32_t)sim::WAVES; ++wave)
    for (uint32_t ms = wave; ms < S; ms += sim::WAVES) {
      const uint32_t c0 = M.ms_off.at(ms), c1 = M.ms_off.at(ms + 1);
      msets::Individual ind[sim::WAVE] = {};
      double comp = 0.0, cont = 0.0;
      for (uint32_t base = c0; base < c1; base += sim::WAVE) {
        double tc[sim::WAVE], tn[sim::WAVE];
        for (int lane = 0; lane < sim::WAVE; ++lane) {
          const uint32_t c = base + (uint32_t)lane;
          tc[lane] = tn[lane] = 0.0;
          if (c < c1) msets::set_terms(M.cs_marker.data(), M.cs_off.at(c), M.cs_off.at(c + 1), counts, tc[lane], tn[lane], ind[lane]);
        }
        const int here = c1 - base < (uint32_t)sim::WAVE ? (int)(c1 - base) : sim::WAVE;
        for (int l = 0; l < here; ++l) { comp += tc[l]; cont += tn[l]; }
      }
      msets::Individual all = {0u, 0ull};
      for (int lane = 0; lane < sim::WAVE; ++lane) { all.present += ind[lane].present; all.multi += ind[lane].multi; }
      const uint64_t at = ((uint64_t)b * S + ms) * 4;
      (void)out.at(at + 3);
      msets::finish(all, M.num_markers.at(ms), comp, cont, c1 - c0, &out.at(at));
    }
}

}  // namespace ckm
