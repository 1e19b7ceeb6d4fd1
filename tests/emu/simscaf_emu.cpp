// simscaf_emu.cpp -- TEST INFRASTRUCTURE: the layout, the arithmetic, the packing and the round cuts of the scaffold simulation
// (checkm_amd/csrc/simscaf_dev.h) compiled by g++ against a HOST executor, so that the CPU test suite runs the kernel's own arithmetic.
// simscaf_kernel of kernels_simscaf.hip and score_sets of sim_score.h are restated as loops over their blocks, wavefronts and lanes; every
// buffer the kernel reads or writes has exactly the size the library gives it (the staged rows and the counts exactly the size the block
// uses), the counts and the outputs start from poison values, so that a word that was never written shows.  Nothing in checkm_amd loads
// this.
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>
#include "../../include/checkm_hip.h"
#include "../../checkm_amd/csrc/simscaf_dev.h"

using namespace ckm;

namespace {
simscaf::Args args_of(const ckm_simscaf_args *a) {
  return simscaf::Args{a->ngenomes, a->nscaf, a->nmarkers, a->sc_off, a->sc, a->nsets, a->ms_off, a->cs_off, a->cs_marker, a->nreplicates, a->test, a->cont, a->bit_off, a->bits};
}

// simscaf_kernel: block b of the launch for replicates [r0, r0 + nr)
void block(const ckm_simscaf_args *a, const simscaf::Packed &P, uint32_t r0, uint32_t b, uint64_t bit_base, const std::vector<uint32_t> &bits, std::vector<uint32_t> &scratch,
           std::vector<double> &out) {
  const uint32_t U = a->nmarkers, S = a->nsets, r = r0 + b;
  const uint32_t g = a->test[r], h = a->cont[r];
  const uint32_t wt = simscaf::row_words(a->nscaf[g]), wc = h == simscaf::NONE ? 0u : simscaf::row_words(a->nscaf[h]);
  const uint64_t o = a->bit_off[r] - bit_base;
  const bool staged_t = wt <= simscaf::STAGE_WORDS, staged_c = wc <= simscaf::STAGE_WORDS;
  std::vector<uint32_t> sTest, sCont;
  if (staged_t)
    for (uint32_t k = 0; k < wt; ++k) sTest.push_back(bits.at(o + k));
  if (staged_c)
    for (uint32_t k = 0; k < wc; ++k) sCont.push_back(bits.at(o + wt + k));
  if (wt + wc) (void)bits.at(o + wt + wc - 1);
  const uint32_t *trow = staged_t ? sTest.data() : bits.data() + o, *crow = staged_c ? sCont.data() : bits.data() + o + wt;
  std::vector<uint32_t> sCounts(U <= simscaf::STAGE_COUNTS ? U : 0, 0xEEEEEEEEu);
  uint32_t *counts = U <= simscaf::STAGE_COUNTS ? sCounts.data() : &scratch.at((uint64_t)b * U);
  const uint64_t tcell = (uint64_t)g * U, ccell = h == simscaf::NONE ? 0ull : (uint64_t)h * U;
  for (uint32_t thread = 0; thread < (uint32_t)simscaf::THREADS; ++thread)
    for (uint32_t m = thread; m < U; m += simscaf::THREADS) {
      uint32_t c = simscaf::row_count(a->sc, P.sc_off.at(tcell + m), P.sc_off.at(tcell + m + 1), trow);
      if (h != simscaf::NONE) c += simscaf::row_count(a->sc, P.sc_off.at(ccell + m), P.sc_off.at(ccell + m + 1), crow);
      counts[m] = c;
    }
  // score_sets
  const sim::Packed &M = P.sets;
  for (uint32_t wave = 0; wave < (uint32_t)sim::WAVES; ++wave)
    for (uint32_t ms = wave; ms < S; ms += sim::WAVES) {
      const uint32_t c0 = M.ms_off.at(ms), c1 = M.ms_off.at(ms + 1);
      sim::Individual ind[sim::WAVE] = {};
      double comp = 0.0, cont = 0.0;
      for (uint32_t base = c0; base < c1; base += sim::WAVE) {
        double tc[sim::WAVE], tn[sim::WAVE];
        for (int lane = 0; lane < sim::WAVE; ++lane) {
          const uint32_t c = base + (uint32_t)lane;
          tc[lane] = tn[lane] = 0.0;
          if (c < c1) sim::set_terms(M.cs_marker.data(), M.cs_off.at(c), M.cs_off.at(c + 1), counts, tc[lane], tn[lane], ind[lane]);
        }
        const int here = c1 - base < (uint32_t)sim::WAVE ? (int)(c1 - base) : sim::WAVE;
        for (int l = 0; l < here; ++l) { comp += tc[l]; cont += tn[l]; }
      }
      sim::Individual all = {0u, 0ull};
      for (int lane = 0; lane < sim::WAVE; ++lane) { all.present += ind[lane].present; all.multi += ind[lane].multi; }
      const uint64_t at = ((uint64_t)b * S + ms) * 4;
      (void)out.at(at + 3);
      sim::finish(all, M.num_markers.at(ms), comp, cont, c1 - c0, &out.at(at));
    }
}
}  // namespace

// 0, or ARGS_INVALID / ARGS_RANGE
extern "C" int emu_simscaf_check(const ckm_simscaf_args *a) {
  std::string why;
  return simscaf::check(args_of(a), a->nsc, a->ncs, a->nmembers, a->nwords, why);
}

// out [nreplicates * nsets * 4]; info[0] = rounds
extern "C" int emu_simscaf_run(const ckm_simscaf_args *a, uint64_t budget_bytes, double *out, uint64_t *info) {
  const int kind = emu_simscaf_check(a);
  if (kind) return kind;
  const uint32_t R = a->nreplicates, S = a->nsets, U = a->nmarkers;
  info[0] = 0;
  if (R == 0 || S == 0) return 0;
  simscaf::Packed P;
  simscaf::pack(args_of(a), P);
  for (uint32_t r0 = 0; r0 < R;) {
    const uint32_t r1 = simscaf::next_round(R, a->bit_off, U, S, budget_bytes, r0), nr = r1 - r0;
    const uint64_t base = a->bit_off[r0], n = a->bit_off[r1] - base;
    std::vector<uint32_t> bits(n);
    for (uint64_t k = 0; k < n; ++k) bits[k] = a->bits[base + k];
    std::vector<uint32_t> scratch(U > simscaf::STAGE_COUNTS ? (size_t)nr * U : 0, 0xEEEEEEEEu);
    std::vector<double> round_out((size_t)nr * S * 4, std::numeric_limits<double>::quiet_NaN());
    for (uint32_t b = 0; b < nr; ++b) block(a, P, r0, b, base, bits, scratch, round_out);
    memcpy(out + (size_t)r0 * S * 4, round_out.data(), round_out.size() * 8);
    info[0] += 1;
    r0 = r1;
  }
  return 0;
}
