// simscaf_emu.cpp -- TEST INFRASTRUCTURE: the layout, the arithmetic, the packing and the round cuts of the scaffold simulation
// (checkm_amd/csrc/simscaf_dev.h) compiled by g++ against a HOST executor, so that the CPU test suite runs the kernel's own arithmetic.
// simscaf_kernel of kernels_simscaf.hip is restated as loops over its blocks and lanes (its last step is score_sets_emu.h); every
// buffer the kernel reads or writes has exactly the size the library gives it (the staged rows and the counts exactly the size the block
// uses), the counts and the outputs start from poison values, so that a word that was never written shows.  Nothing in checkm_amd loads
// this.
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>
#include "../../include/checkm_hip.h"
#include "../../checkm_amd/csrc/simscaf_dev.h"
#include "score_sets_emu.h"

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
  score_sets_emu(P.sets, S, counts, b, out);
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
