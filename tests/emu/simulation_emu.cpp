// simulation_emu.cpp -- TEST INFRASTRUCTURE: the layout, the arithmetic, the packing and the round cuts of the marker-set simulation
// (checkm_amd/csrc/sim_dev.h) compiled by g++ against a HOST executor, so that the CPU test suite runs the kernel's own arithmetic.
// sim_kernel of kernels_sim.hip is restated as loops over its blocks and lanes (its last step is score_sets_emu.h); every buffer the
// kernel reads or writes has exactly the size the library gives it (the staged starts and the counts exactly the size the block uses),
// the counts and the outputs start from poison values, so that a word that was never written shows.  Nothing in checkm_amd loads this.
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>
#include "../../include/checkm_hip.h"
#include "../../checkm_amd/csrc/sim_dev.h"
#include "score_sets_emu.h"

using namespace ckm;

namespace {
sim::Args args_of(const ckm_sim_args *a) {
  return sim::Args{a->nmarkers, a->key_off, a->key, a->nsets, a->ms_off, a->cs_off, a->cs_marker, a->nreplicates, a->rs_off, a->starts, a->contig_len};
}

// sim_kernel: block b of the launch for replicates [r0, r0 + nr)
void block(const sim::Packed &P, uint32_t U, uint32_t S, uint32_t r0, uint32_t b, const uint64_t *rs_off, uint64_t start_base, const std::vector<int32_t> &starts,
           std::vector<uint32_t> &scratch, std::vector<double> &out) {
  const uint32_t r = r0 + b;
  const uint64_t o = rs_off[r];
  const uint32_t n = (uint32_t)(rs_off[r + 1] - o);
  const bool staged = n <= sim::STAGE_STARTS;
  std::vector<int32_t> sStarts;
  if (staged)
    for (uint32_t k = 0; k < n; ++k) sStarts.push_back(starts.at(o - start_base + k));
  const int32_t *s = staged ? sStarts.data() : starts.data() + (o - start_base);
  std::vector<uint32_t> sCounts(U <= sim::STAGE_COUNTS ? U : 0, 0xEEEEEEEEu);
  uint32_t *counts = U <= sim::STAGE_COUNTS ? sCounts.data() : &scratch.at((uint64_t)b * U);
  const int32_t len = P.contig_len.at(r);
  for (uint32_t thread = 0; thread < (uint32_t)sim::THREADS; ++thread)
    for (uint32_t m = thread; m < U; m += sim::THREADS) counts[m] = sim::marker_count(P.key.data(), P.key_off.at(m), P.key_off.at(m + 1), s, n, len);
  score_sets_emu(P, S, counts, b, out);
}
}  // namespace

// 0, or sim::ARGS_INVALID / sim::ARGS_RANGE
extern "C" int emu_sim_check(const ckm_sim_args *a) {
  std::string why;
  return sim::check(args_of(a), a->ncs, a->nmembers, a->nkeys, a->nstarts, why);
}

// out [nreplicates * nsets * 4]; info[0] = rounds
extern "C" int emu_sim_run(const ckm_sim_args *a, uint64_t budget_bytes, double *out, uint64_t *info) {
  const int kind = emu_sim_check(a);
  if (kind) return kind;
  const sim::Args A = args_of(a);
  const uint32_t R = a->nreplicates, S = a->nsets, U = a->nmarkers;
  info[0] = 0;
  if (R == 0 || S == 0) return 0;
  sim::Packed P;
  sim::pack(A, P);
  for (uint32_t r0 = 0; r0 < R;) {
    const uint32_t r1 = sim::next_round(R, a->rs_off, U, S, budget_bytes, r0), nr = r1 - r0;
    const uint64_t base = a->rs_off[r0], n = a->rs_off[r1] - base;
    std::vector<int32_t> starts(n);
    for (uint64_t k = 0; k < n; ++k) starts[k] = (int32_t)a->starts[base + k];
    std::vector<uint32_t> scratch(U > sim::STAGE_COUNTS ? (size_t)nr * U : 0, 0xEEEEEEEEu);
    std::vector<double> round_out((size_t)nr * S * 4, std::numeric_limits<double>::quiet_NaN());
    for (uint32_t b = 0; b < nr; ++b) block(P, U, S, r0, b, a->rs_off, base, starts, scratch, round_out);
    memcpy(out + (size_t)r0 * S * 4, round_out.data(), round_out.size() * 8);
    info[0] += 1;
    r0 = r1;
  }
  return 0;
}
