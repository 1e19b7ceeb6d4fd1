// selection_emu.cpp -- TEST INFRASTRUCTURE: the layout, the generator, the draw, the packing and the round cuts of the marker-set
// selection (checkm_amd/csrc/select_dev.h) compiled by g++ against a HOST executor, so that the CPU test suite runs the kernel's own
// arithmetic.  select_kernel of kernels_select.hip is restated as loops over its blocks; the threshold pair of the completeness draw is
// found with std::nth_element, not with the kernel's counting passes: the taken set is defined by the rule, not by the method.  Every
// buffer the kernel reads or writes has exactly the size the library gives it (the multiplicities and the counts exactly the size the
// block uses), the counts and the outputs start from poison values, so that a word that was never written shows.  Nothing in checkm_amd
// loads this.
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>
#include "../../include/checkm_hip.h"
#include "../../checkm_amd/csrc/select_dev.h"
#include "score_sets_emu.h"

using namespace ckm;

namespace {
sel::Args args_of(const ckm_select_args *a) {
  return sel::Args{a->ngenomes, a->genome_len, a->nmarkers, a->key_off, a->key, a->nsets, a->ms_off, a->cs_off, a->cs_marker,
                   a->nreplicates, a->contig_len, a->comp_lo, a->comp_hi, a->cont_lo, a->cont_hi, a->seed};
}

// select_kernel: block b of the launch for draws [d0, d0 + nd)
void block(const sel::Packed &P, const int64_t *genome_len, uint32_t U, uint32_t S, uint32_t R, uint32_t d0, uint32_t b, uint64_t row_base, std::vector<double> &truth,
           std::vector<double> &out, std::vector<uint32_t> &scratch, std::vector<uint16_t> *rows) {
  const uint32_t d = d0 + b, g = d / R, r = d % R;
  const uint32_t C = P.ncontigs.at(g);
  const sel::Plan plan = sel::plan_of(P.params, genome_len[g], C, g, r);
  std::vector<uint32_t> mult(C, 0u);
  std::vector<uint64_t> pairs(C);
  for (uint32_t i = 0; i < C; ++i) pairs[i] = sel::pair_of(sel::words_of(P.params.seed, sel::STREAM_COMP, g, r, i / 4).w[i % 4], i);
  if (plan.ncomp > 0) {
    std::vector<uint64_t> order(pairs);
    std::nth_element(order.begin(), order.begin() + (plan.ncomp - 1), order.end());
    const uint64_t threshold = order.at(plan.ncomp - 1);
    for (uint32_t i = 0; i < C; ++i) mult[i] = pairs[i] <= threshold ? 1u : 0u;
  }
  for (uint32_t j = 0; j < plan.ncont; ++j) mult.at(sel::landing(sel::words_of(P.params.seed, sel::STREAM_CONT, g, r, j / 4).w[j % 4], C)) += 1;
  if (rows)
    for (uint32_t i = 0; i < C; ++i) rows->at(P.row_off.at(g) + (uint64_t)r * C - row_base + i) = sel::row_entry(mult[i]);
  std::vector<uint32_t> sCounts(U <= sim::STAGE_COUNTS ? U : 0, 0xEEEEEEEEu);
  uint32_t *counts = U <= sim::STAGE_COUNTS ? sCounts.data() : (U ? &scratch.at((uint64_t)b * U) : nullptr);
  const uint32_t *koff = P.key_off.data() + (uint64_t)g * U;
  for (uint32_t m = 0; m < U; ++m) counts[m] = sel::marker_mult(P.key.data(), koff[m], koff[m + 1], mult.data(), C, P.params.contig_len);
  truth.at((uint64_t)b * 2) = plan.true_comp; truth.at((uint64_t)b * 2 + 1) = plan.true_cont;
  score_sets_emu(P.sets, S, counts, b, out);
}
}  // namespace

// 0, or sim::ARGS_INVALID / sim::ARGS_RANGE
extern "C" int emu_select_check(const ckm_select_args *a) {
  std::string why;
  return sel::check(args_of(a), a->ncs, a->nmembers, a->nkeys, why);
}

extern "C" void emu_philox(const uint32_t *counter, const uint32_t *key, uint32_t *words) {
  const sel::Words w = sel::philox(counter[0], counter[1], counter[2], counter[3], key[0], key[1]);
  memcpy(words, w.w, 16);
}

extern "C" double emu_unit(uint32_t a, uint32_t b) { return sel::unit(a, b); }

// truth [G * R * 2]; out [G * R * nsets * 4]; rows NULL or [sum of R * C_g]; info[0] = rounds
extern "C" int emu_select_run(const ckm_select_args *a, uint64_t budget_bytes, double *truth, double *out, uint16_t *rows, uint64_t *info) {
  const int kind = emu_select_check(a);
  if (kind) return kind;
  const uint32_t G = a->ngenomes, R = a->nreplicates, S = a->nsets, U = a->nmarkers, D = G * R;
  info[0] = 0;
  if (D == 0) return 0;
  sel::Packed P;
  sel::pack(args_of(a), P);
  for (uint32_t d0 = 0; d0 < D;) {
    const uint32_t d1 = sel::next_round(P, R, U, S, rows != nullptr, budget_bytes, d0), nd = d1 - d0;
    const uint64_t row_base = sel::row_at(P, R, d0), nrow = sel::row_at(P, R, d1) - row_base;
    std::vector<uint32_t> scratch(U > sim::STAGE_COUNTS ? (size_t)nd * U : 0, 0xEEEEEEEEu);
    std::vector<double> round_truth((size_t)nd * 2, std::numeric_limits<double>::quiet_NaN()), round_out((size_t)nd * S * 4, std::numeric_limits<double>::quiet_NaN());
    std::vector<uint16_t> round_rows(rows ? nrow : 0, (uint16_t)0xEEEE);
    for (uint32_t b = 0; b < nd; ++b) block(P, a->genome_len, U, S, R, d0, b, row_base, round_truth, round_out, scratch, rows ? &round_rows : nullptr);
    memcpy(truth + (size_t)d0 * 2, round_truth.data(), round_truth.size() * 8);
    if (S) memcpy(out + (size_t)d0 * S * 4, round_out.data(), round_out.size() * 8);
    if (rows && nrow) memcpy(rows + row_base, round_rows.data(), nrow * 2);
    info[0] += 1;
    d0 = d1;
  }
  return 0;
}
