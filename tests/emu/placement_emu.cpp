// placement_emu.cpp -- TEST INFRASTRUCTURE: the layout, the arithmetic, the level schedule and the chunk cuts of the phylogenetic placement
// (checkm_amd/csrc/place_dev.h) compiled by g++ against its HOST executor (place::run_host: the kernels of kernels_place.hip restated as
// loops over their threads, lanes and blocks of sixty-four sites), so that the CPU test suite runs the kernels' own arithmetic.  The
// partials and tables of a chunk start from NaN and poison exponents, so that a word that was never written shows.  Nothing in
// checkm_amd loads this.
#include <string>
#include "../../include/checkm_hip.h"
#include "../../checkm_amd/csrc/place_dev.h"

using namespace ckm;

namespace {
place::Args args_of(const ckm_place_args *a) {
  return place::Args{a->nnodes, a->child_off, a->child, a->nchild, a->length, a->nsites, a->nrows, a->row_off, a->rows, a->nrow_bytes,
                     a->nqueries, a->q_off, a->queries, a->nquery_bytes, a->nrates, a->weights, a->U, a->Uinv, a->pi, a->exp_len, a->exp_half,
                     a->nfrac, a->exp_dist, a->npend, a->exp_pend, a->max_pitches};
}
}  // namespace

// 0, or place::ARGS_INVALID / place::ARGS_RANGE
extern "C" int emu_place_check(const ckm_place_args *a) {
  std::string why;
  place::Schedule sch;
  return place::check(args_of(a), sch, why);
}

// info[0] = chunks, info[1] = sites of a chunk
extern "C" int emu_place_run(const ckm_place_args *a, uint64_t budget_bytes, const ckm_place_out *out, uint64_t *info) {
  std::string why;
  const place::Out o = {out->top_edge, out->scan_m, out->scan_e, out->ref_m, out->ref_e, out->ref_f, out->ref_g};
  return place::run_host(args_of(a), budget_bytes, o, info, why);
}

// the level schedule of a checked tree: up_off / up_nodes / down_off / down_nodes into the caller's arrays (N + 2, N, N + 1, N entries);
// returns the number of upward levels, or -1
extern "C" int emu_place_levels(const ckm_place_args *a, uint32_t *up_off, uint32_t *up_nodes, uint32_t *down_off, uint32_t *down_nodes, uint32_t *ndown) {
  std::string why;
  place::Schedule sch;
  if (place::check(args_of(a), sch, why)) return -1;
  for (size_t k = 0; k < sch.up_off.size(); ++k) up_off[k] = sch.up_off[k];
  for (size_t k = 0; k < sch.up_nodes.size(); ++k) up_nodes[k] = sch.up_nodes[k];
  for (size_t k = 0; k < sch.down_off.size(); ++k) down_off[k] = sch.down_off[k];
  for (size_t k = 0; k < sch.down_nodes.size(); ++k) down_nodes[k] = sch.down_nodes[k];
  *ndown = (uint32_t)sch.down_off.size() - 1;
  return (int)sch.up_off.size() - 1;
}
