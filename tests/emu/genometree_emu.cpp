// genometree_emu.cpp -- TEST INFRASTRUCTURE: the layout, the arithmetic and the batch cuts of the genome tree
// (checkm_amd/csrc/gtree_dev.h) compiled by g++ against the header's HOST executor, so that the CPU test suite runs the kernels' own
// arithmetic: run_host restates the kernels as loops over their threads with the same functions.  The outputs start from poison values,
// so that a word that was never written shows.  Nothing in checkm_amd loads this.
#include <cstring>
#include <limits>
#include <string>
#include <vector>
#include "../../include/checkm_hip.h"
#include "../../checkm_amd/csrc/gtree_dev.h"

using namespace ckm;

namespace {
gtree::Args args_of(const ckm_gtree_args *a) {
  return gtree::Args{a->nrows, a->ncols, a->text, a->ntext_bytes, a->nreps, a->cols, a->base, a->model, a->max_dist, a->matrix, a->nmatrices};
}
}  // namespace

// 0, or gtree::ARGS_INVALID / gtree::ARGS_RANGE
extern "C" int emu_gtree_check(const ckm_gtree_args *a) {
  std::string why;
  return gtree::check(args_of(a), why);
}

// info[0] = batches, info[1] = trees
extern "C" int emu_gtree_run(const ckm_gtree_args *a, uint64_t budget_bytes, const ckm_gtree_out *out, uint64_t *info) {
  std::string why;
  const int kind = gtree::check(args_of(a), why);
  if (kind) return kind;
  const size_t N = a->nrows, T = gtree::trees_of(args_of(a));
  if (out->compared) { memset(out->compared, 0xEE, N * N * 4); memset(out->differ, 0xEE, N * N * 4); }
  if (out->dist) for (size_t k = 0; k < N * N; ++k) out->dist[k] = std::numeric_limits<double>::quiet_NaN();
  if (out->merge_ij) {
    memset(out->merge_ij, 0xEE, T * (N - 1) * 8);
    for (size_t k = 0; k < T * (N - 1) * 2; ++k) out->merge_len[k] = std::numeric_limits<double>::quiet_NaN();
  }
  return gtree::run_host(args_of(a), budget_bytes, gtree::Out{out->compared, out->differ, out->dist, out->merge_ij, out->merge_len}, info, why);
}

extern "C" double emu_gtree_log(double x) { return gtree::log_pos(x); }
extern "C" double emu_gtree_dist(uint32_t compared, uint32_t differ, int model, double max_dist) { return gtree::dist_of(compared, differ, model, max_dist); }
extern "C" double emu_gtree_arg(double p, int model) { return gtree::model_arg(p, model); }
// log_pos over n arguments at once
extern "C" void emu_gtree_logs(const double *x, uint64_t n, double *y) { for (uint64_t k = 0; k < n; ++k) y[k] = gtree::log_pos(x[k]); }
