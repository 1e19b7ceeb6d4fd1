// gtree_host.cpp -- host side of the genome tree (additions to ABI 12): ckm_gtree_check, which says why the alignment, the drawn columns,
// the model or the matrices of a call would be refused and needs no device, and ckm_gtree_host, the host executor of gtree_dev.h behind
// the same arguments (what the stand-alone check and the tools' comparisons run).  Host code only.
#include <string>
#include "ckm_internal.h"
#include "gtree_dev.h"

using namespace ckm;

namespace ckm {
gtree::Args gtree_args_of(const ckm_gtree_args *a) {
  return gtree::Args{a->nrows, a->ncols, a->text, a->ntext_bytes, a->nreps, a->cols, a->base, a->model, a->max_dist, a->matrix, a->nmatrices};
}
int gtree_check_args(const ckm_gtree_args *a, std::string &why) {
  if (!a) { why = "NULL argument"; return gtree::ARGS_INVALID; }
  return gtree::check(gtree_args_of(a), why);
}
}  // namespace ckm

extern "C" int ckm_gtree_check(const ckm_gtree_args *a) {
  return check_entry([&](std::string &why) { return gtree_check_args(a, why); });
}

extern "C" int ckm_gtree_host(const ckm_gtree_args *a, uint64_t budget_bytes, const ckm_gtree_out *out, ckm_gtree_info *info) {
  return check_entry([&](std::string &why) {
    int kind = gtree_check_args(a, why);
    if (kind == gtree::ARGS_OK && (!out || (out->compared && !out->differ) || (out->merge_ij && !out->merge_len))) { kind = gtree::ARGS_INVALID; why = "NULL argument"; }
    if (kind == gtree::ARGS_OK) {
      uint64_t counts[2] = {0, 0};
      kind = gtree::run_host(gtree_args_of(a), batch_budget(budget_bytes, "CKM_GTREE_BATCH_MB", 2048), gtree::Out{out->compared, out->differ, out->dist, out->merge_ij, out->merge_len},
                             counts, why);
      if (kind == gtree::ARGS_OK && info) { *info = ckm_gtree_info(); info->nrounds = counts[0]; info->ntrees = counts[1]; }
    }
    return kind;
  });
}
