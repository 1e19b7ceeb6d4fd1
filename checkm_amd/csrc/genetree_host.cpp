// genetree_host.cpp -- host side of the gene-tree tests (additions to ABI 12): ckm_genetree_check, which says why the forest of a call
// would be refused and needs no device, and ckm_genetree_host, the host executor of genetree_dev.h behind the same arguments (what the
// stand-alone check and the tools' comparisons run).  Host code only.
#include <string>
#include "ckm_internal.h"
#include "genetree_dev.h"

using namespace ckm;

namespace ckm {
genetree::Args genetree_args_of(const ckm_genetree_args *a) {
  return genetree::Args{a->ntrees, a->node_off, a->leaf_off, a->class_off, a->group_off, a->gpair_off, a->first, a->last, a->parent, a->length, a->internal,
                        a->leaf_genome, a->leaf_species, a->leaf_class, a->class_total, a->pair_a, a->pair_b};
}
int genetree_check_args(const ckm_genetree_args *a, std::string &why) {
  if (!a) { why = "NULL argument"; return genetree::ARGS_INVALID; }
  return genetree::check(genetree_args_of(a), why);
}
// the outputs a forest needs: every array that has an element
int genetree_check_out(const ckm_genetree_args *a, const ckm_genetree_out *out, std::string &why) {
  const uint32_t T = a->ntrees, NG = a->group_off[T];
  if (!out || (a->class_off[3 * (uint64_t)T] && !out->consistency) || (a->gpair_off[NG] && !out->pair_flag) || (NG && (!out->group_node || !out->group_mixed))) {
    why = "NULL argument";
    return genetree::ARGS_INVALID;
  }
  return genetree::ARGS_OK;
}
}  // namespace ckm

extern "C" int ckm_genetree_check(const ckm_genetree_args *a) {
  return check_entry([&](std::string &why) { return genetree_check_args(a, why); });
}

extern "C" int ckm_genetree_host(const ckm_genetree_args *a, uint64_t budget_bytes, const ckm_genetree_out *out, ckm_genetree_info *info) {
  return check_entry([&](std::string &why) {
    int kind = genetree_check_args(a, why);
    if (kind == genetree::ARGS_OK) kind = genetree_check_out(a, out, why);
    if (kind == genetree::ARGS_OK) {
      uint64_t counts[2] = {0, 0};
      kind = genetree::run_host(genetree_args_of(a), batch_budget(budget_bytes, "CKM_GENETREE_BATCH_MB", 256),
                                genetree::Out{out->consistency, out->pair_flag, out->group_node, out->group_mixed}, counts, why);
      if (kind == genetree::ARGS_OK && info) { *info = ckm_genetree_info(); info->nrounds = counts[0]; info->ntrees = counts[1]; }
    }
    return kind;
  });
}
