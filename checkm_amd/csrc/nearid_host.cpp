// nearid_host.cpp -- host side of the near-identity pass (additions to ABI 12): ckm_nearid_check, which says why a call would be refused
// and needs no device, and ckm_nearid_host, the host executor of nearid_dev.h behind the same arguments (what the stand-alone check and
// the tools' comparisons run).  Host code only.
#include <string>
#include "ckm_internal.h"
#include "nearid_dev.h"

using namespace ckm;

namespace ckm {
nearid::Args nearid_args_of(const ckm_nearid_args *a) { return nearid::Args{a->text, a->n_rows, a->row_len, a->row_stride, a->limit}; }
int nearid_check_args(const ckm_nearid_args *a, std::string &why) {
  if (!a) { why = "NULL argument"; return nearid::ARGS_INVALID; }
  return nearid::check(nearid_args_of(a), why);
}
}  // namespace ckm

extern "C" int ckm_nearid_check(const ckm_nearid_args *a) {
  return check_entry([&](std::string &why) { return nearid_check_args(a, why); });
}

extern "C" int ckm_nearid_host(const ckm_nearid_args *a, uint64_t budget_bytes, const ckm_nearid_out *out, ckm_nearid_info *info) {
  return check_entry([&](std::string &why) {
    int kind = nearid_check_args(a, why);
    if (kind == nearid::ARGS_OK && (!out || !out->near)) { why = "NULL argument"; kind = nearid::ARGS_INVALID; }
    if (kind == nearid::ARGS_OK) {
      uint64_t counts[2] = {0, 0};
      kind = nearid::run_host(nearid_args_of(a), batch_budget(budget_bytes, "CKM_NEARID_BATCH_MB", 256), out->near, counts, why);
      if (kind == nearid::ARGS_OK && info) { *info = ckm_nearid_info(); info->nbands = counts[0]; info->npairs = counts[1]; }
    }
    return kind;
  });
}
