// aai_host.cpp -- host side of the all-pairs amino-acid identity (additions to ABI 12): the argument tests of ckm_aai_run, which need no
// device.  The tests themselves, the packing and the batches are aai_dev.h's, shared with the host executor of the CPU tests.  Host code only.
#include <string>
#include "ckm_internal.h"
#include "aai_dev.h"

using namespace ckm;

extern "C" int ckm_aai_check(uint32_t ngroups, const uint64_t *group_row_off, const uint64_t *row_off, const char *text) {
  try {
    std::string why;
    const int kind = aai::check_args(ngroups, group_row_off, row_off, text, why);
    if (kind == aai::ARGS_OK) return CKM_OK;
    set_last_error(why);
    return kind == aai::ARGS_RANGE ? CKM_ERANGE : CKM_EINVAL;
  } catch (const std::bad_alloc &) { set_last_error("out of host memory"); return CKM_ENOMEM; }
}
