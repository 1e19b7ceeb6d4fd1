// aai_host.cpp -- host side of the all-pairs amino-acid identity (additions to ABI 12): the argument tests of ckm_aai_run, which need no
// device.  The tests themselves, the packing and the batches are aai_dev.h's, shared with the host executor of the CPU tests.  Host code only.
#include <string>
#include "ckm_internal.h"
#include "aai_dev.h"

using namespace ckm;

extern "C" int ckm_aai_check(uint32_t ngroups, const uint64_t *group_row_off, const uint64_t *row_off, const char *text) {
  return check_entry([&](std::string &why) { return aai::check_args(ngroups, group_row_off, row_off, text, why); });
}
