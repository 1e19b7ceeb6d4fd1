// simscaf_host.cpp -- host side of the scaffold simulation (additions to ABI 12): ckm_simscaf_check, which says why the resident tables, the
// marker sets or the replicates of a call would be refused and needs no device.  The tests themselves, the packing and the round cuts are
// simscaf_dev.h's, shared with the host executor of the CPU tests and the stand-alone check.  Host code only.
#include <string>
#include "ckm_internal.h"
#include "simscaf_dev.h"

using namespace ckm;

namespace ckm {
int simscaf_check_args(const ckm_simscaf_args *a, std::string &why) {
  if (!a) { why = "NULL argument"; return simscaf::ARGS_INVALID; }
  const simscaf::Args A = {a->ngenomes, a->nscaf, a->nmarkers, a->sc_off, a->sc, a->nsets, a->ms_off, a->cs_off, a->cs_marker,
                           a->nreplicates, a->test, a->cont, a->bit_off, a->bits};
  return simscaf::check(A, a->nsc, a->ncs, a->nmembers, a->nwords, why);
}
}  // namespace ckm

extern "C" int ckm_simscaf_check(const ckm_simscaf_args *a) {
  return check_entry([&](std::string &why) { return simscaf_check_args(a, why); });
}
