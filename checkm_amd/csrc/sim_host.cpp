// sim_host.cpp -- host side of the marker-set simulation (additions to ABI 12): ckm_sim_check, which says why the keys, the marker sets or
// the replicates of a call would be refused and needs no device.  The tests themselves, the packing and the round cuts are sim_dev.h's,
// shared with the host executor of the CPU tests and the stand-alone check.  Host code only.
#include <string>
#include "ckm_internal.h"
#include "sim_dev.h"

using namespace ckm;

namespace ckm {
int sim_check_args(const ckm_sim_args *a, std::string &why) {
  if (!a) { why = "NULL argument"; return sim::ARGS_INVALID; }
  const sim::Args A = {a->nmarkers, a->key_off, a->key, a->nsets, a->ms_off, a->cs_off, a->cs_marker, a->nreplicates, a->rs_off, a->starts, a->contig_len};
  return sim::check(A, a->ncs, a->nmembers, a->nkeys, a->nstarts, why);
}
}  // namespace ckm

extern "C" int ckm_sim_check(const ckm_sim_args *a) {
  return check_entry([&](std::string &why) { return sim_check_args(a, why); });
}
