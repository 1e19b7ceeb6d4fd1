// select_host.cpp -- host side of the marker-set selection (additions to ABI 12): ckm_select_check, which says why the genomes, the keys,
// the marker sets or the ranges of a call would be refused and needs no device.  The tests themselves, the packing and the round cuts are
// select_dev.h's, shared with the host executor of the CPU tests and the stand-alone check.  Host code only.
#include <string>
#include "ckm_internal.h"
#include "select_dev.h"

using namespace ckm;

namespace ckm {
sel::Args select_args_of(const ckm_select_args *a) {
  return sel::Args{a->ngenomes, a->genome_len, a->nmarkers, a->key_off, a->key, a->nsets, a->ms_off, a->cs_off, a->cs_marker,
                   a->nreplicates, a->contig_len, a->comp_lo, a->comp_hi, a->cont_lo, a->cont_hi, a->seed};
}
int select_check_args(const ckm_select_args *a, std::string &why) {
  if (!a) { why = "NULL argument"; return sim::ARGS_INVALID; }
  return sel::check(select_args_of(a), a->ncs, a->nmembers, a->nkeys, why);
}
}  // namespace ckm

extern "C" int ckm_select_check(const ckm_select_args *a) {
  return check_entry([&](std::string &why) { return select_check_args(a, why); });
}
