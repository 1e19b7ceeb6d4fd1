// nhmm_host.cpp -- host side of the nucleotide model scan (additions to ABI 12): ckm_nhmm_check, which says why the models, the
// thresholds or the tile geometry of a call would be refused and needs no device, and the columns of a result.  The tests themselves are
// nhmm_dev.h's, shared with the host executor of the CPU tests and the stand-alone check.  Host code only.
#include <string>
#include "ckm_internal.h"
#include "nhmm_dev.h"

using namespace ckm;

namespace ckm {
nhmm::Args nhmm_args_of(const ckm_nhmm_args *a) {
  return nhmm::Args{a->nmodels, a->M, a->tab_off, a->emis, a->trans, a->ntab, a->min_score, a->stride, a->overlap, a->strands};
}
int nhmm_check_args(const ckm_nhmm_args *a, std::string &why) {
  if (!a) { why = "NULL argument"; return nhmm::ARGS_INVALID; }
  return nhmm::check(nhmm_args_of(a), why);
}
}  // namespace ckm

extern "C" int ckm_nhmm_check(const ckm_nhmm_args *a) {
  return check_entry([&](std::string &why) { return nhmm_check_args(a, why); });
}

extern "C" int ckm_nhmm_columns_get(const ckm_nhmm_result *r, ckm_nhmm_columns *out) {
  if (!r || !out) { set_last_error("NULL argument"); return CKM_EINVAL; }
  const nhmm::Rows &w = r->rows;
  const nhmm::Hits &h = r->hits;
  *out = ckm_nhmm_columns{w.size(), w.model.data(), w.seq.data(), w.strand.data(), w.pos.data(), w.start.data(), w.score.data(),
                          h.size(), h.model.data(), h.seq.data(), h.strand.data(), h.from.data(), h.to.data(), h.score.data()};
  return CKM_OK;
}

extern "C" void ckm_nhmm_free(ckm_nhmm_result *r) { delete r; }
