// place_host.cpp -- host side of the phylogenetic placement (additions to ABI 12): ckm_place_check, which says why the tree, the
// alignment, the queries or the tables of a call would be refused, builds the level schedule of one that is not, and needs no device.
// The tests themselves and the schedule are place_dev.h's, shared with the host executor of the CPU tests and the stand-alone check.
// Host code only.
#include <string>
#include "ckm_internal.h"
#include "place_dev.h"

using namespace ckm;

namespace ckm {
place::Args place_args_of(const ckm_place_args *a) {
  return place::Args{a->nnodes, a->child_off, a->child, a->nchild, a->length, a->nsites, a->nrows, a->row_off, a->rows, a->nrow_bytes,
                     a->nqueries, a->q_off, a->queries, a->nquery_bytes, a->nrates, a->weights, a->U, a->Uinv, a->pi, a->exp_len, a->exp_half,
                     a->nfrac, a->exp_dist, a->npend, a->exp_pend, a->max_pitches};
}
int place_check_args(const ckm_place_args *a, place::Schedule &sch, std::string &why) {
  if (!a) { why = "NULL argument"; return place::ARGS_INVALID; }
  return place::check(place_args_of(a), sch, why);
}
}  // namespace ckm

extern "C" int ckm_place_check(const ckm_place_args *a) {
  return check_entry([&](std::string &why) {
    place::Schedule sch;
    return place_check_args(a, sch, why);
  });
}
