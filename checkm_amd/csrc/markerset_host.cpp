// markerset_host.cpp -- host side of MarkerSetBuilder (additions to ABI 12): ckm_mset_check, which says why a table, the queries of a call
// or a distance threshold would be refused and needs no device.  The tests themselves, the rounds, the tile lists and the output batches
// are markerset_dev.h's, shared with the host executor of the CPU tests and the stand-alone check.  Host code only.
#include <string>
#include "ckm_internal.h"
#include "markerset_dev.h"

using namespace ckm;

extern "C" int ckm_mset_check(uint32_t ngenomes, uint32_t nfamilies, const uint8_t *count_class, const uint64_t *pos_off, const int64_t *pos, uint32_t nqueries,
                              const uint64_t *qg_off, const uint32_t *qg, const uint64_t *qm_off, const uint32_t *qm, double dist_threshold) {
  return check_entry([&](std::string &why) {
    int kind = ms::check_dist(dist_threshold, why);
    if (kind == ms::ARGS_OK) kind = ms::check_table(ngenomes, nfamilies, count_class, pos_off, pos, why);
    if (kind == ms::ARGS_OK && (nqueries || qg_off)) kind = ms::check_queries(ngenomes, nfamilies, nqueries, qg_off, qg, qm_off, qm, why);
    return kind;
  });
}
