// marker_sets.h -- the marker sets of a call, as the three passes that score them take them (sim_dev.h, simscaf_dev.h, select_dev.h):
// the layout, the check, the packing and MarkerSet.genomeCheck's arithmetic (checkm/markerSets.py:206-238), written once for the kernels
// (score_sets of sim_score.h), for the host executors of the CPU tests (tests/emu/score_sets_emu.h) and for the stand-alone checks.
//
// S marker sets over the U distinct markers of a call, each a list of co-located sets over marker indices (CSR in two levels):
//   ms_off[S + 1]        first co-located set of marker set s, into cs_off
//   cs_off[..+ 1]        first member of co-located set c, into cs_marker
//   cs_marker[..]        marker index < U.  A marker may sit in two co-located sets of one marker set: numMarkers() counts it twice, the
//                        individual mode of genomeCheck (which walks the SET getMarkerGenes()) once.  On the device a member that repeats
//                        an earlier member of its marker set carries REPEAT in its top bit (pack, host side).
//   num_markers[S]       numMarkers() of marker set s (device only)
//
// From a count per marker, four float64 per marker set, each in the reference's operation order (the library is built with
// -ffp-contract=off -fno-fast-math):
//   [0] 100 * float(present) / numMarkers        individual mode: present = distinct markers with count > 0
//   [1] 100 * float(multiCopy) / numMarkers      multiCopy = sum of count - 1 over those
//   [2] 100 * comp / nSets                       set mode: comp = sum in list order of float(present_c) / len(c)
//   [3] 100 * cont / nSets                       cont = sum in list order of float(multiCopy_c) / len(c)
#pragma once
#include <cstdint>
#include <string>
#include <vector>
#include "ckm_internal.h"
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SETS_HD __host__ __device__ __forceinline__
#else
#define SETS_HD inline
#endif

namespace ckm {
namespace msets {

using ckm::ARGS_INVALID;
using ckm::ARGS_OK;
using ckm::ARGS_RANGE;
constexpr uint32_t REPEAT = 0x80000000u;            // cs_marker on the device: this member repeats an earlier one of its marker set
constexpr uint32_t MAX_SETS = 1u << 20;             // S
constexpr uint64_t MAX_MEMBERS = 0x7fffffffull;     // entries of cs_marker, and of cs_off

// the marker sets on the device: everything in 32 bits, REPEAT marked
struct SetsDev {
  const uint32_t *ms_off;       // [S + 1]
  const uint32_t *cs_off, *cs_marker, *num_markers;
  uint32_t S;
};

// What a lane adds up for the individual mode: integers, so the order of the lanes does not matter.
struct Individual { uint32_t present; uint64_t multi; };

// One co-located set (members [e0, e1) of cs_marker, e1 > e0): the set mode's two quotients (:222-233), and the set's share of the
// individual mode from the members that do not repeat an earlier one.
SETS_HD void set_terms(const uint32_t *cs_marker, uint32_t e0, uint32_t e1, const uint32_t *counts, double &comp, double &cont, Individual &ind) {
  uint32_t present = 0;
  uint64_t multi = 0;
  for (uint32_t e = e0; e < e1; ++e) {
    const uint32_t m = cs_marker[e], count = counts[m & ~REPEAT];
    if (count == 0) continue;
    present += 1; multi += count - 1;
    if (!(m & REPEAT)) { ind.present += 1; ind.multi += count - 1; }
  }
  const double len = (double)(e1 - e0);
  comp = (double)present / len;
  cont = (double)multi / len;
}

// :216-217 and :235-236
SETS_HD void finish(const Individual &ind, uint32_t num_markers, double comp, double cont, uint32_t nsets, double *out) {
  out[0] = 100.0 * (double)ind.present / (double)num_markers;
  out[1] = 100.0 * (double)ind.multi / (double)num_markers;
  out[2] = 100.0 * comp / (double)nsets;
  out[3] = 100.0 * cont / (double)nsets;
}

// ---- host side, shared by the library, the host executors and the stand-alone checks -------------------------------------------------------
// The caller's tables (ms_off / cs_off / cs_marker over nmarkers markers; ncs and nmembers are what its cs_off and cs_marker hold):
// offsets in order and within their tables, no marker set without a co-located set, no co-located set without a member, every member a
// marker.  No table is indexed before the offsets into it are known to be in order and within it.
inline int check_marker_sets(uint32_t nmarkers, uint32_t nsets, const uint64_t *ms_off, const uint64_t *cs_off, const uint32_t *cs_marker, uint64_t ncs, uint64_t nmembers,
                             std::string &why) {
  auto no = [&](int kind, const std::string &m) { why = m; return kind; };
  if (nsets > MAX_SETS) return no(ARGS_RANGE, "more than 2^20 marker sets");
  if (!ms_off || !cs_off) return no(ARGS_INVALID, "NULL argument");
  if (ms_off[0] != 0) return no(ARGS_INVALID, "ms_off does not start at 0");
  for (uint32_t s = 0; s < nsets; ++s) {
    if (ms_off[s + 1] < ms_off[s]) return no(ARGS_INVALID, "ms_off falls at marker set " + std::to_string(s));
    if (ms_off[s + 1] > ncs) return no(ARGS_INVALID, "ms_off beyond the co-located sets at marker set " + std::to_string(s));
    if (ms_off[s + 1] == ms_off[s]) return no(ARGS_INVALID, "marker set " + std::to_string(s) + " has no sets");
  }
  const uint64_t used_cs = ms_off[nsets];
  if (used_cs > MAX_MEMBERS) return no(ARGS_RANGE, "more than 2^31 - 1 co-located sets");
  if (cs_off[0] != 0) return no(ARGS_INVALID, "cs_off does not start at 0");
  for (uint64_t c = 0; c < used_cs; ++c) {
    if (cs_off[c + 1] < cs_off[c]) return no(ARGS_INVALID, "cs_off falls at co-located set " + std::to_string(c));
    if (cs_off[c + 1] > nmembers) return no(ARGS_INVALID, "cs_off beyond the members at co-located set " + std::to_string(c));
    if (cs_off[c + 1] == cs_off[c]) return no(ARGS_INVALID, "co-located set " + std::to_string(c) + " is empty");
  }
  const uint64_t used_members = cs_off[used_cs];
  if (used_members > MAX_MEMBERS) return no(ARGS_RANGE, "more than 2^31 - 1 members of co-located sets");
  if (used_members && !cs_marker) return no(ARGS_INVALID, "NULL members");
  for (uint64_t e = 0; e < used_members; ++e)
    if (cs_marker[e] >= nmarkers) return no(ARGS_INVALID, "marker index " + std::to_string(cs_marker[e]) + " beyond the keys");
  return ARGS_OK;
}

// The device's copy of the marker sets of a checked call: SetsDev's four tables.
struct Packed {
  std::vector<uint32_t> ms_off, cs_off, cs_marker, num_markers;
};
inline void pack(uint32_t nmarkers, uint32_t nsets, const uint64_t *ms_off, const uint64_t *cs_off, const uint32_t *cs_marker, Packed &P) {
  const uint64_t ncs = ms_off[nsets], nmembers = cs_off[ncs];
  P.ms_off.resize((size_t)nsets + 1); P.cs_off.resize(ncs + 1); P.cs_marker.resize(nmembers);
  for (uint32_t s = 0; s <= nsets; ++s) P.ms_off[s] = (uint32_t)ms_off[s];
  for (uint64_t c = 0; c <= ncs; ++c) P.cs_off[c] = (uint32_t)cs_off[c];
  std::vector<uint32_t> seen(nmarkers, 0u);                                    // the marker set (+ 1) that met the marker last
  P.num_markers.assign(nsets, 0u);
  for (uint32_t s = 0; s < nsets; ++s)
    for (uint64_t e = cs_off[ms_off[s]]; e < cs_off[ms_off[s + 1]]; ++e) {
      const uint32_t m = cs_marker[e];
      P.cs_marker[e] = m | (seen[m] == s + 1 ? REPEAT : 0u);
      seen[m] = s + 1;
      P.num_markers[s] += 1;
    }
}

}  // namespace msets
}  // namespace ckm
