// sim_dev.h -- the data layout, the arithmetic and the round cuts of the marker-set simulation (scripts/simulation.py of the reference,
// worker :97-142; MarkerSetBuilder.containedMarkerGenes, scripts/genometreeworkflow/markerSetBuilder.py:353-369; MarkerSet.genomeCheck,
// checkm/markerSets.py:206-238), written once for the kernel (kernels_sim.hip), for the host executor of the CPU tests
// (tests/emu/simulation_emu.cpp) and for the stand-alone check.
//
// Keys, for the U distinct markers of all marker sets of a call:
//   key_off[U + 1]       first key of marker m; key_off[U] = all keys
//   key[..]              int32 start positions p[0] of the marker's copies in the test genome, each in [0, 2^31); any order
// Marker sets, S of them, each a list of co-located sets over marker indices (CSR in two levels):
//   ms_off[S + 1]        first co-located set of marker set s, into cs_off
//   cs_off[..+ 1]        first member of co-located set c, into cs_marker
//   cs_marker[..]        marker index < U.  A marker may sit in two co-located sets of one marker set: numMarkers() counts it twice, the
//                        individual mode of genomeCheck (which walks the SET getMarkerGenes()) once.  On the device a member that repeats
//                        an earlier member of its marker set carries REPEAT in its top bit (mark_repeats, host side).
// Replicates, R of them:
//   rs_off[R + 1]        first contig start of replicate r
//   starts[..]           int32 contig starts, ascending within a replicate, duplicates allowed (contamination is drawn with replacement)
//   contig_len[R]        in [1, 2^31)
//
// A copy at p counts once for every start s with 0 <= p - s < contigLen:  ends_at(p) - ends_at(p - contigLen), ends_at(x) = starts <= x.
// p and contigLen are below 2^31, so p - contigLen fits int32.  A marker's count is the sum over its copies.
//
// Output, four float64 per (replicate, marker set), each in the reference's operation order (the library is built with
// -ffp-contract=off -fno-fast-math):
//   [0] 100 * float(present) / numMarkers        individual mode: present = distinct markers with count > 0
//   [1] 100 * float(multiCopy) / numMarkers      multiCopy = sum of count - 1 over those
//   [2] 100 * comp / nSets                       set mode: comp = sum in list order of float(present_c) / len(c)
//   [3] 100 * cont / nSets                       cont = sum in list order of float(multiCopy_c) / len(c)
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>
#include "wave_const.h"
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SIM_HD __host__ __device__ __forceinline__
#else
#define SIM_HD inline
#endif

namespace ckm {
namespace sim {

using ckm::WAVE;
constexpr int WAVES = 4;                            // wavefronts of a block; a block owns a replicate
constexpr int THREADS = WAVE * WAVES;
// LDS of a block: 24 KiB of starts and 16 KiB of counts = 40 KiB, four blocks (sixteen wavefronts) on a CU's 160 KiB.  6144 starts hold
// the largest draw of the reference's grid on a 5 Mb genome (1 kb contigs, completeness 1.0 plus contamination 0.2: 6000).
constexpr uint32_t STAGE_STARTS = 6144;             // starts of a replicate staged in LDS; a longer list is searched in global memory
constexpr uint32_t STAGE_COUNTS = 4096;             // marker counts kept in LDS; more markers keep them in a scratch row of global memory
constexpr uint32_t REPEAT = 0x80000000u;            // cs_marker on the device: this member repeats an earlier one of its marker set
constexpr uint32_t MAX_MARKERS = 1u << 24;          // U
constexpr uint32_t MAX_SETS = 1u << 20;             // S
constexpr uint32_t MAX_REPLICATES = 1u << 24;       // R
constexpr uint64_t MAX_KEYS = 0x7fffffffull;        // entries of key: key_off travels as uint32
constexpr uint64_t MAX_MEMBERS = 0x7fffffffull;     // entries of cs_marker, and of cs_off
constexpr uint64_t MAX_COUNT = 0x7fffffffull;       // copies of a marker x starts of a replicate: a count stays exact in uint32
constexpr uint32_t ROUND_REPLICATES = 1u << 20;     // blocks of one launch
constexpr uint32_t OUT_BYTES = 32;                  // four float64 per (replicate, marker set)

// starts[0 .. n) <= x
SIM_HD uint32_t ends_at(const int32_t *starts, uint32_t n, int32_t x) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (starts[mid] <= x) lo = mid + 1; else hi = mid;
  }
  return lo;
}
// the starts s with 0 <= p - s < contig_len
SIM_HD uint32_t copy_count(const int32_t *starts, uint32_t n, int32_t p, int32_t contig_len) {
  return ends_at(starts, n, p) - ends_at(starts, n, p - contig_len);
}
// containedMarkerGenes :357-367 for one marker: len(containedPos)
SIM_HD uint32_t marker_count(const int32_t *key, uint32_t k0, uint32_t k1, const int32_t *starts, uint32_t n, int32_t contig_len) {
  uint32_t c = 0;
  for (uint32_t k = k0; k < k1; ++k) c += copy_count(starts, n, key[k], contig_len);
  return c;
}

// What a lane adds up for the individual mode: integers, so the order of the lanes does not matter.
struct Individual { uint32_t present; uint64_t multi; };

// One co-located set (members [e0, e1) of cs_marker, e1 > e0): the set mode's two quotients (:222-233), and the set's share of the
// individual mode from the members that do not repeat an earlier one.
SIM_HD void set_terms(const uint32_t *cs_marker, uint32_t e0, uint32_t e1, const uint32_t *counts, double &comp, double &cont, Individual &ind) {
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
SIM_HD void finish(const Individual &ind, uint32_t num_markers, double comp, double cont, uint32_t nsets, double *out) {
  out[0] = 100.0 * (double)ind.present / (double)num_markers;
  out[1] = 100.0 * (double)ind.multi / (double)num_markers;
  out[2] = 100.0 * comp / (double)nsets;
  out[3] = 100.0 * cont / (double)nsets;
}

// ---- host side, shared by the library, the host executor and the stand-alone check ---------------------------------------------------------
enum { ARGS_OK = 0, ARGS_INVALID = 1, ARGS_RANGE = 2 };

struct Args {
  uint32_t nmarkers; const uint64_t *key_off; const int64_t *key;
  uint32_t nsets; const uint64_t *ms_off, *cs_off; const uint32_t *cs_marker;
  uint32_t nreplicates; const uint64_t *rs_off; const int64_t *starts, *contig_len;
};

// The marker sets of a call (ms_off / cs_off / cs_marker over nmarkers markers): offsets in order and within their tables, no marker set
// without a co-located set, no co-located set without a member, every member a marker.  Shared with simscaf_dev.h.
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

// Why a call is refused.  No table is indexed before the offsets into it are known to be in order and within it: ncs and nmembers are
// what the caller's cs_off and cs_marker hold (the library's entries take them from the caller, the tables themselves cannot say).
inline int check(const Args &a, uint64_t ncs, uint64_t nmembers, uint64_t nkeys, uint64_t nstarts, std::string &why) {
  auto no = [&](int kind, const std::string &m) { why = m; return kind; };
  if (a.nmarkers > MAX_MARKERS) return no(ARGS_RANGE, "more than 2^24 markers");
  if (a.nsets > MAX_SETS) return no(ARGS_RANGE, "more than 2^20 marker sets");
  if (a.nreplicates > MAX_REPLICATES) return no(ARGS_RANGE, "more than 2^24 replicates");
  if (!a.key_off || !a.ms_off || !a.cs_off || !a.rs_off || (a.nreplicates && !a.contig_len)) return no(ARGS_INVALID, "NULL argument");
  // keys
  if (a.key_off[0] != 0) return no(ARGS_INVALID, "key_off does not start at 0");
  uint64_t max_copies = 0;
  for (uint32_t m = 0; m < a.nmarkers; ++m) {
    if (a.key_off[m + 1] < a.key_off[m]) return no(ARGS_INVALID, "key_off falls at marker " + std::to_string(m));
    if (a.key_off[m + 1] > nkeys) return no(ARGS_INVALID, "key_off beyond the keys at marker " + std::to_string(m));
    max_copies = std::max(max_copies, a.key_off[m + 1] - a.key_off[m]);
  }
  if (a.key_off[a.nmarkers] > MAX_KEYS) return no(ARGS_RANGE, "more than 2^31 - 1 keys");
  if (a.key_off[a.nmarkers] && !a.key) return no(ARGS_INVALID, "NULL keys");
  for (uint64_t k = 0; k < a.key_off[a.nmarkers]; ++k)
    if (a.key[k] < 0 || a.key[k] > 2147483647ll) return no(ARGS_RANGE, "key " + std::to_string(a.key[k]) + " does not fit int32");
  // marker sets
  if (const int kind = check_marker_sets(a.nmarkers, a.nsets, a.ms_off, a.cs_off, a.cs_marker, ncs, nmembers, why)) return kind;
  // replicates
  if (a.rs_off[0] != 0) return no(ARGS_INVALID, "rs_off does not start at 0");
  uint64_t max_starts = 0;
  for (uint32_t r = 0; r < a.nreplicates; ++r) {
    if (a.rs_off[r + 1] < a.rs_off[r]) return no(ARGS_INVALID, "rs_off falls at replicate " + std::to_string(r));
    if (a.rs_off[r + 1] > nstarts) return no(ARGS_INVALID, "rs_off beyond the starts at replicate " + std::to_string(r));
    max_starts = std::max(max_starts, a.rs_off[r + 1] - a.rs_off[r]);
    if (a.contig_len[r] < 1 || a.contig_len[r] > 2147483647ll) return no(ARGS_RANGE, "contigLen " + std::to_string(a.contig_len[r]) + " outside [1, 2^31)");
  }
  if (a.rs_off[a.nreplicates] && !a.starts) return no(ARGS_INVALID, "NULL starts");
  for (uint32_t r = 0; r < a.nreplicates; ++r)
    for (uint64_t k = a.rs_off[r]; k < a.rs_off[r + 1]; ++k) {
      if (a.starts[k] < 0 || a.starts[k] > 2147483647ll) return no(ARGS_RANGE, "start " + std::to_string(a.starts[k]) + " does not fit int32");
      if (k > a.rs_off[r] && a.starts[k] < a.starts[k - 1]) return no(ARGS_INVALID, "the starts of replicate " + std::to_string(r) + " are not ascending");
    }
  if (max_copies * max_starts > MAX_COUNT) return no(ARGS_RANGE, "copies of a marker times starts of a replicate beyond 2^31 - 1");
  return ARGS_OK;
}

// The device's copies of the tables of a checked call: everything in 32 bits, the repeats marked.
struct Packed {
  std::vector<uint32_t> key_off, ms_off, cs_off, cs_marker, num_markers;      // num_markers[s]: numMarkers() of marker set s
  std::vector<int32_t> key, contig_len;
};
inline void mark_repeats(const Args &a, Packed &P) {
  std::vector<uint32_t> seen(a.nmarkers, 0u);                                  // the marker set (+ 1) that met the marker last
  P.num_markers.assign(a.nsets, 0u);
  for (uint32_t s = 0; s < a.nsets; ++s)
    for (uint64_t e = a.cs_off[a.ms_off[s]]; e < a.cs_off[a.ms_off[s + 1]]; ++e) {
      const uint32_t m = a.cs_marker[e];
      P.cs_marker[e] = m | (seen[m] == s + 1 ? REPEAT : 0u);
      seen[m] = s + 1;
      P.num_markers[s] += 1;
    }
}
inline void pack(const Args &a, Packed &P) {
  const uint64_t ncs = a.ms_off[a.nsets], nmembers = a.cs_off[ncs], nkeys = a.key_off[a.nmarkers];
  P.key_off.resize((size_t)a.nmarkers + 1); P.ms_off.resize((size_t)a.nsets + 1); P.cs_off.resize(ncs + 1); P.cs_marker.resize(nmembers);
  P.key.resize(nkeys); P.contig_len.resize(a.nreplicates);
  for (uint32_t m = 0; m <= a.nmarkers; ++m) P.key_off[m] = (uint32_t)a.key_off[m];
  for (uint32_t s = 0; s <= a.nsets; ++s) P.ms_off[s] = (uint32_t)a.ms_off[s];
  for (uint64_t c = 0; c <= ncs; ++c) P.cs_off[c] = (uint32_t)a.cs_off[c];
  for (uint64_t k = 0; k < nkeys; ++k) P.key[k] = (int32_t)a.key[k];
  for (uint32_t r = 0; r < a.nreplicates; ++r) P.contig_len[r] = (int32_t)a.contig_len[r];
  mark_repeats(a, P);
}

// what one replicate needs on the device during a round: its starts, its output rows, and a scratch row of counts when they do not fit LDS
inline uint64_t replicate_bytes(uint64_t nstarts, uint32_t nmarkers, uint32_t nsets) {
  return nstarts * 4 + (uint64_t)nsets * OUT_BYTES + (nmarkers > STAGE_COUNTS ? (uint64_t)nmarkers * 4 : 0);
}
// A round: replicates [r0, r1) that fit budget_bytes -- always at least one, never more than ROUND_REPLICATES.  Returns r1.
inline uint32_t next_round(uint32_t nreplicates, const uint64_t *rs_off, uint32_t nmarkers, uint32_t nsets, uint64_t budget_bytes, uint32_t r0) {
  uint64_t bytes = 0;
  uint32_t r = r0;
  for (; r < nreplicates && r - r0 < ROUND_REPLICATES; ++r) {
    const uint64_t b = replicate_bytes(rs_off[r + 1] - rs_off[r], nmarkers, nsets);
    if (r > r0 && bytes + b > budget_bytes) break;
    bytes += b;
  }
  return r;
}

}  // namespace sim
}  // namespace ckm
