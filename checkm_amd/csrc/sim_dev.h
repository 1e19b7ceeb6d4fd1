// sim_dev.h -- the data layout, the arithmetic and the round cuts of the marker-set simulation (scripts/simulation.py of the reference,
// worker :97-142; MarkerSetBuilder.containedMarkerGenes, scripts/genometreeworkflow/markerSetBuilder.py:353-369; MarkerSet.genomeCheck,
// checkm/markerSets.py:206-238), written once for the kernel (kernels_sim.hip), for the host executor of the CPU tests
// (tests/emu/simulation_emu.cpp) and for the stand-alone check.
//
// Keys, for the U distinct markers of all marker sets of a call:
//   key_off[U + 1]       first key of marker m; key_off[U] = all keys
//   key[..]              int32 start positions p[0] of the marker's copies in the test genome, each in [0, 2^31); any order
// Marker sets, S of them over the U markers: ms_off / cs_off / cs_marker, marker_sets.h's two-level CSR.
// Replicates, R of them:
//   rs_off[R + 1]        first contig start of replicate r
//   starts[..]           int32 contig starts, ascending within a replicate, duplicates allowed (contamination is drawn with replacement)
//   contig_len[R]        in [1, 2^31)
//
// A copy at p counts once for every start s with 0 <= p - s < contigLen:  ends_at(p) - ends_at(p - contigLen), ends_at(x) = starts <= x.
// p and contigLen are below 2^31, so p - contigLen fits int32.  A marker's count is the sum over its copies.
//
// Output: marker_sets.h's four float64 per (replicate, marker set), from the replicate's counts.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>
#include "marker_sets.h"
#include "wave_const.h"
#define SIM_HD SETS_HD

namespace ckm {
namespace sim {

using ckm::WAVE;
using ckm::ARGS_INVALID;
using ckm::ARGS_OK;
using ckm::ARGS_RANGE;
using msets::Individual;                            // marker_sets.h's, under the names the host executors have always used
using msets::set_terms;
using msets::finish;
constexpr int WAVES = 4;                            // wavefronts of a block; a block owns a replicate
constexpr int THREADS = WAVE * WAVES;
// LDS of a block: 24 KiB of starts and 16 KiB of counts = 40 KiB, four blocks (sixteen wavefronts) on a CU's 160 KiB.  6144 starts hold
// the largest draw of the reference's grid on a 5 Mb genome (1 kb contigs, completeness 1.0 plus contamination 0.2: 6000).
constexpr uint32_t STAGE_STARTS = 6144;             // starts of a replicate staged in LDS; a longer list is searched in global memory
constexpr uint32_t STAGE_COUNTS = 4096;             // marker counts kept in LDS; more markers keep them in a scratch row of global memory
constexpr uint32_t MAX_MARKERS = 1u << 24;          // U
constexpr uint32_t MAX_REPLICATES = 1u << 24;       // R
constexpr uint64_t MAX_KEYS = 0x7fffffffull;        // entries of key: key_off travels as uint32
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

// what the kernel takes by value (kernels_sim.hip, ckm_sim.hip)
struct SimDev {
  const uint32_t *key_off;      // [U + 1]
  const int32_t *key;
  msets::SetsDev sets;
  uint32_t U;
};

// ---- host side, shared by the library, the host executor and the stand-alone check ---------------------------------------------------------
struct Args {
  uint32_t nmarkers; const uint64_t *key_off; const int64_t *key;
  uint32_t nsets; const uint64_t *ms_off, *cs_off; const uint32_t *cs_marker;
  uint32_t nreplicates; const uint64_t *rs_off; const int64_t *starts, *contig_len;
};

// Why a call is refused.  No table is indexed before the offsets into it are known to be in order and within it: ncs and nmembers are
// what the caller's cs_off and cs_marker hold (the library's entries take them from the caller, the tables themselves cannot say).
inline int check(const Args &a, uint64_t ncs, uint64_t nmembers, uint64_t nkeys, uint64_t nstarts, std::string &why) {
  auto no = [&](int kind, const std::string &m) { why = m; return kind; };
  if (a.nmarkers > MAX_MARKERS) return no(ARGS_RANGE, "more than 2^24 markers");
  if (a.nsets > msets::MAX_SETS) return no(ARGS_RANGE, "more than 2^20 marker sets");
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
  if (const int kind = msets::check_marker_sets(a.nmarkers, a.nsets, a.ms_off, a.cs_off, a.cs_marker, ncs, nmembers, why)) return kind;
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

// The device's copies of the tables of a checked call: everything in 32 bits.
struct Packed : msets::Packed {                      // the marker sets, and with them:
  std::vector<uint32_t> key_off;
  std::vector<int32_t> key, contig_len;
  Packed() = default;
  Packed(const msets::Packed &sets) : msets::Packed(sets) {}      // marker sets alone, as a host executor written against sim::Packed reads them
};
inline void pack(const Args &a, Packed &P) {
  const uint64_t nkeys = a.key_off[a.nmarkers];
  P.key_off.resize((size_t)a.nmarkers + 1); P.key.resize(nkeys); P.contig_len.resize(a.nreplicates);
  for (uint32_t m = 0; m <= a.nmarkers; ++m) P.key_off[m] = (uint32_t)a.key_off[m];
  for (uint64_t k = 0; k < nkeys; ++k) P.key[k] = (int32_t)a.key[k];
  for (uint32_t r = 0; r < a.nreplicates; ++r) P.contig_len[r] = (int32_t)a.contig_len[r];
  msets::pack(a.nmarkers, a.nsets, a.ms_off, a.cs_off, a.cs_marker, P);
}

// what one replicate needs on the device during a round: its starts (simscaf_dev.h: the words of its bit rows), its output rows, and a scratch row of counts when they do not fit LDS
inline uint64_t replicate_bytes(uint64_t nstarts /* entries of 4 bytes */, uint32_t nmarkers, uint32_t nsets) {
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
