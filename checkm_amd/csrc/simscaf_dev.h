// simscaf_dev.h -- the data layout, the arithmetic and the round cuts of the scaffold simulation (scripts/simulationScaffoldsRandom.py and
// scripts/simulationScaffoldsByLength.py of the reference, workers :137-162; MarkerSetBuilder.markerGenesOnScaffolds,
// scripts/genometreeworkflow/markerSetBuilder.py:371-378; MarkerSet.genomeCheck, checkm/markerSets.py:206-238), written once for the kernel
// (kernels_simscaf.hip), for the host executor of the CPU tests (tests/emu/simscaf_emu.cpp) and for the stand-alone check.  The marker
// sets, their check, their packing and their scores are marker_sets.h's; the round cuts are sim_dev.h's.
//
// Resident, for G genomes and the U distinct markers of all marker sets of a call:
//   nscaf[G]             scaffolds of genome g
//   sc_off[G * U + 1]    first copy of cell (g, m) = g * U + m; sc_off[G * U] = all copies
//   sc[..]               uint32 scaffold index < nscaf[g], one entry per copy: two copies on one scaffold are two entries
//   ms_off, cs_off, cs_marker   the marker sets, marker_sets.h's two-level CSR
// Replicates, R of them:
//   test[R]              the test genome, < G
//   cont[R]              the contaminant, < G (it may be the test genome), or NONE
//   bit_off[R + 1]       first word of replicate r in bits
//   bits[..]             row_words(nscaf[test]) words, bit i of the row = scaffold i of the test genome is kept, then
//                        row_words(nscaf[cont]) words (none for NONE), bit i = scaffold i of the contaminant is sampled in.  Bits at and
//                        beyond nscaf are 0.
//
// A marker's count is the number of its copies in the test genome whose bit is set plus the same for the contaminant; the four float64 per
// (replicate, marker set) follow from the counts as in marker_sets.h.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>
#include "marker_sets.h"
#include "sim_dev.h"

namespace ckm {
namespace simscaf {

using sim::WAVE;
using sim::WAVES;
using sim::THREADS;
using sim::STAGE_COUNTS;
using sim::OUT_BYTES;
using sim::ARGS_OK;
using sim::ARGS_INVALID;
using sim::ARGS_RANGE;
using sim::next_round;                             // a replicate's 4-byte entries are the words of its bit rows
using sim::replicate_bytes;
// LDS of a block: two bit rows of 4 KiB and 16 KiB of counts = 24 KiB, six blocks (twenty-four wavefronts) on a CU's 160 KiB.
constexpr uint32_t STAGE_BITS = 32768;              // scaffolds of a bit row staged in LDS; a longer row is read from global memory
constexpr uint32_t STAGE_WORDS = STAGE_BITS / 32;
constexpr uint32_t NONE = 0xffffffffu;              // cont[r]: no contaminant
constexpr uint32_t MAX_GENOMES = 1u << 24;          // G
constexpr uint32_t MAX_SCAFFOLDS = 1u << 30;        // nscaf[g]
constexpr uint64_t MAX_CELLS = 1ull << 28;          // G * U: sc_off travels as uint32 [G * U + 1]
constexpr uint64_t MAX_COPIES = 0x7fffffffull;      // entries of sc

SIM_HD uint32_t row_words(uint32_t nscaf) { return (nscaf + 31u) / 32u; }
SIM_HD uint32_t bit_at(const uint32_t *row, uint32_t i) { return (row[i >> 5] >> (i & 31u)) & 1u; }
// markerGenesOnScaffolds :373-378 for one marker in one genome: the copies sc[k0 .. k1) whose scaffold's bit is set
SIM_HD uint32_t row_count(const uint32_t *sc, uint32_t k0, uint32_t k1, const uint32_t *row) {
  uint32_t c = 0;
  for (uint32_t k = k0; k < k1; ++k) c += bit_at(row, sc[k]);
  return c;
}

// what the kernel takes by value (kernels_simscaf.hip, ckm_simscaf.hip)
struct SimScafDev {
  const uint32_t *nscaf;        // [G]
  const uint32_t *sc_off;       // [G * U + 1]
  const uint32_t *sc;
  msets::SetsDev sets;
  uint32_t U;
};

// ---- host side, shared by the library, the host executor and the stand-alone check ---------------------------------------------------------
struct Args {
  uint32_t ngenomes; const uint32_t *nscaf;
  uint32_t nmarkers; const uint64_t *sc_off; const uint32_t *sc;
  uint32_t nsets; const uint64_t *ms_off, *cs_off; const uint32_t *cs_marker;
  uint32_t nreplicates; const uint32_t *test, *cont; const uint64_t *bit_off; const uint32_t *bits;
};

// Why a call is refused.  No table is indexed before the offsets into it are known to be in order and within it: nsc, ncs, nmembers and
// nwords are what the caller's sc, cs_off, cs_marker and bits hold.
inline int check(const Args &a, uint64_t nsc, uint64_t ncs, uint64_t nmembers, uint64_t nwords, std::string &why) {
  auto no = [&](int kind, const std::string &m) { why = m; return kind; };
  if (a.ngenomes > MAX_GENOMES) return no(ARGS_RANGE, "more than 2^24 genomes");
  if (a.nmarkers > sim::MAX_MARKERS) return no(ARGS_RANGE, "more than 2^24 markers");
  if (a.nreplicates > sim::MAX_REPLICATES) return no(ARGS_RANGE, "more than 2^24 replicates");
  const uint64_t ncells = (uint64_t)a.ngenomes * a.nmarkers;
  if (ncells > MAX_CELLS) return no(ARGS_RANGE, "more than 2^28 (genome, marker) cells");
  if (!a.sc_off || !a.bit_off || (a.ngenomes && !a.nscaf) || (a.nreplicates && (!a.test || !a.cont))) return no(ARGS_INVALID, "NULL argument");
  // scaffolds and copies
  for (uint32_t g = 0; g < a.ngenomes; ++g)
    if (a.nscaf[g] > MAX_SCAFFOLDS) return no(ARGS_RANGE, "more than 2^30 scaffolds in genome " + std::to_string(g));
  if (a.sc_off[0] != 0) return no(ARGS_INVALID, "sc_off does not start at 0");
  uint64_t max_copies = 0;
  for (uint64_t c = 0; c < ncells; ++c) {
    if (a.sc_off[c + 1] < a.sc_off[c]) return no(ARGS_INVALID, "sc_off falls at cell " + std::to_string(c));
    if (a.sc_off[c + 1] > nsc) return no(ARGS_INVALID, "sc_off beyond the copies at cell " + std::to_string(c));
    max_copies = std::max(max_copies, a.sc_off[c + 1] - a.sc_off[c]);
  }
  if (a.sc_off[ncells] > MAX_COPIES) return no(ARGS_RANGE, "more than 2^31 - 1 copies");
  if (a.sc_off[ncells] && !a.sc) return no(ARGS_INVALID, "NULL copies");
  if (2 * max_copies > sim::MAX_COUNT) return no(ARGS_RANGE, "copies of a marker in two genomes beyond 2^31 - 1");
  for (uint32_t g = 0; g < a.ngenomes; ++g)
    for (uint64_t k = a.sc_off[(uint64_t)g * a.nmarkers]; k < a.sc_off[(uint64_t)(g + 1) * a.nmarkers]; ++k)
      if (a.sc[k] >= a.nscaf[g]) return no(ARGS_INVALID, "scaffold index " + std::to_string(a.sc[k]) + " beyond the scaffolds of genome " + std::to_string(g));
  // marker sets
  if (const int kind = msets::check_marker_sets(a.nmarkers, a.nsets, a.ms_off, a.cs_off, a.cs_marker, ncs, nmembers, why)) return kind;
  // replicates
  if (a.bit_off[0] != 0) return no(ARGS_INVALID, "bit_off does not start at 0");
  for (uint32_t r = 0; r < a.nreplicates; ++r) {
    const uint32_t g = a.test[r], h = a.cont[r];
    if (g >= a.ngenomes) return no(ARGS_INVALID, "test genome of replicate " + std::to_string(r) + " beyond the genomes");
    if (h != NONE && h >= a.ngenomes) return no(ARGS_INVALID, "contaminant of replicate " + std::to_string(r) + " beyond the genomes");
    if (a.bit_off[r + 1] < a.bit_off[r]) return no(ARGS_INVALID, "bit_off falls at replicate " + std::to_string(r));
    if (a.bit_off[r + 1] > nwords) return no(ARGS_INVALID, "bit_off beyond the bits at replicate " + std::to_string(r));
    const uint32_t wt = row_words(a.nscaf[g]), wc = h == NONE ? 0u : row_words(a.nscaf[h]);
    if (a.bit_off[r + 1] - a.bit_off[r] != (uint64_t)wt + wc) return no(ARGS_INVALID, "the bit rows of replicate " + std::to_string(r) + " have the wrong length");
    if (a.bit_off[r + 1] && !a.bits) return no(ARGS_INVALID, "NULL bits");
    const uint32_t *row = a.bits + a.bit_off[r];
    const uint32_t tail_t = a.nscaf[g] & 31u, tail_c = h == NONE ? 0u : a.nscaf[h] & 31u;
    if (tail_t && (row[wt - 1] >> tail_t)) return no(ARGS_INVALID, "bits beyond the scaffolds of the test genome in replicate " + std::to_string(r));
    if (tail_c && (row[wt + wc - 1] >> tail_c)) return no(ARGS_INVALID, "bits beyond the scaffolds of the contaminant in replicate " + std::to_string(r));
  }
  return ARGS_OK;
}

// The device's copies of the resident tables of a checked call: everything in 32 bits.
struct Packed {
  std::vector<uint32_t> sc_off;
  msets::Packed sets;
};
inline void pack(const Args &a, Packed &P) {
  const uint64_t ncells = (uint64_t)a.ngenomes * a.nmarkers;
  P.sc_off.resize(ncells + 1);
  for (uint64_t c = 0; c <= ncells; ++c) P.sc_off[c] = (uint32_t)a.sc_off[c];
  msets::pack(a.nmarkers, a.nsets, a.ms_off, a.cs_off, a.cs_marker, P.sets);
}

}  // namespace simscaf
}  // namespace ckm
