// select_dev.h -- the data layout, the generator, the draw and the round cuts of the marker-set selection (scripts/simInferBestMarkerSet.py
// of the reference, __selectMarkerSet :89-110: per replicate random.uniform twice, MarkerSetBuilder.sampleGenome,
// scripts/genometreeworkflow/markerSetBuilder.py:265-289, then containedMarkerGenes and MarkerSet.genomeCheck for every set of the chain),
// written once for the kernel (kernels_select.hip), for the host executor of the CPU tests (tests/emu/selection_emu.cpp) and for the
// stand-alone check.  The draws are made where they are scored: nothing of a draw but its results leaves the device.
//
// A call covers the G test genomes of one node, R replicates each:
//   genome_len[G]            bases of genome g; C_g = genome_len[g] / contig_len contigs (integer quotient), 1 <= C_g <= MAX_CONTIGS
//   key_off[G * U + 1]       first key of cell (g, m) = g * U + m
//   key[..]                  int32 start positions p[0] of the copies of marker m in genome g, each in [0, 2^31); any order
//   ms_off / cs_off / cs_marker   the S marker sets over the U markers, marker_sets.h's two-level CSR (its check, its packing, its scores)
//   contig_len, comp_lo, comp_hi, cont_lo, cont_hi, seed
//
// Generator: Philox4x32-10 (Salmon et al., SC'11) in plain 32-bit integers.  Key = (seed low half, seed high half), counter =
// (index, replicate, genome, stream): every word a draw uses is a function of the call's arguments alone, never of the launch shape.
//
// Draw (g, r):
//   stream FRAC, index 0     u0 from words 0 and 1, u1 from words 2 and 3: u = ((w >> 5) * 2^26 + (w' >> 6)) * 2^-53, in [0, 1)
//                            testComp = comp_lo + (comp_hi - comp_lo) * u0, testCont likewise from u1 (random.uniform's formula)
//                            nComp = (int)(C * testComp + 0.5), nCont = (int)(C * testCont + 0.5)
//                            trueComp = (double)nComp * contig_len * 100 / genome_len, trueCont likewise
//                            comp_hi <= 1 keeps nComp <= C: C * (1 + 2^-52) + 0.5 < C + 1 for every C <= MAX_CONTIGS.
//   stream COMP              contig i gets word i % 4 of index i / 4; it is taken iff (w_i, i) is among the nComp smallest pairs in
//                            lexicographic order -- a uniform random subset, whichever way the threshold pair is found
//   stream CONT              draw j (word j % 4 of index j / 4) lands on contig ((uint64)w_j * C) >> 32; a contig's probability is off
//                            1 / C by at most 2^-32 (the multiply-high's bias, at most C / 2^32 relative)
//   mult[c]                  times contig c was drawn, both kinds together
//   A copy at p counts mult[p / contig_len] when p / contig_len < C, else 0 (the genome's partial tail and what lies beyond it are in
//   no contig): what containedMarkerGenes gives for the starts c * contig_len.  A marker's count is the sum over its copies.
//
// Output per draw: trueComp and trueCont; four float64 per marker set (marker_sets.h's, in the reference's operation order); on request the
// row mult[0 .. C_g) as uint16, genome g's rows at row_off[g] = sum over h < g of R * C_h.  A row entry is min(mult, 65535): nCont <=
// MAX_CONT_DRAWS and one completeness draw could exceed it only with every contamination draw on one contig.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>
#include "marker_sets.h"
#include "sim_dev.h"

namespace ckm {
namespace sel {

using ckm::WAVE;
using sim::ARGS_INVALID;
using sim::ARGS_OK;
using sim::ARGS_RANGE;
using sim::STAGE_COUNTS;
using sim::THREADS;
using sim::WAVES;
// LDS of a block: one uint32 multiplicity per contig (the target of ds_add_u32; during the selection the same word holds the contig's
// random word), sized by the call's largest genome, beside sim_dev.h's 16 KiB of marker counts and a 1 KiB histogram.  16384 contigs
// hold the 1 kb contigs of Simulation's grid on a 15 Mb genome (15000) and make 64 + 17 = 81 KiB, one block short of two per CU's
// 160 KiB; the selection's own draws (10 kb contigs, a few hundred of them) take 2 KiB and leave the CU's wavefront slots the limit.
constexpr uint32_t MAX_CONTIGS = 16384;
constexpr uint32_t MAX_CONT_DRAWS = 65535;          // nCont
constexpr uint32_t MAX_GENOMES = 1u << 24;          // G
constexpr uint32_t MAX_REPLICATES = 1u << 24;       // R
constexpr uint64_t MAX_DRAWS = 0x7fffffffull;       // G * R
constexpr uint64_t MAX_COUNT = 0xffffffffull;       // copies of a marker x (nCont + 1): a count stays exact in uint32
constexpr uint32_t ROUND_DRAWS = 1u << 20;          // blocks of one launch
constexpr uint32_t BINS = 256;                      // a radix pass looks at 8 bits
constexpr int PASSES = 6;                           // of the pair (w, i): four over the word, two over the contig index (< 2^16)
enum : uint32_t { STREAM_FRAC = 0, STREAM_COMP = 1, STREAM_CONT = 2 };
static_assert(MAX_CONTIGS <= 65536, "the contig index takes two radix passes");

// ---- Philox4x32-10 -------------------------------------------------------------------------------------------------------------------------
struct Words { uint32_t w[4]; };
SIM_HD Words philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return Words{{c0, c1, c2, c3}};
}
SIM_HD Words words_of(uint64_t seed, uint32_t stream, uint32_t genome, uint32_t replicate, uint32_t index) {
  return philox(index, replicate, genome, stream, (uint32_t)seed, (uint32_t)(seed >> 32));
}
// 53 bits of two words, as random.random() takes them from two words of its own generator
SIM_HD double unit(uint32_t a, uint32_t b) {
  return (double)(((uint64_t)(a >> 5) << 26) | (uint64_t)(b >> 6)) * (1.0 / 9007199254740992.0);
}

// ---- the draw ----------------------------------------------------------------------------------------------------------------------------
struct Params { int32_t contig_len; double comp_lo, comp_hi, cont_lo, cont_hi; uint64_t seed; };
struct Plan { uint32_t ncomp, ncont; double true_comp, true_cont; };

SIM_HD double fraction(double lo, double hi, double u) { return lo + (hi - lo) * u; }
SIM_HD uint32_t rounded(uint32_t C, double fraction_) { return (uint32_t)(int64_t)((double)C * fraction_ + 0.5); }
SIM_HD double true_percent(uint32_t n, int32_t contig_len, int64_t genome_len) { return (double)n * (double)contig_len * 100.0 / (double)genome_len; }
SIM_HD Plan plan_of(const Params &P, int64_t genome_len, uint32_t C, uint32_t genome, uint32_t replicate) {
  const Words f = words_of(P.seed, STREAM_FRAC, genome, replicate, 0);
  Plan d;
  d.ncomp = rounded(C, fraction(P.comp_lo, P.comp_hi, unit(f.w[0], f.w[1])));
  d.ncont = rounded(C, fraction(P.cont_lo, P.cont_hi, unit(f.w[2], f.w[3])));
  d.true_comp = true_percent(d.ncomp, P.contig_len, genome_len);
  d.true_cont = true_percent(d.ncont, P.contig_len, genome_len);
  return d;
}
// the pair (w_i, i) as one number: pairs compare as their numbers do, and no two are equal
SIM_HD uint64_t pair_of(uint32_t w, uint32_t i) { return ((uint64_t)w << 32) | i; }
// radix pass p: the digit's shift, and the bits above the digit (what the passes before have fixed)
SIM_HD int pass_shift(int p) { return p < 4 ? 56 - 8 * p : 8 * (5 - p); }
SIM_HD uint64_t pass_above(int p) { return p == 0 ? 0ull : ~((1ull << (pass_shift(p) + 8)) - 1); }
// where contamination draw word w lands
SIM_HD uint32_t landing(uint32_t w, uint32_t C) { return (uint32_t)(((uint64_t)w * C) >> 32); }
// what a copy at p counts
SIM_HD uint32_t copy_mult(const uint32_t *mult, uint32_t C, int32_t p, int32_t contig_len) {
  const uint32_t c = (uint32_t)p / (uint32_t)contig_len;
  return c < C ? mult[c] : 0u;
}
SIM_HD uint32_t marker_mult(const int32_t *key, uint32_t k0, uint32_t k1, const uint32_t *mult, uint32_t C, int32_t contig_len) {
  uint32_t n = 0;
  for (uint32_t k = k0; k < k1; ++k) n += copy_mult(mult, C, key[k], contig_len);
  return n;
}
SIM_HD uint16_t row_entry(uint32_t mult) { return (uint16_t)(mult < 65535u ? mult : 65535u); }

// what the kernel takes by value (kernels_select.hip, ckm_select.hip)
struct SelectDev {
  const int64_t *genome_len;    // [G]
  const uint32_t *ncontigs;     // [G]
  const uint64_t *row_off;      // [G + 1]
  const uint32_t *key_off;      // [G * U + 1]
  const int32_t *key;
  msets::SetsDev sets;
  uint32_t U, R;
  Params P;
};

// ---- host side, shared by the library, the host executor and the stand-alone check ---------------------------------------------------------
struct Args {
  uint32_t ngenomes; const int64_t *genome_len;
  uint32_t nmarkers; const uint64_t *key_off; const int64_t *key;
  uint32_t nsets; const uint64_t *ms_off, *cs_off; const uint32_t *cs_marker;
  uint32_t nreplicates; int64_t contig_len; double comp_lo, comp_hi, cont_lo, cont_hi; uint64_t seed;
};

// the largest fraction a range can give: u < 1, and the product and the sum round monotonically
inline double top_fraction(double lo, double hi) { return fraction(lo, hi, 1.0 - 1.0 / 9007199254740992.0); }

// Why a call is refused.  No table is indexed before the offsets into it are known to be in order and within it: ncs, nmembers and nkeys
// are what the caller's cs_off, cs_marker and key hold.
inline int check(const Args &a, uint64_t ncs, uint64_t nmembers, uint64_t nkeys, std::string &why) {
  auto no = [&](int kind, const std::string &m) { why = m; return kind; };
  if (a.ngenomes > MAX_GENOMES) return no(ARGS_RANGE, "more than 2^24 genomes");
  if (a.nmarkers > sim::MAX_MARKERS) return no(ARGS_RANGE, "more than 2^24 markers");
  if (a.nsets > msets::MAX_SETS) return no(ARGS_RANGE, "more than 2^20 marker sets");
  if (a.nreplicates > MAX_REPLICATES) return no(ARGS_RANGE, "more than 2^24 replicates");
  if ((uint64_t)a.ngenomes * a.nreplicates > MAX_DRAWS) return no(ARGS_RANGE, "more than 2^31 - 1 draws");
  if (!a.key_off || !a.ms_off || !a.cs_off || (a.ngenomes && !a.genome_len)) return no(ARGS_INVALID, "NULL argument");
  if (a.contig_len < 1 || a.contig_len > 2147483647ll) return no(ARGS_RANGE, "contigLen " + std::to_string(a.contig_len) + " outside [1, 2^31)");
  auto bad = [](double lo, double hi, double top) { return !(std::isfinite(lo) && std::isfinite(hi)) || lo < 0.0 || hi > top || lo > hi; };
  if (bad(a.comp_lo, a.comp_hi, 1.0)) return no(ARGS_RANGE, "the completeness range is not within [0, 1]");
  if (bad(a.cont_lo, a.cont_hi, 8.0)) return no(ARGS_RANGE, "the contamination range is not within [0, 8]");
  // genomes
  uint32_t max_cont = 0;
  for (uint32_t g = 0; g < a.ngenomes; ++g) {
    if (a.genome_len[g] < 1) return no(ARGS_RANGE, "genome " + std::to_string(g) + " has no bases");
    const int64_t C = a.genome_len[g] / a.contig_len;
    if (C == 0) return no(ARGS_RANGE, "genome " + std::to_string(g) + " is shorter than a contig");
    if (C > (int64_t)MAX_CONTIGS) return no(ARGS_RANGE, "genome " + std::to_string(g) + " has more than " + std::to_string(MAX_CONTIGS) + " contigs");
    const uint32_t ncont = rounded((uint32_t)C, top_fraction(a.cont_lo, a.cont_hi));
    if (ncont > MAX_CONT_DRAWS) return no(ARGS_RANGE, "more than 65535 contamination draws on genome " + std::to_string(g));
    max_cont = std::max(max_cont, ncont);
  }
  // keys
  const uint64_t cells = (uint64_t)a.ngenomes * a.nmarkers;
  if (cells > sim::MAX_KEYS) return no(ARGS_RANGE, "more than 2^31 - 1 (genome, marker) cells");
  if (a.key_off[0] != 0) return no(ARGS_INVALID, "key_off does not start at 0");
  uint64_t max_copies = 0;
  for (uint64_t c = 0; c < cells; ++c) {
    if (a.key_off[c + 1] < a.key_off[c]) return no(ARGS_INVALID, "key_off falls at cell " + std::to_string(c));
    if (a.key_off[c + 1] > nkeys) return no(ARGS_INVALID, "key_off beyond the keys at cell " + std::to_string(c));
    max_copies = std::max(max_copies, a.key_off[c + 1] - a.key_off[c]);
  }
  if (a.key_off[cells] > sim::MAX_KEYS) return no(ARGS_RANGE, "more than 2^31 - 1 keys");
  if (a.key_off[cells] && !a.key) return no(ARGS_INVALID, "NULL keys");
  for (uint64_t k = 0; k < a.key_off[cells]; ++k)
    if (a.key[k] < 0 || a.key[k] > 2147483647ll) return no(ARGS_RANGE, "key " + std::to_string(a.key[k]) + " does not fit int32");
  if (max_copies * ((uint64_t)max_cont + 1) > MAX_COUNT) return no(ARGS_RANGE, "copies of a marker times draws on a contig beyond 2^32 - 1");
  // marker sets
  return msets::check_marker_sets(a.nmarkers, a.nsets, a.ms_off, a.cs_off, a.cs_marker, ncs, nmembers, why);
}

// The device's copies of the tables of a checked call: everything in 32 bits.
struct Packed {
  msets::Packed sets;
  std::vector<uint32_t> key_off, ncontigs;           // [G * U + 1], [G]
  std::vector<int32_t> key;
  std::vector<uint64_t> row_off;                     // [G + 1]: genome g's multiplicity rows, R * C_g entries
  uint32_t max_contigs = 0;
  Params params;
};
inline void pack(const Args &a, Packed &P) {
  const uint64_t cells = (uint64_t)a.ngenomes * a.nmarkers, nkeys = a.key_off[cells];
  msets::pack(a.nmarkers, a.nsets, a.ms_off, a.cs_off, a.cs_marker, P.sets);
  P.key_off.resize(cells + 1); P.key.resize(nkeys); P.ncontigs.resize(a.ngenomes); P.row_off.assign((size_t)a.ngenomes + 1, 0);
  for (uint64_t c = 0; c <= cells; ++c) P.key_off[c] = (uint32_t)a.key_off[c];
  for (uint64_t k = 0; k < nkeys; ++k) P.key[k] = (int32_t)a.key[k];
  P.max_contigs = 0;
  for (uint32_t g = 0; g < a.ngenomes; ++g) {
    P.ncontigs[g] = (uint32_t)(a.genome_len[g] / a.contig_len);
    P.max_contigs = std::max(P.max_contigs, P.ncontigs[g]);
    P.row_off[g + 1] = P.row_off[g] + (uint64_t)a.nreplicates * P.ncontigs[g];
  }
  P.params = Params{(int32_t)a.contig_len, a.comp_lo, a.comp_hi, a.cont_lo, a.cont_hi, a.seed};
}

// draw d = g * R + r, R > 0: where its multiplicity row starts (d = G * R: where the last one ends)
inline uint64_t row_at(const Packed &P, uint32_t R, uint64_t d) {
  const uint64_t g = d / R, r = d % R;
  return g == P.ncontigs.size() ? P.row_off[g] : P.row_off[g] + r * P.ncontigs[g];
}
// what one draw needs on the device during a round: its results, a scratch row of counts when they do not fit LDS, its multiplicity row
inline uint64_t draw_bytes(uint32_t C, uint32_t nmarkers, uint32_t nsets, bool with_rows) {
  return 16 + (uint64_t)nsets * sim::OUT_BYTES + (nmarkers > STAGE_COUNTS ? (uint64_t)nmarkers * 4 : 0) + (with_rows ? (uint64_t)C * 2 : 0);
}
// A round: draws [d0, d1) that fit budget_bytes -- always at least one, never more than ROUND_DRAWS.  Returns d1.
inline uint32_t next_round(const Packed &P, uint32_t R, uint32_t nmarkers, uint32_t nsets, bool with_rows, uint64_t budget_bytes, uint32_t d0) {
  const uint32_t ndraws = (uint32_t)P.ncontigs.size() * R;
  uint64_t bytes = 0;
  uint32_t d = d0;
  for (; d < ndraws && d - d0 < ROUND_DRAWS; ++d) {
    const uint64_t b = draw_bytes(P.ncontigs[d / R], nmarkers, nsets, with_rows);
    if (d > d0 && bytes + b > budget_bytes) break;
    bytes += b;
  }
  return d;
}

}  // namespace sel
}  // namespace ckm
