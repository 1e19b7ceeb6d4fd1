// merge_dev.h -- the per-pair arithmetic of `checkm merge` (checkm/merger.py:64-106), written once for the kernels (kernels_merge.hip)
// and for the host executor of the CPU tests (tests/emu/merge_emu.cpp).
//
// A bin X is three integers and a bit row: member bits over the common marker genes G (bit g set: gene g is a key of the bin's hit
// dict), S_X = the number of hits to those genes, n_X = numMarkers() of the bin's marker set.  With c_X = popcount(row X) and
// u = popcount(row I | row J) the reference's float64 results are
//
//   comp_X = 100*float(c_X)/n_X        cont_X = 100*float(S_X - c_X)/n_X
//   comp_M = 100*float(u)/n_J          cont_M = 100*float(S_I + S_J - u)/n_J               (the merged pair is judged by J's marker set)
//   kept   = comp_M >= minMergedComp and cont_M < maxMergedCont
//   dComp  = comp_M - max(comp_I, comp_J)     dCont = cont_M - max(cont_I, cont_J)     delta = dComp - dCont
//   written = kept and dComp >= minDeltaComp and dCont < maxDeltaCont
//
// Every operation is one IEEE multiplication, division or subtraction in the order above: 100*float(x) first (exact: x is far below
// 2^46), the division second.  The library and the host executor are built with -ffp-contract=off and without fast-math.
#pragma once
#include <cstdint>
#include "pairs_dev.h"
#include "wave_const.h"

#if defined(__HIP__)
#include <hip/hip_runtime.h>
#define MG_HD __host__ __device__ __forceinline__
#else
#define MG_HD inline
#endif

namespace ckm {
namespace mg {

using ckm::WAVE;
constexpr int TILE_I = 64;                       // rows of a tile (bin I)
constexpr int TILE_J = WAVE;                     // columns of a tile (bin J): a lane per column
constexpr int WAVES = 4;                         // wavefronts of a block
constexpr int ROWS_PER_WAVE = TILE_I / WAVES;    // rows one wavefront walks: its running union counts live in registers
constexpr int WORD_CHUNK = 16;                   // words of a bit row staged at once: no compiled-in limit on the row's length
constexpr int NCOL = 9;                          // float64 columns of a reported pair, in the order of the output line

struct Thresholds { double min_delta_comp, max_delta_cont, min_merged_comp, max_merged_cont; };

// the per-bin operands of a pair
struct BinSide { int64_t hit_sum; int32_t n_markers; double comp, cont; };

using pc::pair_slot;                             // where the fill pass puts a reported pair

struct PairCols { double v[NCOL]; };             // compI, contI, compJ, contJ, deltaComp, deltaCont, delta, compM, contM

// what the kernels take by value (kernels_merge.hip, ckm_merge.hip)
struct MergeBins {
  const uint64_t *bits;        // [nbins * nwords]
  const int64_t *hit_sum;      // [nbins]
  const int32_t *n_markers;    // [nbins]
  double *comp, *cont;         // [nbins]
  uint32_t nbins, nwords;
};

struct MergeOut {
  const uint64_t *row_base;    // [rows of the count pass]: reported pairs of the rows before
  uint64_t batch_base, cap;    // first pair of this output batch; pairs the columns hold
  uint32_t *pi, *pj;           // [cap]
  double *cols;                // [NCOL * cap]
};

MG_HD int popc64(uint64_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popcll(x);
#else
  return __builtin_popcountll(x);
#endif
}

MG_HD double pct(int64_t x, int32_t n) { const double hundred_x = 100.0 * (double)x; return hundred_x / (double)n; }
MG_HD double pymax(double a, double b) { return b > a ? b : a; }         // Python's max(a, b): the first unless the second is larger

MG_HD void bin_stats(int32_t members, int64_t hit_sum, int32_t n_markers, double &comp, double &cont) {
  comp = pct(members, n_markers);
  cont = pct(hit_sum - (int64_t)members, n_markers);
}

// one word of the union count
MG_HD int union_word(uint64_t a, uint64_t b) { return popc64(a | b); }

// The two tests of merger.py:92 and :100 and the nine columns; `out` is complete only when the pair is written.
MG_HD bool pair_eval(int32_t u, const BinSide &I, const BinSide &J, const Thresholds &t, PairCols &out) {
  const double comp_m = pct(u, J.n_markers);
  const double cont_m = pct(I.hit_sum + J.hit_sum - (int64_t)u, J.n_markers);
  if (!(comp_m >= t.min_merged_comp && cont_m < t.max_merged_cont)) return false;
  const double d_comp = comp_m - pymax(I.comp, J.comp);
  const double d_cont = cont_m - pymax(I.cont, J.cont);
  const double delta = d_comp - d_cont;
  out.v[0] = I.comp; out.v[1] = I.cont; out.v[2] = J.comp; out.v[3] = J.cont;
  out.v[4] = d_comp; out.v[5] = d_cont; out.v[6] = delta; out.v[7] = comp_m; out.v[8] = cont_m;
  return d_comp >= t.min_delta_comp && d_cont < t.max_delta_cont;
}

}  // namespace mg
}  // namespace ckm
