// outlier_dev.h -- the float64 arithmetic of `checkm outliers` (checkm/binTools.py:148-209,249-292), written once for the kernels
// (kernels_outliers.hip) and for the host executor of the CPU tests (tests/emu/outliers_emu.cpp).
//
// Every result must equal the reference's bit for bit, so every function here fixes an evaluation order.  Nothing in this file may be
// contracted into a fused multiply-add: acc + x * w below is a rounded product and then a rounded sum (numpy computes the weighted row
// first and adds it afterwards), and one fused operation changes the last bit.  The library and the host executor are both built with
// -ffp-contract=off and without fast-math; these functions depend on it.
//
//   (a) per sequence   gc = double(g + c) / double(a + c + g + t), cd = double(coding) / double(len), w = double(len) / double(bin len)
//       per bin        mean = double(integer sum) / double(integer sum); delta = value - mean            (gcDist, codingDensityDist)
//   (b) bin signature  acc = sig[s0][c] * w0, then acc = acc + sig[s][c] * w_s in file order             (binTetraSig)
//   (c) TD             numpy's pairwise sum of |sig - bin_sig| over 136 values: elements 0..63 and 64..135 apart, each with eight
//                      running sums over strides of 8 combined as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)); first + second
//                                                                                   (GenomicSignatures.distance: np.sum(np.abs(..)))
//   (d) flags          nearest sequence-length key (first minimum of |key - len| in float64) and three comparisons, false on nan
#pragma once
#include <cstdint>
#include "wave_const.h"

#if defined(__HIP__)
#include <hip/hip_runtime.h>
#define OL_HD __host__ __device__ __forceinline__
#else
#define OL_HD inline
#endif

namespace ckm {
namespace ol {

constexpr int NSIG = ckm::NKMER;   // canonical tetranucleotides: one row of the profile
constexpr int TD_SPLIT = 64;       // numpy's pairwise sum cuts 136 elements at 64 (n / 2 rounded down to a multiple of 8)
constexpr int TD_ACC = 8;          // running sums of one half
using ckm::WAVE;
constexpr int TD_SEQS = WAVE / TD_ACC;   // sequences a wavefront takes at once: eight lanes (= eight running sums) each
enum { F_GC = 1, F_CD = 2, F_TD = 4 };

// (a) every quotient is one IEEE division of two exactly converted integers (all below 2^53)
OL_HD double ratio(uint64_t num, uint64_t den) { return (double)num / (double)den; }
OL_HD double ratio(int64_t num, uint64_t den) { return (double)num / (double)den; }

// (b) one step of the serial sum of column c: product rounded, then sum rounded
OL_HD double binsig_first(double x, double w) { return x * w; }
OL_HD double binsig_next(double acc, double x, double w) { const double p = x * w; return acc + p; }

OL_HD double absd(double x) { return __builtin_fabs(x); }

// (c) running sum r (0..7) of one half: elements first + r, first + r + 8, ... (count / 8 of them), in that order
OL_HD double td_running(const double *sig, const double *bin, int first, int count, int r) {
  double acc = absd(sig[first + r] - bin[first + r]);
  for (int k = TD_ACC; k < count; k += TD_ACC) acc = acc + absd(sig[first + r + k] - bin[first + r + k]);
  return acc;
}
// The combine of the eight running sums is a butterfly over the eight lanes that hold them, partners 1, 2, 4 in that order: after the
// step with partner p every lane of a group of 2p holds the same sum, and addition commutes, so lane 0 ends with
// ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)).  `Exchange` hands a lane its partner's value (a cross-lane move on the device, an array here).
template <class Exchange>
OL_HD double td_combine(double v, Exchange partner) {
  v = v + partner(v, 1);
  v = v + partner(v, 2);
  v = v + partner(v, 4);
  return v;
}

// (d) np.abs(np.array(keys) - len).argmin(): the first smallest distance
OL_HD int nearest_key(const double *key, int n, double len) {
  int best = 0;
  double bd = absd(key[0] - len);
  for (int k = 1; k < n; ++k) {
    const double d = absd(key[k] - len);
    if (d < bd) { bd = d; best = k; }
  }
  return best;
}
OL_HD uint8_t flag_bits(double delta_gc, double gc_lo, double gc_hi, double delta_cd, double cd_lo, double td, double td_hi) {
  uint8_t f = 0;
  if (delta_gc < gc_lo || delta_gc > gc_hi) f |= F_GC;
  if (delta_cd < cd_lo) f |= F_CD;
  if (td > td_hi) f |= F_TD;
  return f;
}

// The bound tables as the kernels read them: table t owns rows tab_off[t] .. tab_off[t + 1] of key / lo / hi, in the distribution's
// dict order.  A GC table holds (length key, lower, upper), a CD table (length key, lower, unused), the TD table (length key, unused, bound).
struct Tables {
  const uint32_t *tab_off;
  const double *key, *lo, *hi;
};

// per-sequence columns
struct SeqCols {
  double *gc, *delta_gc, *cd, *delta_cd, *w, *td;
  uint8_t *flags;
};

// (a) for sequence s of bin b.  count: the eight counters per sequence of the nucleotide pass (A, C, G, T+U, N, n, code points, ..)
OL_HD void seq_stats(uint32_t s, const uint64_t *count, const int64_t *coding, uint64_t bin_len, double mean_gc, double mean_cd, const SeqCols &o) {
  const uint64_t *c = count + (uint64_t)s * 8;
  const uint64_t gcn = c[2] + c[1], bases = c[0] + c[1] + c[2] + c[3], len = c[6];
  const double gc = ratio(gcn, bases), cd = ratio(coding[s], len);
  o.gc[s] = gc; o.cd[s] = cd;
  o.delta_gc[s] = gc - mean_gc; o.delta_cd[s] = cd - mean_cd;
  o.w[s] = ratio(len, bin_len);
}

// (d) for sequence s
OL_HD uint8_t seq_flags(uint32_t s, double len, const Tables &T, uint32_t gc_tab, uint32_t cd_tab, uint32_t td_tab, const SeqCols &o) {
  const uint32_t g0 = T.tab_off[gc_tab], c0 = T.tab_off[cd_tab], t0 = T.tab_off[td_tab];
  const int kg = nearest_key(T.key + g0, (int)(T.tab_off[gc_tab + 1] - g0), len);
  const int kc = nearest_key(T.key + c0, (int)(T.tab_off[cd_tab + 1] - c0), len);
  const int kt = nearest_key(T.key + t0, (int)(T.tab_off[td_tab + 1] - t0), len);
  return flag_bits(o.delta_gc[s], T.lo[g0 + kg], T.hi[g0 + kg], o.delta_cd[s], T.lo[c0 + kc], o.td[s], T.hi[t0 + kt]);
}

}  // namespace ol
}  // namespace ckm
