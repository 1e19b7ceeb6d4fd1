// kernels_outliers.hip -- per-sequence GC, coding density and tetranucleotide distance of `checkm outliers` against their bin, and the
// outlier flags (checkm/binTools.py:148-209,249-292).  gfx950 only.  The arithmetic is outlier_dev.h, shared with the host executor of the
// CPU tests; every result is float64 and equals the reference's bit for bit.
//
// These kernels depend on the library's -ffp-contract=off -fno-fast-math: a fused multiply-add in the bin signature's serial sum, or a
// reassociated sum anywhere, changes the last bit.
//
//   outliers_seq_kernel     a thread per sequence: gc, cd, their difference to the bin's means, the sequence's weight in the bin
//                           signature; the first sequence of a bin also stores the bin's means.
//   outliers_binsig_kernel  a wavefront per (bin, 64 columns of the 136): lanes are columns, the bin's sequences are walked in file order
//                           (the sum's order is the result).  Bins have one to tens of thousands of sequences, so the work items are
//                           handed out longest bin first and no lane waits for a block mate beyond its own bin's length.  Row loads are
//                           512 contiguous bytes per wavefront and do not depend on the running sum: four rows are in flight.
//   outliers_td_kernel      a wavefront per eight consecutive sequences: lane = (sequence, running sum r of numpy's pairwise sum).  A row
//                           is 136 doubles = 1088 bytes = 17 * 64: per load the eight lanes of a sequence read one aligned 64-byte piece
//                           of its row, and the eight rows of a wavefront are contiguous.  The eight running sums are combined by DPP
//                           moves inside the group of eight lanes in numpy's tree.
//   outliers_flags_kernel   a thread per sequence: nearest length key of the bin's bound tables, three comparisons.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "outlier_dev.h"
#include "xlane.h"

namespace ckm {
using namespace ol;

__global__ __launch_bounds__(256) void outliers_seq_kernel(uint32_t nseq, const uint32_t *__restrict__ seq_bin, const uint32_t *__restrict__ bin_first,
                                                            const uint64_t *__restrict__ count, const int64_t *__restrict__ coding,
                                                            const uint64_t *__restrict__ bin_sum /* [nbins * 4]: g+c, a+c+g+t, coding, len */,
                                                            double *__restrict__ mean_gc, double *__restrict__ mean_cd, SeqCols cols) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s >= nseq) return;
  const uint32_t b = seq_bin[s];
  const uint64_t *bs = bin_sum + (uint64_t)b * 4;
  const double mgc = ratio(bs[0], bs[1]), mcd = ratio(bs[2], bs[3]);
  seq_stats(s, count, coding, bs[3], mgc, mcd, cols);
  if (s == bin_first[b]) { mean_gc[b] = mgc; mean_cd[b] = mcd; }
}

constexpr int SIG_CHUNKS = (NSIG + WAVE - 1) / WAVE;   // 3: columns 0..63, 64..127, 128..135

__global__ __launch_bounds__(256) void outliers_binsig_kernel(uint32_t nbins, const uint32_t *__restrict__ bin_order, const uint32_t *__restrict__ bin_first,
                                                               const double *__restrict__ sig, const double *__restrict__ w, double *__restrict__ bin_sig) {
  const int lane = threadIdx.x & (WAVE - 1);
  const uint32_t item = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (item >= nbins * SIG_CHUNKS) return;
  const uint32_t b = bin_order[item / SIG_CHUNKS];
  const int col = (int)(item % SIG_CHUNKS) * WAVE + lane;
  if (col >= NSIG) return;
  const uint32_t s0 = bin_first[b], s1 = bin_first[b + 1];
  if (s0 >= s1) return;
  const double *row = sig + (uint64_t)s0 * NSIG + col;
  double acc = binsig_first(row[0], w[s0]);
  uint32_t s = s0 + 1;
  row += NSIG;
  for (; s + 4 <= s1; s += 4, row += 4 * NSIG) {
    const double x0 = row[0], x1 = row[NSIG], x2 = row[2 * NSIG], x3 = row[3 * NSIG];
    const double w0 = w[s], w1 = w[s + 1], w2 = w[s + 2], w3 = w[s + 3];
    acc = binsig_next(acc, x0, w0);
    acc = binsig_next(acc, x1, w1);
    acc = binsig_next(acc, x2, w2);
    acc = binsig_next(acc, x3, w3);
  }
  for (; s < s1; ++s, row += NSIG) acc = binsig_next(acc, row[0], w[s]);
  bin_sig[(uint64_t)b * NSIG + col] = acc;
}

template <int CTRL>
__device__ __forceinline__ double dpp_d(double v) {
  const uint64_t u = __builtin_bit_cast(uint64_t, v);
  const int lo = (int)(uint32_t)u, hi = (int)(uint32_t)(u >> 32);
  const uint32_t plo = (uint32_t)dpp_i<CTRL>(lo, lo), phi = (uint32_t)dpp_i<CTRL>(hi, hi);
  return __builtin_bit_cast(double, (uint64_t)plo | ((uint64_t)phi << 32));
}
// The partner of a lane inside its group of eight.  Partner 4 is taken as the mirror lane (7 - z): after the steps with partners 1 and 2
// the four lanes of each half hold the same sum, so the mirror lane holds what lane z ^ 4 holds.
struct DppPartner {
  __device__ __forceinline__ double operator()(double v, int p) const {
    return p == 1 ? dpp_d<DPP_QUAD_XOR1>(v) : p == 2 ? dpp_d<DPP_QUAD_XOR2>(v) : dpp_d<DPP_ROW_HALF_MIRROR>(v);
  }
};

__global__ __launch_bounds__(256) void outliers_td_kernel(uint32_t nseq, const uint32_t *__restrict__ seq_bin, const double *__restrict__ sig,
                                                           const double *__restrict__ bin_sig, double *__restrict__ td) {
  const int lane = threadIdx.x & (WAVE - 1), r = lane & (TD_ACC - 1);
  const uint64_t wave = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
  const uint64_t want = wave * TD_SEQS + (uint64_t)(lane >> 3);
  if (wave * TD_SEQS >= nseq) return;                       // whole wavefronts only: the cross-lane moves below need every lane of a group
  const uint32_t s = want < nseq ? (uint32_t)want : nseq - 1;
  const double *row = sig + (uint64_t)s * NSIG, *bin = bin_sig + (uint64_t)seq_bin[s] * NSIG;
  const double first = td_combine(td_running(row, bin, 0, TD_SPLIT, r), DppPartner());
  const double second = td_combine(td_running(row, bin, TD_SPLIT, NSIG - TD_SPLIT, r), DppPartner());
  if (r == 0 && want < nseq) td[s] = first + second;
}

__global__ __launch_bounds__(256) void outliers_flags_kernel(uint32_t nseq, const uint32_t *__restrict__ seq_bin, const uint64_t *__restrict__ count, Tables T,
                                                              const uint32_t *__restrict__ bin_gc_tab, const uint32_t *__restrict__ bin_cd_tab, uint32_t td_tab, SeqCols cols) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s >= nseq) return;
  const uint32_t b = seq_bin[s];
  cols.flags[s] = seq_flags(s, (double)count[(uint64_t)s * 8 + 6], T, bin_gc_tab[b], bin_cd_tab[b], td_tab, cols);
}

void launch_outliers_seq(hipStream_t st, uint32_t nseq, const uint32_t *seq_bin, const uint32_t *bin_first, const uint64_t *count, const int64_t *coding,
                         const uint64_t *bin_sum, double *mean_gc, double *mean_cd, const SeqCols &cols) {
  if (nseq) hipLaunchKernelGGL(outliers_seq_kernel, dim3((nseq + 255) / 256), dim3(256), 0, st, nseq, seq_bin, bin_first, count, coding, bin_sum, mean_gc, mean_cd, cols);
}
void launch_outliers_binsig(hipStream_t st, uint32_t nbins, const uint32_t *bin_order, const uint32_t *bin_first, const double *sig, const double *w, double *bin_sig) {
  const uint32_t items = nbins * SIG_CHUNKS;
  if (items) hipLaunchKernelGGL(outliers_binsig_kernel, dim3((items + 3) / 4), dim3(256), 0, st, nbins, bin_order, bin_first, sig, w, bin_sig);
}
void launch_outliers_td(hipStream_t st, uint32_t nseq, const uint32_t *seq_bin, const double *sig, const double *bin_sig, double *td) {
  const uint32_t waves = (nseq + TD_SEQS - 1) / TD_SEQS;
  if (waves) hipLaunchKernelGGL(outliers_td_kernel, dim3((waves + 3) / 4), dim3(256), 0, st, nseq, seq_bin, sig, bin_sig, td);
}
void launch_outliers_flags(hipStream_t st, uint32_t nseq, const uint32_t *seq_bin, const uint64_t *count, const Tables &T, const uint32_t *bin_gc_tab,
                           const uint32_t *bin_cd_tab, uint32_t td_tab, const SeqCols &cols) {
  if (nseq) hipLaunchKernelGGL(outliers_flags_kernel, dim3((nseq + 255) / 256), dim3(256), 0, st, nseq, seq_bin, count, T, bin_gc_tab, bin_cd_tab, td_tab, cols);
}

}  // namespace ckm
