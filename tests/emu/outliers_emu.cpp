// outliers_emu.cpp -- TEST INFRASTRUCTURE: the arithmetic of the outlier pass (checkm_amd/csrc/outlier_dev.h) compiled by g++ against a
// HOST executor, so that the CPU test suite can compare its evaluation orders with numpy bit for bit.  The kernels of
// kernels_outliers.hip are restated as loops over their threads; the eight lanes that hold the running sums of one sequence's TD are an
// array, and a lane's partner value is recomputed as the partner lane computed it.  Built with -ffp-contract=off like the library.
// Nothing in checkm_amd loads this.
#include <cstring>
#include <vector>
#include "../../checkm_amd/csrc/outlier_dev.h"

using namespace ckm::ol;

namespace {
// what the lane (l ^ p) of a group of eight holds when lane l asks for it in td_combine: the sum of its own group of p lanes, built by
// the same steps
struct ArrayPartner {
  const double *r; int lane;
  static double held(const double *r, int l, int p) {        // value of lane l before the step with partner p
    if (p == 1) return r[l];
    const double mine = held(r, l, p >> 1), other = held(r, l ^ (p >> 1), p >> 1);
    return mine + other;
  }
  double operator()(double, int p) const { return held(r, lane ^ p, p); }
};

double td_of(const double *row, const double *bin) {
  double half[2];
  for (int h = 0; h < 2; ++h) {
    const int first = h ? TD_SPLIT : 0, count = h ? NSIG - TD_SPLIT : TD_SPLIT;
    double r[TD_ACC], lane_result[TD_ACC];
    for (int l = 0; l < TD_ACC; ++l) r[l] = td_running(row, bin, first, count, l);
    for (int l = 0; l < TD_ACC; ++l) lane_result[l] = td_combine(r[l], ArrayPartner{r, l});
    half[h] = lane_result[0];
  }
  return half[0] + half[1];
}
}  // namespace

extern "C" double emu_td(const double *row, const double *bin) { return td_of(row, bin); }

extern "C" int emu_nearest_key(const double *key, int n, double len) { return nearest_key(key, n, len); }

// the four kernels over one batch; outputs as ckm_outliers_columns lays them out
extern "C" int emu_outliers(uint32_t nseq, uint32_t nbins, const uint32_t *bin_first, const uint64_t *count, const int64_t *coding, const double *sig,
                            const uint32_t *tab_off, const double *key, const double *lo, const double *hi, const uint32_t *bin_gc_tab, const uint32_t *bin_cd_tab,
                            uint32_t td_tab, double *gc, double *delta_gc, double *cd, double *delta_cd, double *td, double *weight, uint8_t *flags,
                            double *mean_gc, double *mean_cd, double *bin_sig) {
  std::vector<uint32_t> seq_bin(nseq);
  std::vector<uint64_t> bin_sum((size_t)nbins * 4, 0);
  for (uint32_t b = 0; b < nbins; ++b)
    for (uint32_t s = bin_first[b]; s < bin_first[b + 1]; ++s) {
      const uint64_t *c = count + (size_t)s * 8;
      if (c[0] + c[1] + c[2] + c[3] == 0 || c[6] == 0) return -1;
      bin_sum[b * 4] += c[2] + c[1]; bin_sum[b * 4 + 1] += c[0] + c[1] + c[2] + c[3]; bin_sum[b * 4 + 2] += (uint64_t)coding[s]; bin_sum[b * 4 + 3] += c[6];
      seq_bin[s] = b;
    }
  const SeqCols cols = {gc, delta_gc, cd, delta_cd, weight, td, flags};
  for (uint32_t s = 0; s < nseq; ++s) {                      // outliers_seq_kernel
    const uint64_t *bs = &bin_sum[(size_t)seq_bin[s] * 4];
    const double mgc = ratio(bs[0], bs[1]), mcd = ratio(bs[2], bs[3]);
    seq_stats(s, count, coding, bs[3], mgc, mcd, cols);
    mean_gc[seq_bin[s]] = mgc; mean_cd[seq_bin[s]] = mcd;
  }
  for (uint32_t b = 0; b < nbins; ++b)                       // outliers_binsig_kernel: a lane per column
    for (int col = 0; col < NSIG; ++col) {
      const uint32_t s0 = bin_first[b], s1 = bin_first[b + 1];
      if (s0 >= s1) continue;
      double acc = binsig_first(sig[(size_t)s0 * NSIG + col], weight[s0]);
      for (uint32_t s = s0 + 1; s < s1; ++s) acc = binsig_next(acc, sig[(size_t)s * NSIG + col], weight[s]);
      bin_sig[(size_t)b * NSIG + col] = acc;
    }
  for (uint32_t s = 0; s < nseq; ++s) td[s] = td_of(sig + (size_t)s * NSIG, bin_sig + (size_t)seq_bin[s] * NSIG);   // outliers_td_kernel
  const Tables T = {tab_off, key, lo, hi};
  for (uint32_t s = 0; s < nseq; ++s)                        // outliers_flags_kernel
    flags[s] = seq_flags(s, (double)count[(size_t)s * 8 + 6], T, bin_gc_tab[seq_bin[s]], bin_cd_tab[seq_bin[s]], td_tab, cols);
  return 0;
}
