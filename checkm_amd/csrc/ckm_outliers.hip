// ckm_outliers.hip -- C ABI of the outlier pass (kernels_outliers.hip): the counters of the nucleotide pass, every sequence's row of the
// tetranucleotide profile and its coding bases in; per-sequence GC, coding density, tetranucleotide distance, their differences to the bin
// and the outlier flags out.  Integer sums per bin on the host, four kernels, one download.
#include <algorithm>
#include <memory>
#include <numeric>
#include <string>
#include <vector>
#include "ckm_host.h"
#include "nucstats_host.h"
#include "outlier_dev.h"

namespace ckm {
void launch_outliers_seq(hipStream_t st, uint32_t nseq, const uint32_t *seq_bin, const uint32_t *bin_first, const uint64_t *count, const int64_t *coding,
                         const uint64_t *bin_sum, double *mean_gc, double *mean_cd, const ol::SeqCols &cols);
void launch_outliers_binsig(hipStream_t st, uint32_t nbins, const uint32_t *bin_order, const uint32_t *bin_first, const double *sig, const double *w, double *bin_sig);
void launch_outliers_td(hipStream_t st, uint32_t nseq, const uint32_t *seq_bin, const double *sig, const double *bin_sig, double *td);
void launch_outliers_flags(hipStream_t st, uint32_t nseq, const uint32_t *seq_bin, const uint64_t *count, const ol::Tables &T, const uint32_t *bin_gc_tab,
                           const uint32_t *bin_cd_tab, uint32_t td_tab, const ol::SeqCols &cols);
}  // namespace ckm
using namespace ckm;

struct ckm_outliers {
  uint32_t nseq = 0, nbins = 0;
  std::vector<double> seq;                 // six columns of nseq: gc, delta_gc, cd, delta_cd, td, weight
  std::vector<uint8_t> flags;
  std::vector<double> mean_gc, mean_cd, bin_sig;
  double ms_upload = 0, ms_seq = 0, ms_binsig = 0, ms_td = 0, ms_flags = 0, ms_total = 0;
};

extern "C" int ckm_outliers_run(ckm_ctx *ctx, const ckm_nucseq *b, const uint64_t *count, const double *sig, const int64_t *coding_per_seq,
                                const ckm_outlier_bounds *bounds, int64_t *zero_seq, ckm_outliers **out) {
  CallStream cs;
  return guarded([&] {
    if (!ctx || !b || !count || !sig || !coding_per_seq || !bounds || !zero_seq || !out) throw Error(CKM_EINVAL, "NULL argument");
    *out = nullptr; *zero_seq = -1;
    const WallClock t0;
    const uint32_t nseq = (uint32_t)b->seq_off.size(), nbins = (uint32_t)b->file_first.size() - 1;
    // the bound tables: every index inside its array, no empty table (the kernels read key[0] of the table they are given)
    const ckm_outlier_bounds &B = *bounds;
    if (!B.ntables || !B.tab_off || !B.key || !B.lo || !B.hi || (nbins && (!B.bin_gc_tab || !B.bin_cd_tab))) throw Error(CKM_EINVAL, "incomplete bound tables");
    if (B.tab_off[0] != 0) throw Error(CKM_EINVAL, "bound tables must start at row 0");
    for (uint32_t t = 0; t < B.ntables; ++t)
      if (B.tab_off[t + 1] <= B.tab_off[t]) throw Error(CKM_EINVAL, "bound table " + std::to_string(t) + " has no sequence-length key");
    if (B.td_tab >= B.ntables) throw Error(CKM_EINVAL, "td_tab outside the bound tables");
    for (uint32_t k = 0; k < nbins; ++k)
      if (B.bin_gc_tab[k] >= B.ntables || B.bin_cd_tab[k] >= B.ntables) throw Error(CKM_EINVAL, "bound table of bin " + std::to_string(k) + " outside the tables");
    const uint32_t nrows = B.tab_off[B.ntables];
    // integer sums per bin; the first division by zero the reference would meet (gcDist / codingDensityDist, checkm/binTools.py:158-181)
    std::vector<uint64_t> bin_sum((size_t)std::max(1u, nbins) * 4, 0);
    std::vector<uint32_t> seq_bin(std::max(1u, nseq), 0);
    for (uint32_t k = 0; k < nbins; ++k) {
      uint64_t *bs = &bin_sum[(size_t)k * 4];
      for (uint32_t s = b->file_first[k]; s < b->file_first[k + 1]; ++s) {
        const uint64_t *c = count + (size_t)s * 8;
        if (coding_per_seq[s] < 0) throw Error(CKM_EINVAL, "sequence " + std::to_string(s) + " has no coding bases: its bin has no gene file");
        if (c[0] + c[1] + c[2] + c[3] == 0 || c[6] == 0) { *zero_seq = s; throw Error(CKM_EINVAL, "division by zero: sequence " + b->ids[s] + " has no A, C, G, T or U"); }
        bs[0] += c[2] + c[1]; bs[1] += c[0] + c[1] + c[2] + c[3]; bs[2] += (uint64_t)coding_per_seq[s]; bs[3] += c[6];
        seq_bin[s] = k;
      }
      if (b->file_first[k] == b->file_first[k + 1]) { *zero_seq = b->file_first[k]; throw Error(CKM_EINVAL, "division by zero: bin " + std::to_string(k) + " has no sequence"); }
    }
    std::vector<uint32_t> order(nbins);                    // longest bin first
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
      return b->file_first[x + 1] - b->file_first[x] > b->file_first[y + 1] - b->file_first[y];
    });
    std::unique_ptr<ckm_outliers> o(new ckm_outliers());
    o->nseq = nseq; o->nbins = nbins;
    o->seq.assign((size_t)nseq * 6, 0.0); o->flags.assign(nseq, 0);
    o->mean_gc.assign(nbins, 0.0); o->mean_cd.assign(nbins, 0.0); o->bin_sig.assign((size_t)nbins * ol::NSIG, 0.0);
    if (nseq) {
      cs.open(ctx->device);
      DevBuf d_count, d_sig, d_coding, d_seqbin, d_first, d_order, d_sum, d_seq, d_flags, d_mean, d_binsig, d_tab, d_tabidx;
      const size_t n = nseq;
      d_seq.ensure(n * 48); d_flags.ensure(n); d_mean.ensure((size_t)nbins * 16); d_binsig.ensure((size_t)nbins * ol::NSIG * 8);
      d_tab.ensure((size_t)nrows * 24 + ((size_t)B.ntables + 1) * 4 + 8); d_tabidx.ensure((size_t)nbins * 8);
      cs.mark(0);
      cs.put(d_count, count, n * 64);
      cs.put(d_sig, sig, n * ol::NSIG * 8);
      cs.put(d_coding, coding_per_seq, n * 8);
      cs.put(d_seqbin, seq_bin.data(), n * 4);
      cs.put(d_first, b->file_first.data(), ((size_t)nbins + 1) * 4);
      cs.put(d_order, order.data(), (size_t)nbins * 4);
      cs.put(d_sum, bin_sum.data(), (size_t)nbins * 32);
      // tables: key, lo, hi (nrows doubles each), then tab_off
      double *tk = d_tab.as<double>();
      HIPCHK(hipMemcpyAsync(tk, B.key, (size_t)nrows * 8, hipMemcpyHostToDevice, cs.st));
      HIPCHK(hipMemcpyAsync(tk + nrows, B.lo, (size_t)nrows * 8, hipMemcpyHostToDevice, cs.st));
      HIPCHK(hipMemcpyAsync(tk + 2 * (size_t)nrows, B.hi, (size_t)nrows * 8, hipMemcpyHostToDevice, cs.st));
      uint32_t *toff = reinterpret_cast<uint32_t *>(tk + 3 * (size_t)nrows);
      HIPCHK(hipMemcpyAsync(toff, B.tab_off, ((size_t)B.ntables + 1) * 4, hipMemcpyHostToDevice, cs.st));
      uint32_t *gct = d_tabidx.as<uint32_t>(), *cdt = gct + nbins;
      HIPCHK(hipMemcpyAsync(gct, B.bin_gc_tab, (size_t)nbins * 4, hipMemcpyHostToDevice, cs.st));
      HIPCHK(hipMemcpyAsync(cdt, B.bin_cd_tab, (size_t)nbins * 4, hipMemcpyHostToDevice, cs.st));
      cs.mark(1);
      double *ds = d_seq.as<double>();
      const ol::SeqCols cols = {ds, ds + n, ds + 2 * n, ds + 3 * n, ds + 5 * n, ds + 4 * n, d_flags.as<uint8_t>()};
      double *mgc = d_mean.as<double>(), *mcd = mgc + nbins;
      launch_outliers_seq(cs.st, nseq, d_seqbin.as<uint32_t>(), d_first.as<uint32_t>(), d_count.as<uint64_t>(), d_coding.as<int64_t>(), d_sum.as<uint64_t>(), mgc, mcd, cols);
      HIPCHK(hipGetLastError());
      cs.mark(2);
      launch_outliers_binsig(cs.st, nbins, d_order.as<uint32_t>(), d_first.as<uint32_t>(), d_sig.as<double>(), cols.w, d_binsig.as<double>());
      HIPCHK(hipGetLastError());
      cs.mark(3);
      launch_outliers_td(cs.st, nseq, d_seqbin.as<uint32_t>(), d_sig.as<double>(), d_binsig.as<double>(), cols.td);
      HIPCHK(hipGetLastError());
      cs.mark(4);
      const ol::Tables T = {toff, tk, tk + nrows, tk + 2 * (size_t)nrows};
      launch_outliers_flags(cs.st, nseq, d_seqbin.as<uint32_t>(), d_count.as<uint64_t>(), T, gct, cdt, B.td_tab, cols);
      HIPCHK(hipGetLastError());
      cs.mark(5);
      HIPCHK(hipMemcpyAsync(o->seq.data(), d_seq.p, n * 48, hipMemcpyDeviceToHost, cs.st));
      HIPCHK(hipMemcpyAsync(o->flags.data(), d_flags.p, n, hipMemcpyDeviceToHost, cs.st));
      HIPCHK(hipMemcpyAsync(o->mean_gc.data(), mgc, (size_t)nbins * 8, hipMemcpyDeviceToHost, cs.st));
      HIPCHK(hipMemcpyAsync(o->mean_cd.data(), mcd, (size_t)nbins * 8, hipMemcpyDeviceToHost, cs.st));
      HIPCHK(hipMemcpyAsync(o->bin_sig.data(), d_binsig.p, (size_t)nbins * ol::NSIG * 8, hipMemcpyDeviceToHost, cs.st));
      HIPCHK(hipStreamSynchronize(cs.st));
      o->ms_upload = cs.ms(0, 1); o->ms_seq = cs.ms(1, 2); o->ms_binsig = cs.ms(2, 3); o->ms_td = cs.ms(3, 4); o->ms_flags = cs.ms(4, 5);
    }
    o->ms_total = t0.ms();
    *out = o.release();
  });
}

extern "C" int ckm_outliers_columns_get(const ckm_outliers *r, ckm_outliers_columns *c) {
  if (!r || !c) { set_last_error("NULL argument"); return CKM_EINVAL; }
  const size_t n = r->nseq;
  const double *s = r->seq.data();
  c->nseq = r->nseq; c->nbins = r->nbins;
  c->gc = s; c->delta_gc = s + n; c->cd = s + 2 * n; c->delta_cd = s + 3 * n; c->td = s + 4 * n; c->weight = s + 5 * n;
  c->flags = r->flags.data();
  c->mean_gc = r->mean_gc.data(); c->mean_cd = r->mean_cd.data(); c->bin_sig = r->bin_sig.data();
  c->ms_upload = r->ms_upload; c->ms_seq = r->ms_seq; c->ms_binsig = r->ms_binsig; c->ms_td = r->ms_td; c->ms_flags = r->ms_flags; c->ms_total = r->ms_total;
  return CKM_OK;
}

extern "C" void ckm_outliers_free(ckm_outliers *r) { delete r; }
