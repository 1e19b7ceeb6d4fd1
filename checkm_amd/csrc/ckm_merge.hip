// ckm_merge.hip -- C ABI of the all-pairs comparison of `checkm merge` (kernels_merge.hip): one bit row and three integers per bin in;
// the reported pairs in the reference's order out, as columns and / or as the lines of merger.tsv.  A count pass, a scan and a fill pass
// per stretch of rows; the fill pass runs in batches of whole rows whose output fits the budget, so the memory of a call does not grow
// with the number of reported pairs.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>
#include "ckm_host.h"
#include "merge_host.h"
#include "pairs_host.h"

namespace ckm {
using mg::MergeBins;
using mg::MergeOut;
void launch_merge_bins(hipStream_t st, const MergeBins &B);
void launch_merge_tiles(hipStream_t st, bool fill, const MergeBins &B, const mg::Thresholds &thr, uint32_t row_lo, uint32_t row_hi, uint32_t count_row0,
                        uint32_t *tile_count, const MergeOut &out);
void launch_merge_scan(hipStream_t st, uint32_t row0, uint32_t nrows, uint32_t ntiles_j, uint32_t *tile_count, uint32_t *row_total);
}  // namespace ckm
using namespace ckm;

struct ckm_merge {
  uint64_t npairs = 0, compared = 0, nbatches = 0;
  bool kept = false;
  std::vector<uint32_t> pi, pj;
  std::vector<double> col[mg::NCOL];
  double ms_upload = 0, ms_bins = 0, ms_count = 0, ms_scan = 0, ms_fill = 0, ms_download = 0, ms_write = 0, ms_total = 0;
};

extern "C" int ckm_merge_check(uint32_t nbins, uint32_t ngenes, const uint64_t *member_bits, const int64_t *hit_sum, const int32_t *n_markers, const double *thr) {
  const std::string why = mg::check_args(nbins, ngenes, member_bits, hit_sum, n_markers, thr);
  if (!why.empty()) { set_last_error(why); return CKM_EINVAL; }
  return CKM_OK;
}

extern "C" int ckm_merge_run(ckm_ctx *ctx, uint32_t nbins, uint32_t ngenes, const uint64_t *member_bits, const int64_t *hit_sum, const int32_t *n_markers,
                             const double *thr, const char *const *bin_ids, const char *append_path, uint64_t budget_bytes, int keep_columns, ckm_merge **out) {
  CallStream cs;
  std::unique_ptr<FILE, int (*)(FILE *)> fp(nullptr, fclose);      // an error leaves the file closed
  return guarded([&] {
    if (!ctx || !out) throw Error(CKM_EINVAL, "NULL argument");
    *out = nullptr;
    if (append_path && !bin_ids) throw Error(CKM_EINVAL, "lines cannot be written without the bin ids");
    const std::string why = mg::check_args(nbins, ngenes, member_bits, hit_sum, n_markers, thr);
    if (!why.empty()) throw Error(CKM_EINVAL, why);
    const WallClock t0;
    budget_bytes = batch_budget(budget_bytes, "CKM_MERGE_BATCH_MB", 256);
    const uint64_t cap_pairs = mg::budget_pairs(budget_bytes);
    const mg::Thresholds T = {thr[0], thr[1], thr[2], thr[3]};
    std::unique_ptr<ckm_merge> o(new ckm_merge());
    o->kept = keep_columns != 0;
    o->compared = (uint64_t)nbins * (nbins ? nbins - 1 : 0) / 2;
    if (append_path) {
      fp.reset(fopen(append_path, "ab"));
      if (!fp) throw Error(CKM_EIO, std::string("cannot append to ") + append_path);
    }
    if (nbins > 1) {
      const uint32_t nwords = mg::words_for(ngenes), ntj = mg::tiles_for(nbins);
      const size_t nb = nbins;
      cs.open(ctx->device);      // every phase below is waited for (cs.timed): the host needs its result before the next one
      DevBuf d_bits, d_sum, d_n, d_stat, d_count;
      PairBatches pb;
      d_stat.ensure(nb * 16);
      cs.timed(o->ms_upload, [&] {
        cs.put(d_bits, member_bits, nb * nwords * 8);
        cs.put(d_sum, hit_sum, nb * 8);
        cs.put(d_n, n_markers, nb * 4);
      });
      const MergeBins B = {d_bits.as<uint64_t>(), d_sum.as<int64_t>(), d_n.as<int32_t>(), d_stat.as<double>(), d_stat.as<double>() + nb, nbins, nwords};
      cs.timed(o->ms_bins, [&] { launch_merge_bins(cs.st, B); HIPCHK(hipGetLastError()); });
      const uint32_t pass_rows = mg::count_pass_rows(nbins);
      d_count.ensure((size_t)pass_rows * ntj * 4);
      std::string lines;
      // a batch on the host: columns first (8-byte values), then the two index columns
      auto take = [&](const void *h_out, uint64_t n) {
        const double *hc = static_cast<const double *>(h_out);
        const uint32_t *hi = reinterpret_cast<const uint32_t *>(hc + mg::NCOL * n), *hj = hi + n;
        if (o->kept) {
          o->pi.insert(o->pi.end(), hi, hi + n); o->pj.insert(o->pj.end(), hj, hj + n);
          for (int c = 0; c < mg::NCOL; ++c) o->col[c].insert(o->col[c].end(), hc + (size_t)c * n, hc + (size_t)(c + 1) * n);
        }
        if (fp) {
          const WallClock w0;
          constexpr uint64_t STEP = 1 << 16;                 // the text of a batch is several times its columns: formatted and written in pieces
          for (uint64_t k = 0; k < n; k += STEP) {
            const uint64_t m = std::min<uint64_t>(STEP, n - k);
            lines.clear();
            mg::format_lines(lines, bin_ids, hi + k, hj + k, hc + k, n, m);
            if (fwrite(lines.data(), 1, lines.size(), fp.get()) != lines.size()) throw Error(CKM_EIO, std::string("cannot write to ") + append_path);
          }
          o->ms_write += w0.ms();
        }
        o->npairs += n; o->nbatches += 1;
      };
      for (uint32_t r0 = 0; r0 < nbins; r0 += pass_rows) {
        const uint32_t r1 = std::min<uint64_t>(nbins, (uint64_t)r0 + pass_rows), nr = r1 - r0;
        MergeOut none = {nullptr, 0, 0, nullptr, nullptr, nullptr};
        cs.timed(o->ms_count, [&] { launch_merge_tiles(cs.st, false, B, T, r0, r1, r0, d_count.as<uint32_t>(), none); HIPCHK(hipGetLastError()); });
        pb.run(cs, r0, nr, cap_pairs, mg::PAIR_BYTES, o->ms_scan, o->ms_fill, o->ms_download,
               [&](uint32_t *d_total) { launch_merge_scan(cs.st, r0, nr, ntj, d_count.as<uint32_t>(), d_total); },
               [&](const pc::Group &g, void *d_out, uint64_t n) {
                 double *dc = static_cast<double *>(d_out);
                 uint32_t *di = reinterpret_cast<uint32_t *>(dc + mg::NCOL * n);
                 const MergeOut mo = {pb.d_base.as<uint64_t>(), g.base, n, di, di + n, dc};
                 launch_merge_tiles(cs.st, true, B, T, g.row_lo, g.row_hi, r0, d_count.as<uint32_t>(), mo);
               },
               take);
      }
    }
    if (fp && fclose(fp.release()) != 0) throw Error(CKM_EIO, std::string("cannot write to ") + append_path);
    o->ms_total = t0.ms();
    *out = o.release();
  });
}

extern "C" int ckm_merge_columns_get(const ckm_merge *r, ckm_merge_columns *c) {
  if (!r || !c) { set_last_error("NULL argument"); return CKM_EINVAL; }
  c->npairs = r->npairs; c->compared = r->compared; c->nbatches = r->nbatches;
  c->kept = r->kept ? 1 : 0;
  c->i = r->pi.data(); c->j = r->pj.data();
  for (int k = 0; k < mg::NCOL; ++k) c->col[k] = r->col[k].data();
  c->ms_upload = r->ms_upload; c->ms_bins = r->ms_bins; c->ms_count = r->ms_count; c->ms_scan = r->ms_scan; c->ms_fill = r->ms_fill;
  c->ms_download = r->ms_download; c->ms_write = r->ms_write; c->ms_total = r->ms_total;
  return CKM_OK;
}

extern "C" void ckm_merge_free(ckm_merge *r) { delete r; }
