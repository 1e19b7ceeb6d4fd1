// ckm_coverage.hip -- C ABI of `checkm coverage`: the BAM handle (bam_host.cpp; no device) and the device pass over its records
// (kernels_coverage.hip).  Batch by batch: the host inflates a batch, the records and their offsets go up, the kernel adds to the
// per-reference counters; every phase is waited for (the reader's buffer is reused by the next batch), so inflating and the kernel do
// not overlap.  The counters come down once, at the end.  CoverageWindows (`checkm gc_bias_plot`; kernels_covwin.hip) runs the same batch
// loop with its own chain and two more accumulators, the window arrays, which a scan turns into window sums after the last batch.
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>
#include "ckm_host.h"
#include "bam_host.h"
#include "covwin_dev.h"

namespace ckm {
void launch_coverage(hipStream_t st, const uint8_t *data, const uint32_t *offsets, uint32_t nrec, uint64_t first_ordinal, const cv::Params &P,
                     unsigned long long *counters, unsigned long long *err_slot);
void launch_covwin(hipStream_t st, const uint8_t *data, const uint32_t *offsets, uint32_t nrec, uint64_t first_ordinal, const cw::Params &P, const int64_t *ref_len,
                   const int64_t *ref_first, unsigned long long *counters, unsigned long long *direct, unsigned long long *diff, unsigned long long *err_slot);
void launch_covwin_scan(hipStream_t st, unsigned long long *direct, const unsigned long long *diff, unsigned long long *sums, uint32_t n);
}

struct ckm_bam {
  std::unique_ptr<HostPool> pool;
  std::unique_ptr<bam::Reader> reader;
  std::vector<const char *> names;
};

static std::string check_window_params(const ckm_coverage_windows_params *p) {
  if (!p) return "NULL argument";
  if (std::isnan(p->min_align_per) || std::isnan(p->max_edit_dist_per)) return "a coverage threshold is not a number";
  if (p->window_size < 1 || p->window_size > cw::MAX_WINDOW) return "the window size must be between 1 and 2^31 - 1";
  return "";
}

// first[k] = the first slot of reference k, first[n_ref] = all slots; refuses more than 2^31 - 1
static void window_layout(const bam::Reader &rd, int64_t w, int64_t *first) {
  const std::vector<int64_t> &len = rd.ref_lengths();
  int64_t at = 0;
  for (size_t k = 0; k < len.size(); ++k) {
    first[k] = at;
    at += cw::slots_of(len[k], w);
    if (at > cw::MAX_SLOTS) throw Error(CKM_EINVAL, rd.path() + ": more than 2^31 - 1 windows with a window size of " + std::to_string(w));
  }
  first[len.size()] = at;
}

static std::string check_params(const ckm_coverage_params *p) {
  if (!p) return "NULL argument";
  if (std::isnan(p->min_align_per) || std::isnan(p->max_edit_dist_per) || std::isnan(p->min_qc)) return "a coverage threshold is not a number";
  return "";
}

extern "C" int ckm_bam_open(const char *path, ckm_bam **out) {
  return guarded([&] {
    if (!path || !out) throw Error(CKM_EINVAL, "NULL argument");
    *out = nullptr;
    std::unique_ptr<ckm_bam> b(new ckm_bam());
    b->pool.reset(new HostPool(ingest_threads()));
    b->reader.reset(new bam::Reader(path, b->pool.get()));
    for (const std::string &n : b->reader->ref_names()) b->names.push_back(n.c_str());
    *out = b.release();
  });
}

extern "C" int ckm_bam_header(const ckm_bam *b, ckm_bam_header_view *out) {
  if (!b || !out) { set_last_error("NULL argument"); return CKM_EINVAL; }
  out->n_ref = (uint32_t)b->names.size();
  out->names = b->names.data(); out->lengths = b->reader->ref_lengths().data();
  out->header_bytes = b->reader->header_bytes();
  return CKM_OK;
}

extern "C" void ckm_bam_close(ckm_bam *b) { delete b; }

extern "C" int ckm_coverage_check(const ckm_coverage_params *params) {
  const std::string why = check_params(params);
  if (!why.empty()) { set_last_error(why); return CKM_EINVAL; }
  return CKM_OK;
}

namespace {

const char *const kRecordWhat[] = {"", "an auxiliary field runs past the record", "tag 'NM' not present", "tag 'NM' is not an integer", "an auxiliary field of unknown type",
                                   "the read has no CIGAR, so no aligned length", "a mapped read starts before its reference (pos < 0)"};

// The batch loop of both passes.  check: throws for bad arguments (before anything is touched); begin: allocates and clears the
// accumulators; launch: the kernel over one batch; end: what follows the last batch (scan, copies down).  A record the kernel could not
// walk ends the pass with a message that names the file, the ordinal and the read.
template <class Timing, class Check, class Begin, class Launch, class End>
int coverage_pass(ckm_ctx *ctx, ckm_bam *b, uint64_t budget_bytes, Timing *timing, Check &&check, Begin &&begin, Launch &&launch, End &&end) {
  CallStream ck;      // every phase is waited for (ck.timed): the reader's buffer is reused by the next batch
  return guarded([&] {
    check();
    memset(timing, 0, sizeof *timing);
    const WallClock t0;
    bam::Reader &rd = *b->reader;
    const uint64_t budget = bam::batch_budget(budget_bytes);
    ck.open(ctx->device);
    DevBuf d_data, d_off, d_err;
    uint64_t slot = cv::NO_ERROR;
    ck.timed(timing->ms_upload, [&] {
      begin(ck);
      ck.put(d_err, &slot, 8);
    });
    bam::Batch bt;
    while (rd.next(budget, bt)) {
      const size_t nrec = bt.offsets.size();
      ck.timed(timing->ms_upload, [&] {
        ck.put(d_data, bt.data, bt.bytes);
        ck.put(d_off, bt.offsets.data(), nrec * 4);
      });
      ck.timed(timing->ms_kernel, [&] {
        launch(ck.st, d_data.as<uint8_t>(), d_off.as<uint32_t>(), (uint32_t)nrec, bt.first_ordinal, d_err.as<unsigned long long>());
        HIPCHK(hipGetLastError());
      });
      ck.timed(timing->ms_download, [&] { HIPCHK(hipMemcpyAsync(&slot, d_err.p, 8, hipMemcpyDeviceToHost, ck.st)); });
      timing->records += nrec; timing->batches += 1;
      if (slot != cv::NO_ERROR) {
        const uint64_t ord = slot >> 3;
        const uint32_t reason = (uint32_t)(slot & 7);
        const uint8_t *rec = bt.data + bt.offsets[ord - bt.first_ordinal];
        const size_t ln = rec[12] ? rec[12] - 1 : 0;
        memcpy(timing->error_read, rec + cv::FIXED, std::min<size_t>(ln, sizeof timing->error_read - 1));
        timing->error_reason = reason; timing->error_record = ord;
        throw Error(CKM_EINVAL, rd.path() + ": record " + std::to_string(ord) + " (read '" + timing->error_read + "'): " + kRecordWhat[reason <= 6 ? reason : 0]);
      }
    }
    end(ck);
    timing->blocks = rd.blocks(); timing->inflated_bytes = rd.inflated();
    timing->ms_read = rd.timing.ms_read; timing->ms_inflate = rd.timing.ms_inflate; timing->ms_offsets = rd.timing.ms_offsets;
    timing->ms_total = t0.ms();
  });
}

}  // namespace

extern "C" int ckm_coverage_run(ckm_ctx *ctx, ckm_bam *b, const ckm_coverage_params *params, int64_t *out_counters, ckm_coverage_timing *timing) {
  DevBuf d_cnt;
  cv::Params P = {};
  size_t cbytes = 0;
  return coverage_pass(ctx, b, params ? params->budget_bytes : 0, timing,
    [&] {
      if (!ctx || !b || !out_counters || !timing) throw Error(CKM_EINVAL, "NULL argument");
      const std::string why = check_params(params);
      if (!why.empty()) throw Error(CKM_EINVAL, why);
      const uint64_t n_ref = b->reader->ref_names().size();
      P = {params->min_align_per, params->max_edit_dist_per, params->min_qc, params->all_reads ? 1 : 0, (int32_t)n_ref};
      cbytes = (size_t)n_ref * cv::NSLOT * 8;
    },
    [&](CallStream &ck) {
      d_cnt.ensure(cbytes + 8);
      HIPCHK(hipMemsetAsync(d_cnt.p, 0, cbytes + 8, ck.st));
    },
    [&](hipStream_t st, const uint8_t *data, const uint32_t *offsets, uint32_t nrec, uint64_t first_ordinal, unsigned long long *err_slot) {
      launch_coverage(st, data, offsets, nrec, first_ordinal, P, d_cnt.as<unsigned long long>(), err_slot);
    },
    [&](CallStream &ck) {
      if (cbytes) ck.timed(timing->ms_download, [&] { HIPCHK(hipMemcpyAsync(out_counters, d_cnt.p, cbytes, hipMemcpyDeviceToHost, ck.st)); });
    });
}

extern "C" int ckm_coverage_windows_check(const ckm_coverage_windows_params *params) {
  const std::string why = check_window_params(params);
  if (!why.empty()) { set_last_error(why); return CKM_EINVAL; }
  return CKM_OK;
}

extern "C" int ckm_coverage_windows_layout(const ckm_bam *b, int64_t window_size, int64_t *out_first) {
  return guarded([&] {
    if (!b || !out_first) throw Error(CKM_EINVAL, "NULL argument");
    if (window_size < 1 || window_size > cw::MAX_WINDOW) throw Error(CKM_EINVAL, "the window size must be between 1 and 2^31 - 1");
    window_layout(*b->reader, window_size, out_first);
  });
}

extern "C" int ckm_coverage_windows_run(ckm_ctx *ctx, ckm_bam *b, const ckm_coverage_windows_params *params, int64_t *out_counters, int64_t *out_window_sums,
                                        ckm_coverage_windows_timing *timing) {
  DevBuf d_cnt, d_len, d_first, d_direct, d_diff, d_sums;
  cw::Params P = {};
  std::vector<int64_t> first;
  size_t cbytes = 0, n_ref = 0, wbytes = 0;
  return coverage_pass(ctx, b, params ? params->budget_bytes : 0, timing,
    [&] {
      if (!ctx || !b || !out_counters || !out_window_sums || !timing) throw Error(CKM_EINVAL, "NULL argument");
      const std::string why = check_window_params(params);
      if (!why.empty()) throw Error(CKM_EINVAL, why);
      n_ref = b->reader->ref_names().size();
      first.assign(n_ref + 1, 0);
      window_layout(*b->reader, params->window_size, first.data());
      P = {params->min_align_per, params->max_edit_dist_per, params->all_reads ? 1 : 0, (int32_t)n_ref, (uint32_t)params->window_size};
      cbytes = n_ref * cv::NSLOT * 8; wbytes = (size_t)first[n_ref] * 8;
    },
    [&](CallStream &ck) {
      timing->slots = (uint64_t)first[n_ref];
      d_cnt.ensure(cbytes + 8); d_len.ensure(n_ref * 8 + 8); d_first.ensure(n_ref * 8 + 8); d_direct.ensure(wbytes + 8); d_diff.ensure(wbytes + 8);
      d_sums.ensure(((size_t)first[n_ref] + cw::SCAN_BLOCK - 1) / cw::SCAN_BLOCK * 8 + 8);
      HIPCHK(hipMemsetAsync(d_cnt.p, 0, cbytes + 8, ck.st));
      HIPCHK(hipMemsetAsync(d_direct.p, 0, wbytes + 8, ck.st));
      HIPCHK(hipMemsetAsync(d_diff.p, 0, wbytes + 8, ck.st));
      if (n_ref) HIPCHK(hipMemcpyAsync(d_len.p, b->reader->ref_lengths().data(), n_ref * 8, hipMemcpyHostToDevice, ck.st));
      HIPCHK(hipMemcpyAsync(d_first.p, first.data(), (n_ref + 1) * 8, hipMemcpyHostToDevice, ck.st));
    },
    [&](hipStream_t st, const uint8_t *data, const uint32_t *offsets, uint32_t nrec, uint64_t first_ordinal, unsigned long long *err_slot) {
      launch_covwin(st, data, offsets, nrec, first_ordinal, P, d_len.as<int64_t>(), d_first.as<int64_t>(), d_cnt.as<unsigned long long>(), d_direct.as<unsigned long long>(),
                    d_diff.as<unsigned long long>(), err_slot);
    },
    [&](CallStream &ck) {
      ck.timed(timing->ms_scan, [&] {
        launch_covwin_scan(ck.st, d_direct.as<unsigned long long>(), d_diff.as<unsigned long long>(), d_sums.as<unsigned long long>(), (uint32_t)first[n_ref]);
        HIPCHK(hipGetLastError());
      });
      ck.timed(timing->ms_download, [&] {
        if (cbytes) HIPCHK(hipMemcpyAsync(out_counters, d_cnt.p, cbytes, hipMemcpyDeviceToHost, ck.st));
        if (wbytes) HIPCHK(hipMemcpyAsync(out_window_sums, d_direct.p, wbytes, hipMemcpyDeviceToHost, ck.st));
      });
    });
}
