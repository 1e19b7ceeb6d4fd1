// ckm_coverage.hip -- C ABI of `checkm coverage`: the BAM handle (bam_host.cpp; no device) and the device pass over its records
// (kernels_coverage.hip).  Batch by batch: the host inflates a batch, the records and their offsets go up, the kernel adds to the
// per-reference counters; every phase is waited for (the reader's buffer is reused by the next batch), so inflating and the kernel do
// not overlap.  The counters come down once, at the end.
#include <chrono>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>
#include "ckm_host.h"
#include "bam_host.h"
#include "coverage_dev.h"

namespace ckm {
void launch_coverage(hipStream_t st, const uint8_t *data, const uint32_t *offsets, uint32_t nrec, uint64_t first_ordinal, const cv::Params &P,
                     unsigned long long *counters, unsigned long long *err_slot);
}

struct ckm_bam {
  std::unique_ptr<HostPool> pool;
  std::unique_ptr<bam::Reader> reader;
  std::vector<const char *> names;
};

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

extern "C" int ckm_coverage_run(ckm_ctx *ctx, ckm_bam *b, const ckm_coverage_params *params, int64_t *out_counters, ckm_coverage_timing *timing) {
  hipStream_t st = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};
  const int rc = guarded([&] {
    if (!ctx || !b || !out_counters || !timing) throw Error(CKM_EINVAL, "NULL argument");
    const std::string why = check_params(params);
    if (!why.empty()) throw Error(CKM_EINVAL, why);
    memset(timing, 0, sizeof *timing);
    const auto t0 = std::chrono::steady_clock::now();
    bam::Reader &rd = *b->reader;
    const uint64_t n_ref = rd.ref_names().size(), budget = bam::batch_budget(params->budget_bytes);
    const cv::Params P = {params->min_align_per, params->max_edit_dist_per, params->min_qc, params->all_reads ? 1 : 0, (int32_t)n_ref};
    const size_t cbytes = (size_t)n_ref * cv::NSLOT * 8;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    for (auto &e : ev) HIPCHK(hipEventCreate(&e));
    // a phase between two events; the wait is part of the design: the reader's buffer is reused by the next batch
    auto timed = [&](double &acc, auto &&fn) {
      HIPCHK(hipEventRecord(ev[0], st));
      fn();
      HIPCHK(hipEventRecord(ev[1], st));
      HIPCHK(hipEventSynchronize(ev[1]));
      float ms = 0; HIPCHK(hipEventElapsedTime(&ms, ev[0], ev[1]));
      acc += ms;
    };
    DevBuf d_data, d_off, d_cnt, d_err;
    d_cnt.ensure(cbytes + 8); d_err.ensure(8);
    uint64_t slot = cv::NO_ERROR;
    timed(timing->ms_upload, [&] {
      HIPCHK(hipMemsetAsync(d_cnt.p, 0, cbytes + 8, st));
      HIPCHK(hipMemcpyAsync(d_err.p, &slot, 8, hipMemcpyHostToDevice, st));
    });
    bam::Batch bt;
    while (rd.next(budget, bt)) {
      const size_t nrec = bt.offsets.size();
      d_data.ensure(bt.bytes); d_off.ensure(nrec * 4);
      timed(timing->ms_upload, [&] {
        HIPCHK(hipMemcpyAsync(d_data.p, bt.data, bt.bytes, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_off.p, bt.offsets.data(), nrec * 4, hipMemcpyHostToDevice, st));
      });
      timed(timing->ms_kernel, [&] {
        launch_coverage(st, d_data.as<uint8_t>(), d_off.as<uint32_t>(), (uint32_t)nrec, bt.first_ordinal, P, d_cnt.as<unsigned long long>(), d_err.as<unsigned long long>());
        HIPCHK(hipGetLastError());
      });
      timed(timing->ms_download, [&] { HIPCHK(hipMemcpyAsync(&slot, d_err.p, 8, hipMemcpyDeviceToHost, st)); });
      timing->records += nrec; timing->batches += 1;
      if (slot != cv::NO_ERROR) {
        const uint64_t ord = slot >> 3;
        const uint32_t reason = (uint32_t)(slot & 7);
        const uint8_t *rec = bt.data + bt.offsets[ord - bt.first_ordinal];
        const size_t ln = rec[12] ? rec[12] - 1 : 0;
        memcpy(timing->error_read, rec + cv::FIXED, std::min<size_t>(ln, sizeof timing->error_read - 1));
        timing->error_reason = reason; timing->error_record = ord;
        static const char *const what[] = {"", "an auxiliary field runs past the record", "tag 'NM' not present", "tag 'NM' is not an integer", "an auxiliary field of unknown type"};
        throw Error(CKM_EINVAL, rd.path() + ": record " + std::to_string(ord) + " (read '" + timing->error_read + "'): " + what[reason <= 4 ? reason : 0]);
      }
    }
    if (cbytes) timed(timing->ms_download, [&] { HIPCHK(hipMemcpyAsync(out_counters, d_cnt.p, cbytes, hipMemcpyDeviceToHost, st)); });
    timing->blocks = rd.blocks(); timing->inflated_bytes = rd.inflated();
    timing->ms_read = rd.timing.ms_read; timing->ms_inflate = rd.timing.ms_inflate; timing->ms_offsets = rd.timing.ms_offsets;
    timing->ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  });
  for (auto &e : ev) if (e) (void)hipEventDestroy(e);
  if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
  return rc;
}
