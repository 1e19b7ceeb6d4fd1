// ckm_refdist.hip -- C ABI of the reference-distribution pass (kernels_refdist.hip): a genome read by ckm_nucseq_read and a list of
// windows (start, size) of its scaffold in; per window two counters (GC, CD) or the tetranucleotide distance to the genome's signature
// (TD) out, and the totals of the scaffold.  The scaffold is joined on the host while the upload buffer is filled and goes up once; the
// prefix rows stay on the device; the 136-count rows of the TD windows go through seqwin_td_kernel in batches that fit a byte budget.
#include <cstdlib>
#include <vector>
#include "ckm_host.h"
#include "nucstats_host.h"
#include "outlier_dev.h"
#include "refdist_dev.h"

namespace ckm {
void launch_refdist_blocks(hipStream_t st, const uint8_t *text, uint64_t L, uint32_t block, uint32_t nblocks, int td, const uint8_t *canon, uint32_t *rows);
void launch_refdist_scan(hipStream_t st, uint32_t *rows, uint32_t nblocks, uint32_t ncol);
void launch_refdist_windows(hipStream_t st, const uint8_t *text, uint32_t block, int stat, const uint32_t *starts, const uint32_t *sizes, uint64_t win0, uint32_t nwin,
                            const uint8_t *canon, const uint32_t *rows, uint32_t *cnt, uint32_t *tet);
void launch_seqwin_td(hipStream_t st, uint32_t nwin, const uint32_t *tet, const uint32_t *win_file, const double *bin_sig, double *td);
}  // namespace ckm
using namespace ckm;

extern "C" int ckm_refdist_run(ckm_ctx *ctx, const ckm_nucseq *b, int stat, uint32_t sep_len, uint32_t block, const int64_t *starts, const int64_t *sizes, uint64_t nwin,
                               uint64_t budget_bytes, uint32_t *out_counts, double *out_td, uint64_t *out_totals, ckm_refdist_timing *timing) {
  CallStream cs;
  return guarded([&] {
    if (!ctx || !b || !out_totals || !timing) throw Error(CKM_EINVAL, "NULL argument");
    const uint32_t nseq = (uint32_t)b->seq_off.size();
    const uint64_t L = rd::scaffold_len(b->seq_bytes.data(), nseq, sep_len);
    const std::string refusal = rd::check_args(stat, sep_len, block, L, starts, sizes, nwin);
    if (!refusal.empty()) throw Error(rd::refusal_code(L, nwin), refusal);
    const bool td = stat == rd::STAT_TD;
    if (td ? !out_td : !out_counts) throw Error(CKM_EINVAL, td ? "stat td needs out_td" : "stat gc / cd needs out_counts");
    for (uint32_t s = 0; s < nseq; ++s)
      if (b->seq_cp[s] != b->seq_bytes[s]) throw Error(CKM_EINVAL, "sequence " + b->ids[s] + " holds non-ASCII characters: its scaffold is not taken");
    if (block == 0) block = rd::DEFAULT_BLOCK;
    budget_bytes = batch_budget(budget_bytes, "CKM_NUCSTATS_BATCH_MB", 1024);
    const WallClock t0;
    *timing = ckm_refdist_timing{};
    std::vector<uint8_t> text;
    rd::join_scaffold(b->text.data(), b->seq_off.data(), b->seq_bytes.data(), nseq, sep_len, text);
    std::vector<uint32_t> s32((size_t)std::max<uint64_t>(1, nwin)), w32((size_t)std::max<uint64_t>(1, nwin));
    for (uint64_t x = 0; x < nwin; ++x) { s32[x] = (uint32_t)starts[x]; w32[x] = (uint32_t)sizes[x]; }
    timing->ms_scaffold = t0.ms();
    const uint32_t nblocks = (uint32_t)((L + block - 1) / block), ncol = rd::ncol_of(stat);
    const size_t row_bytes = (size_t)ncol * 4, rows_bytes = ((size_t)nblocks + 1) * row_bytes;
    const uint64_t max_windows = std::max<uint64_t>(1, std::min<uint64_t>(budget_bytes / rd::TD_ROW_BYTES, rd::MAX_WINDOWS));
    const size_t scratch_rows = (size_t)std::min<uint64_t>(max_windows, std::max<uint64_t>(1, nwin));
    std::vector<uint32_t> totals(ncol, 0);
    cs.open(ctx->device);
    uint8_t canon[256];
    ns::canonical_table(canon);
    DevBuf d_text, d_canon, d_rows, d_starts, d_sizes, d_cnt, d_tet, d_td, d_file, d_sig;
    d_rows.ensure(rows_bytes);
    if (td) { d_tet.ensure(scratch_rows * rd::TD_ROW_BYTES); d_td.ensure(s32.size() * 8); d_file.ensure(scratch_rows * 4); }
    else d_cnt.ensure(s32.size() * 8);
    cs.mark(0);
    cs.put(d_text, text.data(), text.size());
    cs.put(d_canon, canon, 256);
    cs.put(d_starts, s32.data(), s32.size() * 4);
    cs.put(d_sizes, w32.data(), w32.size() * 4);
    if (td) HIPCHK(hipMemsetAsync(d_file.p, 0, scratch_rows * 4, cs.st));      // every window is compared with signature 0: the genome's
    cs.mark(1);
    launch_refdist_blocks(cs.st, d_text.as<uint8_t>(), L, block, nblocks, td ? 1 : 0, d_canon.as<uint8_t>(), d_rows.as<uint32_t>());
    HIPCHK(hipGetLastError());
    cs.mark(2);
    launch_refdist_scan(cs.st, d_rows.as<uint32_t>(), nblocks, ncol);
    HIPCHK(hipGetLastError());
    cs.mark(3);
    HIPCHK(hipMemcpyAsync(totals.data(), d_rows.as<uint8_t>() + (size_t)nblocks * row_bytes, row_bytes, hipMemcpyDeviceToHost, cs.st));
    HIPCHK(hipStreamSynchronize(cs.st));
    timing->ms_upload += cs.ms(0, 1);
    timing->ms_blocks += cs.ms(1, 2);
    timing->ms_scan += cs.ms(2, 3);
    for (int k = 0; k < rd::NTOTALS; ++k) out_totals[k] = 0;
    if (td) {
      // genomeSig = seqSignature(scaffold): every count over their sum, one division each
      uint64_t sum = 0;
      for (int k = 0; k < rd::NKMER; ++k) { out_totals[2 + k] = totals[k]; sum += totals[k]; }
      double sig[ol::NSIG];
      for (int k = 0; k < ol::NSIG; ++k) sig[k] = ol::ratio((uint64_t)totals[k], sum);
      cs.put(d_sig, sig, sizeof(sig));
      HIPCHK(hipStreamSynchronize(cs.st));
    } else {
      out_totals[0] = totals[0]; out_totals[1] = totals[1];
    }
    const uint64_t per_launch = td ? max_windows : rd::MAX_WINDOWS;   // two counters per window need no scratch: one launch takes them all
    for (uint64_t win0 = 0; win0 < nwin; win0 += per_launch) {
      const uint32_t n = (uint32_t)std::min<uint64_t>(per_launch, nwin - win0);
      cs.mark(0);
      launch_refdist_windows(cs.st, d_text.as<uint8_t>(), block, stat, d_starts.as<uint32_t>(), d_sizes.as<uint32_t>(), win0, n, d_canon.as<uint8_t>(),
                             d_rows.as<uint32_t>(), td ? nullptr : d_cnt.as<uint32_t>(), td ? d_tet.as<uint32_t>() : nullptr);
      HIPCHK(hipGetLastError());
      if (td) {
        launch_seqwin_td(cs.st, n, d_tet.as<uint32_t>(), d_file.as<uint32_t>(), d_sig.as<double>(), d_td.as<double>() + win0);
        HIPCHK(hipGetLastError());
      }
      cs.mark(1);
      HIPCHK(hipStreamSynchronize(cs.st));
      timing->ms_windows += cs.ms(0, 1);
      timing->batches += 1;
    }
    cs.mark(0);
    if (nwin && td) HIPCHK(hipMemcpyAsync(out_td, d_td.p, (size_t)nwin * 8, hipMemcpyDeviceToHost, cs.st));
    if (nwin && !td) HIPCHK(hipMemcpyAsync(out_counts, d_cnt.p, (size_t)nwin * 8, hipMemcpyDeviceToHost, cs.st));
    cs.mark(1);
    HIPCHK(hipStreamSynchronize(cs.st));
    timing->ms_download += cs.ms(0, 1);
    timing->windows = nwin; timing->blocks = nblocks; timing->bytes = L;
    timing->ms_total = t0.ms();
  });
}
