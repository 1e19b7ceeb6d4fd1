// ckm_seqwin.hip -- C ABI of the sequence-window pass (kernels_seqwin.hip): a batch read by ckm_nucseq_read in; per window the base
// counts and the tetranucleotide distance to its file's bin signature out, per sequence the base counts.  The text goes up once; the
// windows go through the device in batches whose 136-count rows fit a byte budget, and only four uint32 and one double per window stay.
#include <cstdlib>
#include <vector>
#include "ckm_host.h"
#include "nucstats_host.h"
#include "outlier_dev.h"
#include "seqwin_dev.h"

namespace ckm {
void launch_seqwin_count(hipStream_t st, const uint8_t *text, const sw::Piece *pieces, uint32_t npieces, const uint8_t *canon, uint32_t *cnt, uint32_t *tet);
void launch_seqwin_td(hipStream_t st, uint32_t nwin, const uint32_t *tet, const uint32_t *win_file, const double *bin_sig, double *td);
}  // namespace ckm
using namespace ckm;

extern "C" int ckm_seq_windows_run(ckm_ctx *ctx, const ckm_nucseq *b, int64_t window_size, int tetra, const double *bin_sig, uint32_t piece_bytes,
                                   uint64_t budget_bytes, uint32_t *out_base_counts, uint64_t *out_seq_counts, double *out_td, uint32_t *out_tetra_counts,
                                   uint8_t *out_skipped, ckm_seq_windows_timing *timing) {
  CallStream cs;
  return guarded([&] {
    if (!ctx || !b || !out_base_counts || !out_seq_counts || !out_skipped || !timing) throw Error(CKM_EINVAL, "NULL argument");
    if (window_size < 1 || (uint64_t)window_size > sw::MAX_WINDOWS) throw Error(CKM_EINVAL, "window_size must be between 1 and 2^31 - 1");
    if (!tetra && (bin_sig || out_td || out_tetra_counts)) throw Error(CKM_EINVAL, "bin_sig, out_td and out_tetra_counts need tetra != 0");
    if (tetra && ((bin_sig == nullptr) != (out_td == nullptr) || (!out_td && !out_tetra_counts))) throw Error(CKM_EINVAL, "tetra != 0 needs bin_sig with out_td, or out_tetra_counts");
    if (piece_bytes == 0) piece_bytes = sw::DEFAULT_PIECE;
    if (piece_bytes < sw::MIN_PIECE || piece_bytes > (1u << 20)) throw Error(CKM_EINVAL, "piece_bytes must be between 16 and 1 MiB");
    budget_bytes = batch_budget(budget_bytes, "CKM_NUCSTATS_BATCH_MB", 1024);
    const WallClock t0;
    *timing = ckm_seq_windows_timing{};
    const uint32_t nseq = (uint32_t)b->seq_off.size(), nfiles = (uint32_t)b->file_first.size() - 1;
    const uint64_t w = (uint64_t)window_size;
    // geometry: code points, the sequences the kernel does not take, the first window of every sequence
    const std::vector<uint64_t> &len = b->seq_cp;
    std::vector<uint64_t> first;
    window_layout(b, w, first);
    std::vector<uint32_t> seq_file(nseq);
    for (uint32_t f = 0; f < nfiles; ++f)
      for (uint32_t s = b->file_first[f]; s < b->file_first[f + 1]; ++s) seq_file[s] = f;
    uint64_t skipped = 0;
    for (uint32_t s = 0; s < nseq; ++s) {
      out_skipped[s] = len[s] != b->seq_bytes[s];
      skipped += out_skipped[s];
    }
    const uint64_t nwin = first[nseq], nrows = nwin + nseq;
    if (nrows > 0xFFFFFFF0ull) throw Error(CKM_ERANGE, "too many windows and sequences in one call");
    if (out_tetra_counts && nwin * sw::ROW_BYTES > budget_bytes)
      throw Error(CKM_ERANGE, "out_tetra_counts of " + std::to_string(nwin) + " windows needs " + std::to_string(nwin * sw::ROW_BYTES) + " bytes, more than the budget of " +
                                  std::to_string(budget_bytes));
    const uint64_t max_windows = std::max<uint64_t>(1, std::min<uint64_t>(budget_bytes / sw::ROW_BYTES, sw::MAX_WINDOWS));
    std::vector<uint32_t> cnt((size_t)nrows * 4, 0);
    if (nseq) {
      cs.open(ctx->device);
      uint8_t canon[256];
      ns::canonical_table(canon);
      const size_t scratch_rows = (size_t)std::min<uint64_t>(max_windows, std::max<uint64_t>(1, nwin));
      DevBuf d_text, d_canon, d_cnt, d_td, d_tet, d_binsig, d_pieces, d_file;
      d_cnt.ensure((size_t)nrows * 16);
      if (tetra) d_tet.ensure(scratch_rows * sw::ROW_BYTES);
      if (out_td) { d_td.ensure(std::max<size_t>(1, nwin) * 8); d_binsig.ensure(std::max<size_t>(1, nfiles) * ol::NSIG * 8); }
      cs.mark(0);
      cs.put(d_text, b->text.data(), b->text.size());
      cs.put(d_canon, canon, 256);
      HIPCHK(hipMemsetAsync(d_cnt.p, 0, (size_t)nrows * 16, cs.st));
      if (out_td && nfiles) HIPCHK(hipMemcpyAsync(d_binsig.p, bin_sig, (size_t)nfiles * ol::NSIG * 8, hipMemcpyHostToDevice, cs.st));
      cs.mark(1);
      HIPCHK(hipStreamSynchronize(cs.st));
      timing->ms_upload += cs.ms(0, 1);
      sw::Cursor cur;
      sw::Batch B;
      while (sw::next_batch(b->seq_off.data(), len.data(), out_skipped, seq_file.data(), nseq, w, piece_bytes, max_windows, nwin, cur, B)) {
        if (B.pieces.size() > 0x7FFFFFF0ull) throw Error(CKM_ERANGE, "too many pieces in one batch: use a larger piece_bytes");
        const uint32_t np = (uint32_t)B.pieces.size();
        d_pieces.ensure(std::max<size_t>(1, np) * sizeof(sw::Piece)); d_file.ensure(std::max<size_t>(1, B.nwin) * 4);
        cs.mark(0);
        if (np) HIPCHK(hipMemcpyAsync(d_pieces.p, B.pieces.data(), (size_t)np * sizeof(sw::Piece), hipMemcpyHostToDevice, cs.st));
        if (out_td && B.nwin) HIPCHK(hipMemcpyAsync(d_file.p, B.win_file.data(), (size_t)B.nwin * 4, hipMemcpyHostToDevice, cs.st));
        if (tetra && B.nwin) HIPCHK(hipMemsetAsync(d_tet.p, 0, (size_t)B.nwin * sw::ROW_BYTES, cs.st));
        cs.mark(1);
        launch_seqwin_count(cs.st, d_text.as<uint8_t>(), d_pieces.as<sw::Piece>(), np, d_canon.as<uint8_t>(), d_cnt.as<uint32_t>(), tetra ? d_tet.as<uint32_t>() : nullptr);
        HIPCHK(hipGetLastError());
        cs.mark(2);
        if (out_td) {
          launch_seqwin_td(cs.st, B.nwin, d_tet.as<uint32_t>(), d_file.as<uint32_t>(), d_binsig.as<double>(), d_td.as<double>() + B.win0);
          HIPCHK(hipGetLastError());
        }
        cs.mark(3);
        if (out_tetra_counts && B.nwin)
          HIPCHK(hipMemcpyAsync(out_tetra_counts + B.win0 * sw::NKMER, d_tet.p, (size_t)B.nwin * sw::ROW_BYTES, hipMemcpyDeviceToHost, cs.st));
        HIPCHK(hipStreamSynchronize(cs.st));
        timing->ms_upload += cs.ms(0, 1);
        timing->ms_count += cs.ms(1, 2);
        timing->ms_td += cs.ms(2, 3);
        timing->pieces += np; timing->batches += 1;
      }
      cs.mark(0);
      if (nrows) HIPCHK(hipMemcpyAsync(cnt.data(), d_cnt.p, (size_t)nrows * 16, hipMemcpyDeviceToHost, cs.st));
      if (out_td && nwin) HIPCHK(hipMemcpyAsync(out_td, d_td.p, (size_t)nwin * 8, hipMemcpyDeviceToHost, cs.st));
      cs.mark(1);
      HIPCHK(hipStreamSynchronize(cs.st));
      timing->ms_download += cs.ms(0, 1);
    }
    if (nwin) memcpy(out_base_counts, cnt.data(), (size_t)nwin * 16);
    sw::seq_counts(cnt.data(), first.data(), nseq, out_seq_counts);
    timing->windows = nwin; timing->bytes = b->text.size(); timing->skipped_seqs = skipped;
    timing->ms_total = t0.ms();
  });
}
