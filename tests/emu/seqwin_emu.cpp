// seqwin_emu.cpp -- TEST INFRASTRUCTURE: the piece logic of the sequence-window pass (checkm_amd/csrc/seqwin_dev.h) and the distance of
// checkm_amd/csrc/outlier_dev.h compiled by g++ against a HOST executor, so that the CPU test suite can compare them with the plain-Python
// restatement.  The kernels of kernels_seqwin.hip are restated as loops over their wavefronts and lanes: a lane's halo bytes come from
// the next lane's word as on the device, the window rows are filled piece by piece, the batches follow the same byte budget.  Built
// with -ffp-contract=off like the library.  Nothing in checkm_amd loads this.
#include <cstring>
#include <vector>
#include "../../checkm_amd/csrc/outlier_dev.h"
#include "../../checkm_amd/csrc/seqwin_dev.h"

using namespace ckm;

namespace {
struct ArrayPartner {
  const double *r; int lane;
  static double held(const double *r, int l, int p) {
    if (p == 1) return r[l];
    return held(r, l, p >> 1) + held(r, l ^ (p >> 1), p >> 1);
  }
  double operator()(double, int p) const { return held(r, lane ^ p, p); }
};

double td_of(const uint32_t *row, const double *bin) {
  double sig[ol::NSIG];
  uint32_t total = 0;
  for (int k = 0; k < ol::NSIG; ++k) total += row[k];
  for (int k = 0; k < ol::NSIG; ++k) sig[k] = ol::ratio((uint64_t)row[k], (uint64_t)total);
  double half[2];
  for (int h = 0; h < 2; ++h) {
    const int first = h ? ol::TD_SPLIT : 0, count = h ? ol::NSIG - ol::TD_SPLIT : ol::TD_SPLIT;
    double r[ol::TD_ACC];
    for (int l = 0; l < ol::TD_ACC; ++l) r[l] = ol::td_running(sig, bin, first, count, l);
    half[h] = ol::td_combine(r[0], ArrayPartner{r, 0});
  }
  return half[0] + half[1];
}

// one wavefront over one piece
void run_piece(const uint8_t *text, const sw::Piece &P, const uint8_t *canon, uint32_t *cnt, uint32_t *tet) {
  uint32_t hist[sw::NKMER] = {0}, acc[4] = {0, 0, 0, 0};
  const bool kmers = tet != nullptr && P.tet_row != sw::NO_ROW;
  const uint64_t pend = P.start + P.len;
  for (uint64_t step = P.start & ~(uint64_t)(sw::LANE_BYTES - 1); step < pend; step += sw::WAVE_BYTES) {
    sw::LaneGeom g[sw::WAVE];
    for (int lane = 0; lane < sw::WAVE; ++lane) g[lane] = sw::lane_geom(P, step, lane);
    for (int lane = 0; lane < sw::WAVE; ++lane) {
      uint8_t b[sw::LANE_BYTES + sw::HALO] = {0};
      if (g[lane].load) memcpy(b, text + g[lane].base, sw::LANE_BYTES);
      if (lane < sw::WAVE - 1) { if (g[lane + 1].load) memcpy(b + sw::LANE_BYTES, text + g[lane + 1].base, sw::HALO); }
      else if (g[lane].kend > sw::LANE_BYTES) memcpy(b + sw::LANE_BYTES, text + g[lane].base + sw::LANE_BYTES, sw::HALO);
      sw::Lane o;
      sw::lane_step(b, g[lane].first, g[lane].end, g[lane].kend, o);
      for (int k = 0; k < 4; ++k) acc[k] += o.cnt[k];
      if (kmers)
        for (uint32_t m = o.kmer_mask; m; m &= m - 1) hist[canon[o.code[__builtin_ctz(m)]]] += 1;
    }
  }
  const bool alone = (P.flags & 4u) != 0;
  uint32_t *row = cnt + (uint64_t)P.cnt_row * 4;
  for (int k = 0; k < 4; ++k) { if (alone) row[k] = acc[k]; else row[k] += acc[k]; }
  if (kmers) {
    uint32_t *trow = tet + (uint64_t)P.tet_row * sw::NKMER;
    for (int k = 0; k < sw::NKMER; ++k) { if (alone) trow[k] = hist[k]; else trow[k] += hist[k]; }
  }
}
}  // namespace

// ckm_seq_windows_run on the host.  info: windows, pieces, batches, skipped sequences.  Returns 0, or -7 for too many windows / an
// out_tetra that does not fit the budget, -1 for a bad argument.
extern "C" int emu_seq_windows_run(const char *text, const uint64_t *seq_off, const uint64_t *seq_bytes, const uint32_t *file_first, uint32_t nseq, uint32_t nfiles,
                                   int64_t window_size, int tetra, const double *bin_sig, uint32_t piece_bytes, uint64_t budget_bytes, uint32_t *out_base,
                                   uint64_t *out_seq, double *out_td, uint32_t *out_tetra, uint8_t *out_skipped, uint64_t *info) {
  if (window_size < 1 || (uint64_t)window_size > sw::MAX_WINDOWS || piece_bytes < sw::MIN_PIECE || !budget_bytes) return -1;
  const uint64_t w = (uint64_t)window_size;
  std::vector<uint64_t> len(nseq), first;
  for (uint32_t s = 0; s < nseq; ++s) len[s] = sw::code_points(text, seq_off[s], seq_bytes[s]);
  if (!sw::window_layout(len.data(), nseq, w, first)) return -7;
  std::vector<uint32_t> seq_file(nseq);
  for (uint32_t f = 0; f < nfiles; ++f)
    for (uint32_t s = file_first[f]; s < file_first[f + 1]; ++s) seq_file[s] = f;
  uint64_t skipped = 0;
  for (uint32_t s = 0; s < nseq; ++s) {
    out_skipped[s] = len[s] != seq_bytes[s];
    skipped += out_skipped[s];
  }
  const uint64_t nwin = first[nseq], nrows = nwin + nseq;
  if (out_tetra && nwin * sw::ROW_BYTES > budget_bytes) return -7;
  const uint64_t max_windows = std::max<uint64_t>(1, std::min<uint64_t>(budget_bytes / sw::ROW_BYTES, sw::MAX_WINDOWS));
  uint8_t canon[256];
  ns::canonical_table(canon);
  std::vector<uint32_t> cnt((size_t)nrows * 4, 0), scratch;
  sw::Cursor cur;
  sw::Batch B;
  info[1] = info[2] = 0;
  while (sw::next_batch(seq_off, len.data(), out_skipped, seq_file.data(), nseq, w, piece_bytes, max_windows, nwin, cur, B)) {
    if (tetra) scratch.assign((size_t)B.nwin * sw::NKMER, 0);
    for (const sw::Piece &P : B.pieces) run_piece((const uint8_t *)text, P, canon, cnt.data(), tetra ? scratch.data() : nullptr);
    if (out_td)
      for (uint32_t x = 0; x < B.nwin; ++x) out_td[B.win0 + x] = td_of(&scratch[(size_t)x * sw::NKMER], bin_sig + (size_t)B.win_file[x] * ol::NSIG);
    if (out_tetra && B.nwin) memcpy(out_tetra + B.win0 * sw::NKMER, scratch.data(), (size_t)B.nwin * sw::ROW_BYTES);
    info[1] += B.pieces.size(); info[2] += 1;
  }
  if (nwin) memcpy(out_base, cnt.data(), (size_t)nwin * 16);
  sw::seq_counts(cnt.data(), first.data(), nseq, out_seq);
  info[0] = nwin; info[3] = skipped;
  return 0;
}
