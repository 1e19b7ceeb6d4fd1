// refdist_emu.cpp -- TEST INFRASTRUCTURE: the geometry of the reference-distribution pass (checkm_amd/csrc/refdist_dev.h), the per-lane
// step of seqwin_dev.h and the distance of outlier_dev.h compiled by g++ against a HOST executor, so that the CPU test suite can compare
// them with the plain-Python restatement.  The kernels of kernels_refdist.hip are restated as loops over their wavefronts and lanes: a
// lane's halo bytes come from the next lane's word as on the device, every block fills its row, the scan runs per column with a carry
// across steps of 64, a window is its prefix difference plus its edges, the TD batches follow the same byte budget.  Built with
// -ffp-contract=off like the library.  Nothing in checkm_amd loads this.
#include <algorithm>
#include <cstring>
#include <vector>
#include "../../checkm_amd/csrc/outlier_dev.h"
#include "../../checkm_amd/csrc/refdist_dev.h"

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

// one wavefront over one piece: rd_wave_piece of kernels_refdist.hip
void wave_piece(const uint8_t *text, const sw::Piece &P, bool kmers, const uint8_t *canon, uint32_t *hist, uint32_t *acc) {
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
}
}  // namespace

// ckm_refdist_run on the host.  info: windows, blocks, batches, scaffold bytes.  Returns 0, -1 for a refused argument (-7 for a scaffold
// or a window count beyond the limits).
extern "C" int emu_refdist_run(const char *text, const uint64_t *seq_off, const uint64_t *seq_bytes, uint32_t nseq, int stat, uint32_t sep_len, uint32_t block,
                               const int64_t *starts, const int64_t *sizes, uint64_t nwin, uint64_t budget_bytes, uint32_t *out_counts, double *out_td,
                               uint64_t *out_totals, uint64_t *info) {
  const uint64_t L = rd::scaffold_len(seq_bytes, nseq, sep_len);
  if (!rd::check_args(stat, sep_len, block, L, starts, sizes, nwin).empty()) return rd::refusal_code(L, nwin);
  if (!budget_bytes) return -1;
  if (block == 0) block = rd::DEFAULT_BLOCK;
  const bool td = stat == rd::STAT_TD;
  std::vector<uint8_t> scaf;
  rd::join_scaffold(text, seq_off, seq_bytes, nseq, sep_len, scaf);
  uint8_t canon[256];
  ns::canonical_table(canon);
  const uint32_t nblocks = (uint32_t)((L + block - 1) / block), ncol = rd::ncol_of(stat);
  std::vector<uint32_t> rows(((size_t)nblocks + 1) * ncol, 0);
  for (uint32_t b = 0; b < nblocks; ++b) {
    uint32_t hist[rd::NKMER] = {0}, acc[4] = {0, 0, 0, 0};
    wave_piece(scaf.data(), rd::block_piece(b, block, L), td, canon, hist, acc);
    if (td) memcpy(&rows[(size_t)b * ncol], hist, sizeof(hist));
    else { rows[(size_t)b * 2] = acc[1] + acc[2]; rows[(size_t)b * 2 + 1] = acc[0] + acc[3]; }
  }
  for (uint32_t col = 0; col < ncol; ++col) {
    uint32_t carry = 0;
    for (uint32_t base = 0; base < nblocks; base += sw::WAVE) {
      uint32_t incl = 0;
      for (uint32_t t = base; t < std::min<uint32_t>(nblocks, base + sw::WAVE); ++t) {
        const uint32_t v = rows[(size_t)t * ncol + col];
        rows[(size_t)t * ncol + col] = carry + incl;
        incl += v;
      }
      carry += incl;
    }
    rows[(size_t)nblocks * ncol + col] = carry;
  }
  for (int k = 0; k < rd::NTOTALS; ++k) out_totals[k] = 0;
  double sig[ol::NSIG];
  if (td) {
    uint64_t sum = 0;
    for (int k = 0; k < rd::NKMER; ++k) { out_totals[2 + k] = rows[(size_t)nblocks * ncol + k]; sum += out_totals[2 + k]; }
    for (int k = 0; k < ol::NSIG; ++k) sig[k] = ol::ratio(out_totals[2 + k], sum);
  } else {
    out_totals[0] = rows[(size_t)nblocks * 2]; out_totals[1] = rows[(size_t)nblocks * 2 + 1];
  }
  const uint64_t max_windows = std::max<uint64_t>(1, std::min<uint64_t>(budget_bytes / rd::TD_ROW_BYTES, rd::MAX_WINDOWS));
  const uint64_t per_launch = td ? max_windows : rd::MAX_WINDOWS;
  std::vector<uint32_t> tet;
  info[2] = 0;
  for (uint64_t win0 = 0; win0 < nwin; win0 += per_launch) {
    const uint64_t n = std::min<uint64_t>(per_launch, nwin - win0);
    if (td) tet.assign((size_t)n * rd::NKMER, 0xDEADBEEFu);
    for (uint64_t x = 0; x < n; ++x) {
      const rd::WindowGeom g = rd::window_geom((uint64_t)starts[win0 + x], (uint64_t)sizes[win0 + x], stat, block);
      uint32_t hist[rd::NKMER] = {0}, acc[4] = {0, 0, 0, 0};
      wave_piece(scaf.data(), g.edge[0], td, canon, hist, acc);
      wave_piece(scaf.data(), g.edge[1], td, canon, hist, acc);
      if (td) {
        for (int k = 0; k < rd::NKMER; ++k)
          tet[(size_t)x * rd::NKMER + k] = hist[k] + (g.whole ? rows[(size_t)g.b1 * ncol + k] - rows[(size_t)g.b0 * ncol + k] : 0u);
      } else {
        uint32_t gc = acc[1] + acc[2], at = acc[0] + acc[3];
        if (g.whole) { gc += rows[(size_t)g.b1 * 2] - rows[(size_t)g.b0 * 2]; at += rows[(size_t)g.b1 * 2 + 1] - rows[(size_t)g.b0 * 2 + 1]; }
        out_counts[(win0 + x) * 2] = gc; out_counts[(win0 + x) * 2 + 1] = at;
      }
    }
    if (td)
      for (uint64_t x = 0; x < n; ++x) out_td[win0 + x] = td_of(&tet[(size_t)x * rd::NKMER], sig);
    info[2] += 1;
  }
  info[0] = nwin; info[1] = nblocks; info[3] = L;
  return 0;
}
