// merge_emu.cpp -- TEST INFRASTRUCTURE: the all-pairs comparison of `checkm merge` (checkm_amd/csrc/merge_dev.h, merge_host.h, pairs_dev.h) compiled by
// g++ against a HOST executor, so that the CPU test suite runs the arithmetic, the placement of the reported pairs and the split into
// output batches of the library.  The kernels of kernels_merge.hip are restated as loops over their tiles, wavefronts and lanes: a
// ballot is a 64-bit word built lane by lane, the lanes below are its low bits.  Built with -ffp-contract=off like the library.
// Nothing in checkm_amd loads this.
#include <cstring>
#include <string>
#include <vector>
#include "../../checkm_amd/csrc/merge_host.h"

using namespace ckm::mg;
namespace pc = ckm::pc;

namespace {

struct Bins {
  const uint64_t *bits; const int64_t *hit_sum; const int32_t *n_markers;
  std::vector<double> comp, cont;
  uint32_t nbins, nwords;
};

struct Out {
  const uint64_t *row_base; uint64_t batch_base, cap;
  uint32_t *pi, *pj; double *cols;
};

// merge_tile_kernel over one tile; returns false when a slot falls outside the batch (the kernel would drop the pair)
bool tile(bool fill, const Bins &B, const Thresholds &thr, uint32_t row_lo, uint32_t row_hi, uint32_t ti, uint32_t tj, uint32_t ntj, uint32_t count_row0,
          std::vector<uint32_t> &tile_count, const Out &out) {
  if (tj < ti) return true;
  const uint32_t i0 = ti * TILE_I, j0 = tj * TILE_J;
  bool ok = true;
  for (int wave = 0; wave < WAVES; ++wave)
    for (int r = 0; r < ROWS_PER_WAVE; ++r) {
      const uint32_t i = i0 + (uint32_t)(wave * ROWS_PER_WAVE + r);
      if (i < row_lo || i >= row_hi || i >= B.nbins) continue;
      const BinSide I = {B.hit_sum[i], B.n_markers[i], B.comp[i], B.cont[i]};
      uint64_t ballot = 0;
      PairCols pc[WAVE];
      for (int lane = 0; lane < WAVE; ++lane) {
        const uint32_t j = j0 + (uint32_t)lane;
        if (j >= B.nbins || j <= i) continue;
        int32_t u = 0;
        for (uint32_t w0 = 0; w0 < B.nwords; w0 += WORD_CHUNK)
          for (uint32_t k = w0; k < B.nwords && k < w0 + WORD_CHUNK; ++k) u += union_word(B.bits[(size_t)i * B.nwords + k], B.bits[(size_t)j * B.nwords + k]);
        const BinSide J = {B.hit_sum[j], B.n_markers[j], B.comp[j], B.cont[j]};
        if (pair_eval(u, I, J, thr, pc[lane])) ballot |= (uint64_t)1 << lane;
      }
      const uint64_t at = (uint64_t)(i - count_row0) * ntj + tj;
      if (!fill) { tile_count[at] = (uint32_t)popc64(ballot); continue; }
      for (int lane = 0; lane < WAVE; ++lane) {
        if (!(ballot >> lane & 1)) continue;
        const int below = popc64(ballot & (((uint64_t)1 << lane) - 1));
        const uint64_t slot = pair_slot(out.row_base[i - count_row0], tile_count[at], below, out.batch_base);
        if (slot >= out.cap) { ok = false; continue; }
        out.pi[slot] = i; out.pj[slot] = j0 + (uint32_t)lane;
        for (int c = 0; c < NCOL; ++c) out.cols[(uint64_t)c * out.cap + slot] = pc[lane].v[c];
      }
    }
  return ok;
}

}  // namespace

// ckm_merge_run without a device.  cap_pairs: pairs an output batch may hold (0: no limit); pass_rows: rows of a count pass (0: the
// library's).  The reported pairs are appended to oi / oj / cols ([9][max_out]); returns their number, -1 for refused arguments, -2 when
// a pair fell outside its batch or max_out.
extern "C" int64_t emu_merge(uint32_t nbins, uint32_t ngenes, const uint64_t *bits, const int64_t *hit_sum, const int32_t *n_markers, const double *thr, uint64_t cap_pairs,
                             uint32_t pass_rows, uint32_t *oi, uint32_t *oj, double *cols, uint64_t max_out, uint64_t *nbatches) {
  if (!check_args(nbins, ngenes, bits, hit_sum, n_markers, thr).empty()) return -1;
  *nbatches = 0;
  if (nbins < 2) return 0;
  Bins B = {bits, hit_sum, n_markers, std::vector<double>(nbins), std::vector<double>(nbins), nbins, words_for(ngenes)};
  for (uint32_t b = 0; b < nbins; ++b) {                                       // merge_bins_kernel
    int32_t members = 0;
    for (uint32_t k = 0; k < B.nwords; ++k) members += popc64(bits[(size_t)b * B.nwords + k]);
    bin_stats(members, hit_sum[b], n_markers[b], B.comp[b], B.cont[b]);
  }
  const Thresholds T = {thr[0], thr[1], thr[2], thr[3]};
  const uint32_t ntj = tiles_for(nbins);
  if (!pass_rows) pass_rows = count_pass_rows(nbins);
  pass_rows = (pass_rows + TILE_I - 1) / TILE_I * TILE_I;
  if (!cap_pairs) cap_pairs = ~(uint64_t)0;
  uint64_t total = 0;
  std::vector<uint32_t> tile_count((size_t)pass_rows * ntj, 0xDEADBEEFu), row_total(pass_rows);      // (poisoned: the scan must not read left of the diagonal)
  std::vector<uint64_t> row_base(pass_rows);
  std::vector<Group> groups;
  for (uint32_t r0 = 0; r0 < nbins; r0 += pass_rows) {
    const uint32_t r1 = (uint32_t)std::min<uint64_t>(nbins, (uint64_t)r0 + pass_rows), nr = r1 - r0;
    const Out none = {nullptr, 0, 0, nullptr, nullptr, nullptr};
    for (uint32_t ti = r0 / TILE_I; ti < (r1 - 1) / TILE_I + 1; ++ti)
      for (uint32_t tj = 0; tj < ntj; ++tj) tile(false, B, T, r0, r1, ti, tj, ntj, r0, tile_count, none);
    for (uint32_t k = 0; k < nr; ++k) row_total[k] = pc::row_scan_host(&tile_count[(size_t)k * ntj], 1, (r0 + k) / TILE_I, ntj);      // merge_scan_kernel
    const uint64_t run = pc::row_prefix(row_total.data(), nr, row_base.data());
    groups.clear();
    plan_groups(row_total.data(), r0, r1, cap_pairs, groups);
    uint64_t seen = 0;
    for (const Group &g : groups) {
      if (g.base != seen) return -2;
      std::vector<uint32_t> pi(g.npairs, 0xFFFFFFFFu), pj(g.npairs, 0xFFFFFFFFu);
      std::vector<double> pc((size_t)NCOL * g.npairs);
      const Out o = {row_base.data(), g.base, g.npairs, pi.data(), pj.data(), pc.data()};
      bool ok = true;
      for (uint32_t ti = g.row_lo / TILE_I; ti < (g.row_hi - 1) / TILE_I + 1; ++ti)
        for (uint32_t tj = 0; tj < ntj; ++tj) ok = tile(true, B, T, g.row_lo, g.row_hi, ti, tj, ntj, r0, tile_count, o) && ok;
      if (!ok || total + g.npairs > max_out) return -2;
      for (uint64_t k = 0; k < g.npairs; ++k) {
        if (pi[k] == 0xFFFFFFFFu) return -2;                                   // a slot nobody filled
        oi[total + k] = pi[k]; oj[total + k] = pj[k];
        for (int c = 0; c < NCOL; ++c) cols[(uint64_t)c * max_out + total + k] = pc[(size_t)c * g.npairs + k];
      }
      total += g.npairs; seen += g.npairs; *nbatches += 1;
    }
    if (seen != run) return -2;
  }
  return (int64_t)total;
}

// the lines of merger.tsv for n pairs, as ckm_merge_run appends them; returns the bytes written into buf (at most cap)
extern "C" uint64_t emu_merge_lines(const char *const *ids, const uint32_t *pi, const uint32_t *pj, const double *cols, uint64_t stride, uint64_t n, char *buf, uint64_t cap) {
  std::string s;
  format_lines(s, ids, pi, pj, cols, stride, n);
  const uint64_t m = std::min<uint64_t>(cap, s.size());
  memcpy(buf, s.data(), m);
  return s.size();
}

extern "C" int emu_merge_check(uint32_t nbins, uint32_t ngenes, const uint64_t *bits, const int64_t *hit_sum, const int32_t *n_markers, const double *thr, char *why, uint32_t cap) {
  const std::string s = check_args(nbins, ngenes, bits, hit_sum, n_markers, thr);
  if (cap) { strncpy(why, s.c_str(), cap - 1); why[cap - 1] = 0; }
  return s.empty() ? 0 : -1;
}
