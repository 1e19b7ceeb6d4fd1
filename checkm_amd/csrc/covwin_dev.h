// covwin_dev.h -- what `checkm gc_bias_plot` does with one BAM record (checkm/coverageWindows.py:55-79), written once for the kernels
// (kernels_covwin.hip) and for the host executor of the CPU tests (tests/emu/covwin_emu.cpp).  The record layout, ld16 / ld32 and the
// auxiliary walk (find_nm) are coverage_dev.h's; classify, Params and RecOut of that header are not touched.
//
// The chain of CoverageWindows is NOT the chain of Coverage; the class is the counter the read adds to:
//   0 unmapped (0x4)   1 duplicate (0x400)   2 secondary (0x100 only: a supplementary read goes on)   3 QC-fail (0x200 only: no mapq test)
//   4 alen < minAlignPer * rlen                5 NM > maxEditDistPer * rlen
//   6 not a proper pair (0x2), unless all reads are asked for      7 mapped: the read adds 1 to the depth of [pos, pos + alen)
// rlen = l_seq; alen = the reference span of the CIGAR = the sum of the M, D, N, = and X lengths, undefined without a CIGAR (the reference
// fails there with a TypeError: ERR_NO_CIGAR).  Both products are ONE float64 multiplication compared with an exactly converted integer.
// NM is looked for only when the chain reaches class 5.  A mapped read with pos < 0 is refused (ERR_NEG_POS): numpy would wrap the slice.
//
// Depth and windows.  numpy clips the slice: a mapped read covers [s, e) = [pos, min(pos + alen, L)), nothing when pos >= L or alen == 0.
// Window k is [k w, (k + 1) w); a reference of length L > 0 has (L - 1) / w + 1 slots: its reported windows and the tail.  scatter()
// turns one clipped read into at most four adds, whatever alen / w is: the bases in its first and last window go to `direct`, the
// whole windows between them are +w at diff[k0 + 1] and -w at diff[k1]; sum[k] = direct[k] + inclusive_prefix(diff)[k].  e <= L keeps
// k1 inside the reference's slots, so every reference's diff nets to zero and ONE scan over all slots needs no segment flags.
#pragma once
#include "coverage_dev.h"

namespace ckm {
namespace cw {

using cv::FIXED;
using cv::NCLASS;
using cv::NO_ERROR;
using cv::NSLOT;
using cv::SLOT_NUMER;
using cv::SLOT_READS;
using cv::WAVE;
using cv::ld16;
using cv::ld32;

// further reasons of the error slot (slot value = record ordinal * 8 + reason), after cv::ERR_AUX_TYPE = 4
constexpr uint32_t ERR_NO_CIGAR = 5, ERR_NEG_POS = 6;
constexpr int SCAN_THREADS = 256, SCAN_ITEMS = 4, SCAN_BLOCK = SCAN_THREADS * SCAN_ITEMS;      // slots per workgroup of the scan
constexpr uint32_t NO_SLOT = 0xffffffffu;
constexpr int64_t MAX_SLOTS = 0x7fffffff, MAX_WINDOW = 0x7fffffff;

struct Params { double min_align_per, max_edit_dist_per; int32_t all_reads, n_ref; uint32_t window; };
struct RecOut { int32_t ref, cls; int64_t pos, alen; uint32_t err; };

CV_HD void classify(const uint8_t *rec, const Params &P, RecOut &o) {
  const uint64_t end = 4 + (uint64_t)ld32(rec);
  o.ref = (int32_t)ld32(rec + 4);
  o.pos = (int32_t)ld32(rec + 8);
  const uint32_t l_name = rec[12], n_cigar = ld16(rec + 16), flag = ld16(rec + 18);
  const int64_t l_seq = (int32_t)ld32(rec + 20);
  o.err = 0; o.alen = 0;
  if (flag & 0x4) { o.cls = 0; return; }
  if (flag & 0x400) { o.cls = 1; return; }
  if (flag & 0x100) { o.cls = 2; return; }
  if (flag & 0x200) { o.cls = 3; return; }
  if (n_cigar == 0) { o.err = ERR_NO_CIGAR; o.cls = -1; return; }
  const uint8_t *cig = rec + FIXED + l_name;
  int64_t alen = 0;
  for (uint32_t k = 0; k < n_cigar; ++k) {
    const uint32_t v = ld32(cig + 4 * k), op = v & 15;
    if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) alen += v >> 4;
  }
  o.alen = alen;
  const double ql = (double)l_seq;
  if ((double)alen < P.min_align_per * ql) { o.cls = 4; return; }
  int64_t nm = 0;
  const uint64_t aux = (uint64_t)FIXED + l_name + 4ull * n_cigar + (uint64_t)((l_seq + 1) / 2) + (uint64_t)l_seq;
  const uint32_t why = aux <= end ? cv::find_nm(rec, aux, end, &nm) : cv::ERR_AUX_RANGE;
  if (why) { o.err = why; o.cls = -1; return; }
  if ((double)nm > P.max_edit_dist_per * ql) { o.cls = 5; return; }
  if (!P.all_reads && !(flag & 0x2)) { o.cls = 6; return; }
  if (o.pos < 0) { o.err = ERR_NEG_POS; o.cls = -1; return; }
  o.cls = 7;
}

// slots of a reference of length L with windows of w bases: the reported windows and the tail
CV_HD int64_t slots_of(int64_t L, int64_t w) { return L > 0 ? (L - 1) / w + 1 : 0; }

// What a mapped read adds.  span = bases covered (the numerator); k0 / k1 = its first and last window; head goes to direct[k0];
// when k1 > k0, tail goes to direct[k1]; when k1 > k0 + 1, +w goes to diff[k0 + 1] and -w to diff[k1].  span == 0: nothing.
struct Scatter { uint32_t span, k0, k1, head, tail; };

CV_HD Scatter scatter(int64_t pos, int64_t alen, int64_t L, uint32_t w) {
  Scatter sc = {0, 0, 0, 0, 0};
  if (pos >= L || alen <= 0) return sc;
  const int64_t e64 = pos + alen < L ? pos + alen : L;
  const uint32_t s = (uint32_t)pos, e = (uint32_t)e64;                  // 0 <= s < e <= L < 2^31
  sc.span = e - s;
  sc.k0 = s / w; sc.k1 = (e - 1) / w;
  if (sc.k0 == sc.k1) { sc.head = e - s; return sc; }
  sc.head = (sc.k0 + 1) * w - s;                                        // (k0 + 1) w <= k1 w < e: no overflow
  sc.tail = e - sc.k1 * w;
  return sc;
}

}  // namespace cw
}  // namespace ckm
