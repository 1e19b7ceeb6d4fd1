// coverage_dev.h -- what `checkm coverage` does with one BAM record (checkm/coverage.py:206-230), written once for the kernel
// (kernels_coverage.hip) and for the host executor of the CPU tests (tests/emu/coverage_emu.cpp).
//
// A record starts at its block_size field; the host reader (bam_host.cpp) has checked that the record lies inside the batch, that its
// fixed part, read name, CIGAR, bases and qualities fit into block_size and that refID is -1 or a reference.  Records start at any
// byte (read names have any length), so every field is assembled from bytes.  The auxiliary fields are walked here, with bounds.
//
// The chain, in the reference's order; the class is the counter the read adds to:
//   0 unmapped (0x4)   1 duplicate (0x400)   2 secondary or supplementary (0x100, 0x800)   3 QC-fail (0x200) or mapq < minQC
//   4 query_alignment_length < minAlignPer * query_length          5 NM > maxEditDistPer * query_length
//   6 not a proper pair (0x2), unless all reads are asked for      7 mapped: the read adds query_alignment_length to the numerator
// Both products are ONE float64 multiplication compared with an exactly converted integer (Python compares an int with a float by
// value; every integer here is below 2^53).  NM is looked for only when the chain reaches class 5.
// query_length = l_seq; query_alignment_length = l_seq minus the leading and trailing soft clips (hard clips outside them skipped; the
// walk from the end stops before the first operation), or the sum of the M, I, = and X lengths when l_seq == 0.
#pragma once
#include <cstdint>
#include "wave_const.h"

#if defined(__HIP__)
#include <hip/hip_runtime.h>
#define CV_HD __host__ __device__ __forceinline__
#else
#define CV_HD inline
#endif

namespace ckm {
namespace cv {

using ckm::WAVE;
constexpr int NCLASS = 8;
constexpr int NSLOT = 9;                 // per reference: reads, classes 1..7, numerator
constexpr int SLOT_READS = 0, SLOT_NUMER = 8;
constexpr int FIXED = 36;                // block_size + the 32 fixed bytes
// reasons of the error slot (slot value = record ordinal * 8 + reason; the smallest wins)
constexpr uint32_t ERR_AUX_RANGE = 1, ERR_NM_ABSENT = 2, ERR_NM_TYPE = 3, ERR_AUX_TYPE = 4;
constexpr uint64_t NO_ERROR = ~(uint64_t)0;

struct Params { double min_align_per, max_edit_dist_per, min_qc; int32_t all_reads, n_ref; };
struct RecOut { int32_t ref, cls; int64_t alen; uint32_t err; };

CV_HD uint32_t ld16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
CV_HD uint32_t ld32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

CV_HD int aux_size(uint8_t t) {
  switch (t) {
    case 'A': case 'c': case 'C': return 1;
    case 's': case 'S': return 2;
    case 'i': case 'I': case 'f': return 4;
    default: return 0;
  }
}

// the first NM field of [p, end): 0 and *nm, or a reason
CV_HD uint32_t find_nm(const uint8_t *rec, uint64_t p, uint64_t end, int64_t *nm) {
  while (p < end) {
    if (p + 3 > end) return ERR_AUX_RANGE;
    const uint8_t t0 = rec[p], t1 = rec[p + 1], ty = rec[p + 2];
    p += 3;
    const int sz = aux_size(ty);
    if (sz) {
      if (p + (uint64_t)sz > end) return ERR_AUX_RANGE;
      if (t0 == 'N' && t1 == 'M') {
        switch (ty) {
          case 'c': *nm = (int8_t)rec[p]; return 0;
          case 'C': *nm = rec[p]; return 0;
          case 's': *nm = (int16_t)ld16(rec + p); return 0;
          case 'S': *nm = ld16(rec + p); return 0;
          case 'i': *nm = (int32_t)ld32(rec + p); return 0;
          case 'I': *nm = ld32(rec + p); return 0;
          default: return ERR_NM_TYPE;
        }
      }
      p += (uint64_t)sz;
    } else if (ty == 'Z' || ty == 'H') {
      if (t0 == 'N' && t1 == 'M') return ERR_NM_TYPE;
      while (p < end && rec[p]) ++p;
      if (p >= end) return ERR_AUX_RANGE;
      ++p;
    } else if (ty == 'B') {
      if (t0 == 'N' && t1 == 'M') return ERR_NM_TYPE;
      if (p + 5 > end) return ERR_AUX_RANGE;
      const int es = aux_size(rec[p]);
      if (!es || rec[p] == 'A') return ERR_AUX_TYPE;
      const uint64_t bytes = (uint64_t)ld32(rec + p + 1) * (uint64_t)es;
      p += 5;
      if (bytes > end - p) return ERR_AUX_RANGE;
      p += bytes;
    } else {
      return ERR_AUX_TYPE;
    }
  }
  return ERR_NM_ABSENT;
}

CV_HD void classify(const uint8_t *rec, const Params &P, RecOut &o) {
  const uint64_t end = 4 + (uint64_t)ld32(rec);
  o.ref = (int32_t)ld32(rec + 4);
  const uint32_t l_name = rec[12], mapq = rec[13], n_cigar = ld16(rec + 16), flag = ld16(rec + 18);
  const int64_t l_seq = (int32_t)ld32(rec + 20);
  o.err = 0; o.alen = 0;
  if (flag & 0x4) { o.cls = 0; return; }
  if (flag & 0x400) { o.cls = 1; return; }
  if (flag & 0x900) { o.cls = 2; return; }
  if ((flag & 0x200) || (double)mapq < P.min_qc) { o.cls = 3; return; }
  const uint8_t *cig = rec + FIXED + l_name;
  int64_t alen = 0;
  if (l_seq == 0) {
    for (uint32_t k = 0; k < n_cigar; ++k) {
      const uint32_t v = ld32(cig + 4 * k), op = v & 15;
      if (op == 0 || op == 1 || op == 7 || op == 8) alen += v >> 4;
    }
  } else {
    int64_t lead = 0, trail = 0;
    for (uint32_t k = 0; k < n_cigar; ++k) {
      const uint32_t v = ld32(cig + 4 * k), op = v & 15;
      if (op == 4) lead += v >> 4; else if (op != 5) break;
    }
    for (uint32_t k = n_cigar; k > 1; --k) {
      const uint32_t v = ld32(cig + 4 * (k - 1)), op = v & 15;
      if (op == 4) trail += v >> 4; else if (op != 5) break;
    }
    alen = l_seq - lead - trail;
  }
  o.alen = alen;
  const double ql = (double)l_seq;
  if ((double)alen < P.min_align_per * ql) { o.cls = 4; return; }
  int64_t nm = 0;
  const uint64_t aux = (uint64_t)FIXED + l_name + 4ull * n_cigar + (uint64_t)((l_seq + 1) / 2) + (uint64_t)l_seq;
  const uint32_t why = aux <= end ? find_nm(rec, aux, end, &nm) : ERR_AUX_RANGE;
  if (why) { o.err = why; o.cls = -1; return; }
  if ((double)nm > P.max_edit_dist_per * ql) { o.cls = 5; return; }
  if (!P.all_reads && !(flag & 0x2)) { o.cls = 6; return; }
  o.cls = 7;
}

}  // namespace cv
}  // namespace ckm
