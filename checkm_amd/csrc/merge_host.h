// merge_host.h -- the host side of `checkm merge` that needs no device: argument checks, the rows of a count pass and the lines of
// merger.tsv (checkm/merger.py:101-106); the split of a pass's rows into output batches is pairs_dev.h's.  Plain C++, used by ckm_merge.hip,
// by the host executor of the CPU tests (tests/emu/merge_emu.cpp) and by the sanitizer harness (tests/native/merge_host_check.cpp).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>
#include "merge_dev.h"

namespace ckm {
namespace mg {

constexpr uint64_t PAIR_BYTES = 2 * sizeof(uint32_t) + NCOL * sizeof(double);      // a reported pair on the device and in the download
constexpr uint64_t COUNT_BYTES = (uint64_t)64 << 20;                                // most the per-(row, tile) counts of one count pass take
constexpr int64_t HIT_SUM_MAX = (int64_t)1 << 40;                                   // 100 * (S_I + S_J) stays exact in float64 far beyond this

inline uint32_t words_for(uint32_t ngenes) { return (ngenes + 63u) / 64u; }
inline uint32_t tiles_for(uint32_t nbins) { return (nbins + (uint32_t)TILE_J - 1) / (uint32_t)TILE_J; }

// "" when the arguments can be computed, else why not
inline std::string check_args(uint32_t nbins, uint32_t ngenes, const uint64_t *bits, const int64_t *hit_sum, const int32_t *n_markers, const double *thr) {
  if (!thr) return "NULL argument";
  if (nbins && (!bits || !hit_sum || !n_markers)) return "NULL argument";
  if (ngenes == 0) return "no marker genes";
  if (nbins > (1u << 24)) return "more than 2^24 bins";
  const uint32_t nwords = words_for(ngenes);
  const uint64_t tail = (ngenes & 63u) ? ~(uint64_t)0 << (ngenes & 63u) : 0;
  for (uint32_t b = 0; b < nbins; ++b) {
    if (n_markers[b] <= 0) return "bin " + std::to_string(b) + ": n_markers must be positive";
    if (hit_sum[b] < 0 || hit_sum[b] > HIT_SUM_MAX) return "bin " + std::to_string(b) + ": hit_sum out of range";
    if (bits[(size_t)b * nwords + nwords - 1] & tail) return "bin " + std::to_string(b) + ": a member bit at or beyond the gene count";
  }
  return std::string();
}

// pairs an output batch may hold; its rows are pairs_dev.h's Group and plan_groups
inline uint64_t budget_pairs(uint64_t budget_bytes) { return pc::budget_pairs(budget_bytes, PAIR_BYTES); }
using pc::Group;
using pc::plan_groups;

// rows of one count pass: whole tiles, the counts within COUNT_BYTES
inline uint32_t count_pass_rows(uint32_t nbins) {
  const uint64_t per_row = (uint64_t)tiles_for(nbins) * sizeof(uint32_t);
  const uint64_t rows = std::max<uint64_t>(TILE_I, COUNT_BYTES / std::max<uint64_t>(1, per_row) / TILE_I * TILE_I);
  return (uint32_t)std::min<uint64_t>(rows, (uint64_t)tiles_for(nbins) * TILE_I);
}

// '%s\t%s' + 9 x '\t%.2f' + '\n' for n pairs; cols[c * stride + k] is column c of pair k.  glibc's %.2f rounds the exact binary value
// to nearest even as CPython's does.
inline void format_lines(std::string &buf, const char *const *ids, const uint32_t *pi, const uint32_t *pj, const double *cols, uint64_t stride, uint64_t n) {
  char num[512];
  for (uint64_t k = 0; k < n; ++k) {
    buf += ids[pi[k]]; buf += '\t'; buf += ids[pj[k]];
    for (int c = 0; c < NCOL; ++c) {
      const int len = snprintf(num, sizeof num, "\t%.2f", cols[(uint64_t)c * stride + k]);
      buf.append(num, (size_t)std::min<int>(std::max(len, 0), (int)sizeof num - 1));
    }
    buf += '\n';
  }
}

}  // namespace mg
}  // namespace ckm
