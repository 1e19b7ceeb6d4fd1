// pairs_dev.h -- the placement of reported pairs shared by the all-pairs passes (`checkm merge`: kernels_merge.hip; MarkerSetBuilder's
// co-location pass: kernels_markerset.hip), written once for the kernels, for the host side of the library (pairs_host.h) and for the host
// executors of the CPU tests (tests/emu/merge_emu.cpp, markerset_emu.cpp).  The reported pairs come out in (row, column) order and no atomic
// decides a position:
//
//   count   a tile kernel stores, per (row, tile column), how many pairs of the row it reports in that tile (pairs_wave.h: count_store)
//   scan    a wavefront per row turns the row's counts into offsets in place and stores the row's total (pairs_wave.h: row_scan)
//   plan    the host prefixes the row totals (row_prefix) and cuts the rows into output batches of at most `cap` pairs (plan_groups)
//   fill    the same tile kernel again, over the rows of one batch: a reported pair goes to pair_slot(...) (pairs_wave.h: lanes_below)
//
// A count pass covers rows [r0, r1) of the pass's own numbering (Merger: a stretch of the bins; MarkerSetBuilder: all rows of a round,
// r0 = 0); row_total[k] and row_base[k] belong to row r0 + k, a batch names its rows in that numbering.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PC_HD __host__ __device__ __forceinline__
#else
#define PC_HD inline
#endif

namespace ckm {
namespace pc {

// Where the fill pass puts a reported pair: row_base = pairs reported by the rows before this one, tile_off = pairs of the row in the
// tiles left of this one, below = reported pairs of this row and tile in lower lanes; minus the first pair of the output batch.
PC_HD uint64_t pair_slot(uint64_t row_base, uint32_t tile_off, int below, uint64_t batch_base) {
  return row_base + tile_off + (uint64_t)below - batch_base;
}

// After the scan a row's tile counts are offsets: what the row reports in tile column tj is the next column's offset (behind the last
// column: the row's total) minus its own.
PC_HD uint32_t tile_pairs(const uint32_t *row_offsets, uint32_t tj, uint32_t ntj, uint32_t row_total) {
  return (tj + 1 < ntj ? row_offsets[tj + 1] : row_total) - row_offsets[tj];
}

// pairs_wave.h's row_scan as a plain loop: row[k * stride] for k in [first, n) becomes the sum of those before it; returns the total
inline uint32_t row_scan_host(uint32_t *row, uint64_t stride, uint32_t first, uint32_t n) {
  uint32_t carry = 0;
  for (uint32_t k = first; k < n; ++k) { const uint32_t v = row[k * stride]; row[k * stride] = carry; carry += v; }
  return carry;
}

// pairs an output batch may hold
inline uint64_t budget_pairs(uint64_t budget_bytes, uint64_t pair_bytes) { return std::max<uint64_t>(1, budget_bytes / pair_bytes); }

// row_base[k] = pairs reported by the rows before k; returns the pairs of all rows
inline uint64_t row_prefix(const uint32_t *row_total, uint32_t nrows, uint64_t *row_base) {
  uint64_t run = 0;
  for (uint32_t k = 0; k < nrows; ++k) { row_base[k] = run; run += row_total[k]; }
  return run;
}

// An output batch: rows [row_lo, row_hi) whose reported pairs are [base, base + npairs) of the count pass they belong to.
struct Group { uint32_t row_lo, row_hi; uint64_t base, npairs; };

// Whole rows, in order, as many as fit `cap` pairs; a row that reports more than `cap` by itself is a batch of its own.  Rows without a
// reported pair never open a batch.  row_total[k] belongs to row r0 + k.
inline void plan_groups(const uint32_t *row_total, uint32_t r0, uint32_t r1, uint64_t cap, std::vector<Group> &out) {
  uint64_t base = 0;
  Group g = {r0, r0, 0, 0};
  for (uint32_t r = r0; r < r1; ++r) {
    const uint64_t n = row_total[r - r0];
    if (g.npairs && g.npairs + n > cap) { g.row_hi = r; out.push_back(g); g = Group{r, r, base, 0}; }
    if (!g.npairs) { g.row_lo = r; g.base = base; }
    g.npairs += n; base += n;
  }
  if (g.npairs) { g.row_hi = r1; out.push_back(g); }
}

}  // namespace pc
}  // namespace ckm
