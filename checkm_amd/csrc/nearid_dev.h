// nearid_dev.h -- the data layout, the arithmetic and the band cuts of the near-identity pass (what __nearlyIdentical of the reference's
// scripts/genometreeworkflow/createSmallTree.py asks of a Python loop, pair by pair), written once for the kernel (kernels_nearid.hip),
// for the host executor (run_host below, nearid_host.cpp) and for the stand-alone check.  DESIGN section 29.
//
// Text: n_rows rows of row_len raw bytes, row i at text + i * row_stride; row_stride >= row_len and a multiple of 16, so that a 64-bit
//   word of a row lies inside the row's stride or past it.  The bytes between row_len and row_stride are never compared (a word that
//   straddles row_len is masked to the row), whatever they hold.  Every byte value counts as itself: gaps, letters of either case and
//   bytes 0x80 .. 0xFF alike.
// Pair (i, j > i): diffs = the columns at which the two rows hold different bytes; the pair is near iff diffs < limit[i], limit[i] >= 1.
// Output: near [n_rows][words], words = ceil(n_rows / 64): bit (j & 63) of word j / 64 of row i is set iff j > i and the pair is near.
//   Every word of the matrix is written, the words below the diagonal as 0.
// Arithmetic: integers only.  Eight columns per 64-bit operation: x = a ^ b, the low seven bits of every byte carried into its top bit,
//   the top bit itself or-ed in, one population count of the eight top bits (diff_bits).  No byte carries into its neighbour:
//   (x & 0x7f) + 0x7f <= 0xfe.
// Bands: the call is cut into bands of row tiles (64 rows each); the text and the limits stay resident, a band adds its bit rows.  No
//   result depends on the cut.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include "ckm_internal.h"
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define NI_HD __host__ __device__ __forceinline__
#else
#define NI_HD inline
#endif

namespace ckm {
namespace nearid {

constexpr uint32_t TILE = 64;                       // rows of a tile: one output word per (row, column tile)
constexpr uint32_t CHUNK = 128;                     // columns staged at a time
constexpr uint32_t MAX_ROWS = 1u << 17;             // the bit matrix stays at or below 2 GiB
constexpr uint32_t MAX_STRIDE = 1u << 24;           // a count of differing columns fits 32 bits with room to spare
constexpr uint64_t MAX_TEXT_BYTES = 1ull << 34;     // n_rows * row_stride
using ckm::ARGS_INVALID;
using ckm::ARGS_OK;
using ckm::ARGS_RANGE;

struct Args { const uint8_t *text; uint32_t n_rows, row_len, row_stride; const uint32_t *limit; };

NI_HD uint32_t words_of(uint32_t n_rows) { return (n_rows + 63) / 64; }
NI_HD uint32_t tiles_of(uint32_t n_rows) { return (n_rows + TILE - 1) / TILE; }

// the bytes of the word at column col that belong to the row: all eight, or the low row_len - col of them (little endian: the low bytes
// are the first columns); col < row_len
NI_HD uint64_t word_mask(uint32_t col, uint32_t row_len) {
  const uint32_t left = row_len - col;
  return left >= 8 ? ~0ull : (1ull << (8 * left)) - 1;
}
// one bit per byte of x that is not zero, at the byte's top bit
NI_HD uint64_t diff_bits(uint64_t x) {
  const uint64_t low = 0x7f7f7f7f7f7f7f7full;
  return (((x & low) + low) | x) & ~low;
}
NI_HD uint32_t pop64(uint64_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__popcll(x);
#else
  return (uint32_t)__builtin_popcountll(x);
#endif
}

// bytes resident whatever the band, and bytes a row tile adds to a band
inline uint64_t fixed_bytes(const Args &a) { return (uint64_t)a.n_rows * a.row_stride + (uint64_t)a.n_rows * 4; }
inline uint64_t tile_bytes(const Args &a) { return (uint64_t)TILE * words_of(a.n_rows) * 8; }
// the band that begins at row tile b0: row tiles b0 .. the returned one; at least one, then as many as the budget leaves room for
inline uint32_t band_end(const Args &a, uint32_t b0, uint64_t budget) {
  const uint64_t fixed = fixed_bytes(a), per = tile_bytes(a);
  uint64_t n = budget > fixed ? (budget - fixed) / per : 0;
  if (n < 1) n = 1;
  const uint32_t nt = tiles_of(a.n_rows);
  return n >= nt - b0 ? nt : b0 + (uint32_t)n;
}

// Why a call would be refused.
inline int check(const Args &a, std::string &why) {
  auto bad = [&](int kind, const std::string &w) { why = w; return kind; };
  if (!a.text || !a.limit) return bad(ARGS_INVALID, "NULL argument");
  if (a.n_rows == 0) return bad(ARGS_INVALID, "no rows");
  if (a.row_len == 0) return bad(ARGS_INVALID, "rows without a column");
  if (a.row_stride < a.row_len) return bad(ARGS_INVALID, "a row stride below the row length");
  if (a.row_stride % 16) return bad(ARGS_INVALID, "a row stride that is not a multiple of 16");
  if (a.n_rows > MAX_ROWS) return bad(ARGS_RANGE, "more than 2^17 rows");
  if (a.row_stride > MAX_STRIDE) return bad(ARGS_RANGE, "a row stride above 2^24");
  if ((uint64_t)a.n_rows * a.row_stride > MAX_TEXT_BYTES) return bad(ARGS_RANGE, "more than 2^34 bytes of text");
  for (uint32_t i = 0; i < a.n_rows; ++i)
    if (a.limit[i] == 0) return bad(ARGS_INVALID, "row " + std::to_string(i) + " has the limit 0");
  return ARGS_OK;
}

// diffs of two rows, or some value >= limit once the count has reached it (the answer is a bit: stopping early is exact)
inline uint32_t diffs_upto(const uint8_t *ra, const uint8_t *rb, uint32_t row_len, uint32_t limit) {
  uint32_t d = 0;
  for (uint32_t col = 0; col < row_len && d < limit; col += 8) {
    uint64_t x, y;
    memcpy(&x, ra + col, 8);
    memcpy(&y, rb + col, 8);
    d += pop64(diff_bits((x ^ y) & word_mask(col, row_len)));
  }
  return d;
}

// The host executor: the same bands, the same word arithmetic, loops where the device has lanes.  counts: bands, pairs.
inline int run_host(const Args &a, uint64_t budget, uint64_t *near, uint64_t counts[2], std::string &why) {
  const int kind = check(a, why);
  if (kind != ARGS_OK) return kind;
  if (!near) { why = "NULL argument"; return ARGS_INVALID; }
  const uint32_t N = a.n_rows, W = words_of(N), nt = tiles_of(N);
  counts[0] = 0; counts[1] = (uint64_t)N * (N - 1) / 2;
  for (uint32_t b0 = 0; b0 < nt;) {
    const uint32_t b1 = band_end(a, b0, budget);
    const uint32_t i1 = (uint64_t)b1 * TILE < N ? b1 * TILE : N;
    for (uint32_t i = b0 * TILE; i < i1; ++i) {
      uint64_t *row = near + (uint64_t)i * W;
      for (uint32_t w = 0; w < W; ++w) row[w] = 0;
      const uint8_t *ra = a.text + (uint64_t)i * a.row_stride;
      for (uint32_t j = i + 1; j < N; ++j)
        if (diffs_upto(ra, a.text + (uint64_t)j * a.row_stride, a.row_len, a.limit[i]) < a.limit[i]) row[j >> 6] |= 1ull << (j & 63);
    }
    counts[0] += 1;
    b0 = b1;
  }
  return ARGS_OK;
}

}  // namespace nearid
}  // namespace ckm
