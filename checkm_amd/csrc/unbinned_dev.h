// unbinned_dev.h -- the per-word step of the selective base count of `checkm unbinned` (kernels_unbinned.hip), written once for the device
// and for the host executor of the CPU tests (tests/emu/unbinned_emu.cpp), plus the host-side geometry both share: tiles and batches.
//
// Unbinned.run (checkm/unbinned.py:33-85) needs of every contig it keeps baseCount (A, C, G, T+U after upper-casing,
// checkm/util/seqUtils.py:279-286) and len(seq) in code points; of a contig it skips it needs nothing.  Only the tiles of the kept
// sequences are listed, and only their bytes travel to the device: a batch is the 16-byte-padded text of its tiles packed back to back, so
// the bytes of a skipped neighbour are never in a buffer the kernel reads.  One wavefront owns a tile and walks it 1 KiB per step, every
// lane one aligned 16-byte chunk: four 32-bit words whose bytes are compared word-parallel.  No byte looks at a neighbour: no halo.
#pragma once
#include <cstdint>
#include <vector>
#include "wave_const.h"
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define UB_HD __host__ __device__ __forceinline__
#else
#define UB_HD inline
#endif

namespace ckm {
namespace ub {

using ckm::LANE_BYTES;
using ckm::WAVE;
using ckm::WAVE_BYTES;
constexpr int NCOUNT = 5;                         // A, C, G, T+U, code points
constexpr uint32_t DEFAULT_TILE = 4096, MAX_TILE = 1u << 20;
constexpr uint32_t HI = 0x80808080u;

struct Tile {
  uint64_t start;       // first byte of the tile in the batch buffer (a multiple of 16)
  uint32_t len;         // its bytes; what follows up to the next multiple of 16 is zero padding
  uint32_t pad;
};

// 0x80 in every byte of w that equals the byte repeated in letter4 (the test of kernels_orf.hip: no carry crosses a byte)
UB_HD uint32_t bytes_equal(uint32_t w, uint32_t letter4) {
  const uint32_t z = w ^ letter4;
  return ~(((z & 0x7f7f7f7fu) + 0x7f7f7f7fu) | z | 0x7f7f7f7fu);
}

// 0x80 in each of the first n bytes (little endian) of a word, n clamped to 0 .. 4
UB_HD uint32_t first_bytes(int n) { return n >= 4 ? HI : n <= 0 ? 0u : (HI & ((1u << (8 * n)) - 1u)); }

// The five masks of one word, 0x80 per byte: A, C, G, T or U (either case), and the bytes that start a code point (outside 0x80-0xBF).
// `& 0xDF` folds the case: only b and b ^ 0x20 map to a letter, and a byte >= 0x80 keeps its top bit and equals none.
struct WordMasks { uint32_t m[NCOUNT]; };
UB_HD WordMasks word_masks(uint32_t w) {
  const uint32_t u = w & 0xDFDFDFDFu;
  WordMasks o;
  o.m[0] = bytes_equal(u, 0x41414141u);
  o.m[1] = bytes_equal(u, 0x43434343u);
  o.m[2] = bytes_equal(u, 0x47474747u);
  o.m[3] = bytes_equal(u & 0xFEFEFEFEu, 0x54545454u);          // 'T' and 'U' differ in bit 0 only
  o.m[4] = ~bytes_equal(w & 0xC0C0C0C0u, HI) & HI;
  return o;
}

UB_HD uint32_t popcount32(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__popc(x);
#else
  return (uint32_t)__builtin_popcount(x);
#endif
}

// One lane's chunk: w[0 .. 3] are its 16 bytes, of which the first nvalid (1 .. 16) belong to the tile.  The masks of the four words
// fall on different bits of one word (bit 7 of every byte moved to bits 0 .. 3), so each counter costs one population count.
UB_HD void lane_counts(const uint32_t *w, int nvalid, uint32_t *acc /* [NCOUNT] += */) {
  uint32_t sum[NCOUNT] = {0, 0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const WordMasks o = word_masks(w[j]);
    const uint32_t valid = first_bytes(nvalid - 4 * j);
#pragma unroll
    for (int k = 0; k < NCOUNT; ++k) sum[k] |= (o.m[k] & valid) >> (7 - j);
  }
#pragma unroll
  for (int k = 0; k < NCOUNT; ++k) acc[k] += popcount32(sum[k]);
}

// host side, shared by the library and the host executor --------------------------------------------------------------------------------

inline uint64_t pad16(uint64_t n) { return (n + 15) & ~(uint64_t)15; }

struct HostTile { uint64_t src; uint32_t len; };                // src: first byte in the reader's text

// The tiles of the kept sequences in order, and first_tile[k] .. first_tile[k + 1] = the tiles of kept sequence number k (an empty
// sequence has none).  tile_bytes: a multiple of 16.
inline void make_tiles(const uint64_t *seq_off, const uint64_t *seq_bytes, const uint8_t *keep, uint32_t nseq, uint32_t tile_bytes, std::vector<HostTile> &tiles,
                       std::vector<uint64_t> &first_tile, std::vector<uint32_t> &kept) {
  tiles.clear(); first_tile.assign(1, 0); kept.clear();
  for (uint32_t s = 0; s < nseq; ++s) {
    if (!keep[s]) continue;
    for (uint64_t o = 0; o < seq_bytes[s]; o += tile_bytes)
      tiles.push_back(HostTile{seq_off[s] + o, (uint32_t)(seq_bytes[s] - o < tile_bytes ? seq_bytes[s] - o : tile_bytes)});
    first_tile.push_back(tiles.size()); kept.push_back(s);
  }
}

// one batch: tiles [t0, t0 + tiles.size()) of the list, their text packed into `bytes` bytes by the copies of `spans`
struct Span { uint64_t src, dst, bytes; };
struct Batch {
  std::vector<Tile> tiles;
  std::vector<Span> spans;                        // runs that are contiguous in the reader's text (adjacent tiles, adjacent kept sequences) are one span
  uint64_t t0 = 0, bytes = 0;
};

// Fills `b` with the next tiles whose padded text fits budget_bytes (at least one tile); false when none is left
inline bool next_batch(const std::vector<HostTile> &all, uint64_t budget_bytes, uint64_t &cursor, Batch &b) {
  b.tiles.clear(); b.spans.clear(); b.t0 = cursor; b.bytes = 0;
  while (cursor < all.size()) {
    const HostTile &h = all[cursor];
    const uint64_t n = pad16(h.len);
    if (!b.tiles.empty() && b.bytes + n > budget_bytes) break;
    if (!b.spans.empty() && b.spans.back().src + b.spans.back().bytes == h.src) b.spans.back().bytes += n;
    else b.spans.push_back(Span{h.src, b.bytes, n});
    b.tiles.push_back(Tile{b.bytes, h.len, 0});
    b.bytes += n; ++cursor;
  }
  return !b.tiles.empty();
}

// a sequence's tile rows summed: what unbinned_sum_kernel does for one kept sequence
UB_HD void sum_rows(const uint32_t *rows, uint64_t first, uint64_t last, uint64_t *out /* [NCOUNT] */) {
  uint64_t t[NCOUNT] = {0, 0, 0, 0, 0};
  for (uint64_t r = first; r < last; ++r)
    for (int k = 0; k < NCOUNT; ++k) t[k] += rows[r * NCOUNT + k];
  for (int k = 0; k < NCOUNT; ++k) out[k] = t[k];
}

}  // namespace ub
}  // namespace ckm
