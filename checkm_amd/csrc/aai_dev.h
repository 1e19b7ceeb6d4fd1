// aai_dev.h -- the per-chunk step, the pair decode and the host-side geometry of the all-pairs amino-acid identity of
// AminoAcidIdentity.run (kernels_aai.hip), written once for the device and for the host executor of the CPU tests (tests/emu/aai_emu.cpp).
//
// A group is one <bin>/<marker>.masked.faa: n rows of L bytes.  For every pair i < j of a group the reference's aai()
// (checkm/aminoAcidIdentity.py:127-161) needs: start = the first column where neither row holds '-', end = L lowered past the trailing
// columns where either does (a scan that never looks at column 0), and over [start, end) the columns whose bytes differ and the
// columns that are not '-' in both rows.  One wavefront owns a pair; every lane holds up to CHUNKS aligned 16-byte chunks of both rows
// and turns each into 16-bit masks, one bit per column, in column order.  Rows are packed at a stride of pad16(L), so a chunk that
// starts inside a row ends inside the row's own padding; the padding is kept out of every mask by the chunk's valid bits.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>
#include "ckm_internal.h"
#include "wave_const.h"
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define AAI_HD __host__ __device__ __forceinline__
#else
#define AAI_HD inline
#endif

namespace ckm {
namespace aai {

using ckm::LANE_BYTES;
using ckm::WAVE;
using ckm::WAVE_BYTES;
constexpr uint32_t MAX_L = 4096;                  // the model limit of DESIGN section 8: a masked row has one byte per match column
constexpr int CHUNKS = MAX_L / WAVE_BYTES;        // chunks of one row a lane holds
constexpr uint64_t MAX_ROWS = 1u << 20;           // rows of one group: n (n - 1) / 2 and the decode's square root stay far inside 2^53
constexpr uint32_t PAIR_BYTES = 16;               // int32 mismatches + int32 compared + double aai
constexpr uint64_t MIN_BATCH_PAIRS = 64;          // what a batch takes when the budget does not even hold the text of one group
constexpr int NO_COLUMN = 0x7fffffff;
constexpr uint32_t HI = 0x80808080u;

// 0x80 in every byte in which a and b agree (no carry crosses a byte; any byte value)
AAI_HD uint32_t bytes_equal(uint32_t a, uint32_t b) {
  const uint32_t z = a ^ b;
  return ~(((z & 0x7f7f7f7fu) + 0x7f7f7f7fu) | z | 0x7f7f7f7fu);
}
// bit 7 of bytes 0 .. 3 of m -> bits 0 .. 3: the partial products of the multiplication land on sixteen different bits, so none carries
AAI_HD uint32_t pack4(uint32_t m) { return ((((m & HI) >> 7) * 0x00204081u) >> 21) & 0xFu; }

AAI_HD int popcount32(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popc(x);
#else
  return __builtin_popcount(x);
#endif
}
AAI_HD int lowest_bit(uint32_t x) {               // x != 0
#if defined(__HIP_DEVICE_COMPILE__)
  return __ffs((int)x) - 1;
#else
  return __builtin_ctz(x);
#endif
}
AAI_HD int highest_bit(uint32_t x) {              // x != 0
#if defined(__HIP_DEVICE_COMPILE__)
  return 31 - __clz((int)x);
#else
  return 31 - __builtin_clz(x);
#endif
}

// One chunk of a pair: x and y are the 16 bytes of rows i and j at the same columns, of which the first nvalid (1 .. 16) belong to the
// rows.  Bit c of a mask is column c of the chunk; gapped, both and differ are zero outside valid.
struct Chunk { uint32_t valid, gapped, both, differ; };      // '-' in either row; '-' in both rows; the two bytes differ
AAI_HD Chunk chunk_masks(const uint32_t *x, const uint32_t *y, int nvalid) {
  Chunk o = {nvalid >= LANE_BYTES ? 0xFFFFu : nvalid <= 0 ? 0u : ((1u << nvalid) - 1u), 0, 0, 0};
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const uint32_t gx = bytes_equal(x[w], 0x2d2d2d2du), gy = bytes_equal(y[w], 0x2d2d2d2du);
    o.gapped |= pack4(gx | gy) << (4 * w);
    o.both |= pack4(gx & gy) << (4 * w);
    o.differ |= pack4(~bytes_equal(x[w], y[w])) << (4 * w);
  }
  o.gapped &= o.valid; o.both &= o.valid; o.differ &= o.valid;
  return o;
}

// What the chunk at column `off` adds to its lane's view of the row ends: the lowest column that is not gapped, and the highest such
// column other than column 0 (the reference's trailing scan runs range(L - 1, 0, -1): it stops in front of column 0).
AAI_HD void chunk_span(const Chunk &c, int off, int &first, int &last) {
  const uint32_t open = ~c.gapped & c.valid;
  if (open) { const int f = off + lowest_bit(open); first = f < first ? f : first; }
  const uint32_t tail = off == 0 ? open & ~1u : open;
  if (tail) { const int l = off + highest_bit(tail); last = l > last ? l : last; }
}

// start and end of the compared span from the minimum of `first` (NO_COLUMN: none) and the maximum of `last` (-1: none) over the pair:
// start = L when every column is gapped; end = 1 when columns 1 .. L-1 all are and L >= 1; end = 0 for L = 0.
AAI_HD void pair_span(int first, int last, int L, int &start, int &end) {
  start = first < L ? first : L;
  end = last >= 1 ? last + 1 : (L < 1 ? L : 1);
}

// the chunk's columns inside [start, end): a mismatch is a column whose bytes differ, a compared column one that is not '-' in both rows
AAI_HD void chunk_count(const Chunk &c, int off, int start, int end, int &mismatches, int &compared) {
  int lo = start - off, hi = end - off;
  lo = lo < 0 ? 0 : lo > LANE_BYTES ? LANE_BYTES : lo;
  hi = hi < 0 ? 0 : hi > LANE_BYTES ? LANE_BYTES : hi;
  if (lo >= hi) return;
  const uint32_t in = ((1u << hi) - 1u) & ~((1u << lo) - 1u) & c.valid;
  mismatches += popcount32(c.differ & in);
  compared += popcount32(~c.both & in);
}

// 1.0 - float(mismatches) / seqLen of the reference, 0.0 for seqLen == 0: one IEEE double division and one subtraction
AAI_HD double identity(int mismatches, int compared) { return compared == 0 ? 0.0 : 1.0 - (double)mismatches / (double)compared; }

AAI_HD uint64_t pad16(uint64_t n) { return (n + 15) & ~(uint64_t)15; }

// ---- flat pair index -> (group, i, j) ---------------------------------------------------------------------------------------------------

// pairs of an n-row group in front of row i's pairs: (i, i+1) .. (i, n-1) follow (i-1, n-1); i <= n - 1 <= 2^20
AAI_HD uint64_t pairs_before(uint64_t n, uint64_t i) { return i * (2 * n - i - 1) / 2; }

// the group g in [lo, hi) with pair_off[g] <= p < pair_off[g + 1]; pair_off[lo] <= p < pair_off[hi].  Groups without a pair repeat
// their neighbour's offset and are never the answer.
AAI_HD uint32_t find_group(const uint64_t *pair_off, uint32_t lo, uint32_t hi, uint64_t p) {
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (pair_off[mid] <= p) lo = mid; else hi = mid;
  }
  return lo;
}

// pair number k (0 <= k < n (n - 1) / 2) of an n-row group, i major and j minor.  The root of i^2 - (2n - 1) i + 2k = 0 in floating
// point is only a first guess: the two loops move it to the one i with pairs_before(n, i) <= k < pairs_before(n, i + 1), in integers.
AAI_HD void decode_pair(uint64_t k, uint64_t n, uint32_t &i, uint32_t &j) {
  const double b = (double)(2 * n - 1);
  double r = (b - sqrt(b * b - 8.0 * (double)k)) * 0.5;
  if (!(r >= 0.0)) r = 0.0;
  uint64_t a = (uint64_t)r;
  if (a > n - 2) a = n - 2;
  while (pairs_before(n, a) > k) --a;
  while (a + 2 < n && pairs_before(n, a + 1) <= k) ++a;
  i = (uint32_t)a;
  j = (uint32_t)(a + 1 + (k - pairs_before(n, a)));
}

// ---- host side, shared by the library, the host executor and the stand-alone check ---------------------------------------------------------

// What the kernel knows of a group: its rows lie at text + text_off + r * stride
struct Group {
  uint64_t text_off;      // first byte of row 0 in the packed text of ALL groups (a multiple of 16)
  uint32_t n, len;        // rows, bytes per row; stride = pad16(len)
};

// Whether the arguments of a call can be taken, and in `why` what is wrong with them: ARGS_INVALID is a bad argument, ARGS_RANGE a size
// limit.  group_row_off[ngroups + 1] counts rows and row_off[group_row_off[ngroups] + 1] counts bytes of `text`; both start at 0 and never
// fall.  No entry of row_off is read before group_row_off is known to be in order.
using ckm::ARGS_INVALID;
using ckm::ARGS_OK;
using ckm::ARGS_RANGE;
inline int check_args(uint32_t ngroups, const uint64_t *group_row_off, const uint64_t *row_off, const char *text, std::string &why) {
  auto no = [&](int kind, const std::string &m) { why = m; return kind; };
  if (!group_row_off || !row_off) return no(ARGS_INVALID, "NULL argument");
  if (group_row_off[0] != 0) return no(ARGS_INVALID, "group_row_off does not start at 0");
  for (uint32_t g = 0; g < ngroups; ++g)
    if (group_row_off[g + 1] < group_row_off[g]) return no(ARGS_INVALID, "group_row_off falls at group " + std::to_string(g));
  const uint64_t nrows = group_row_off[ngroups];
  if (row_off[0] != 0) return no(ARGS_INVALID, "row_off does not start at 0");
  for (uint64_t r = 0; r < nrows; ++r)
    if (row_off[r + 1] < row_off[r]) return no(ARGS_INVALID, "row_off falls at row " + std::to_string(r));
  if (row_off[nrows] && !text) return no(ARGS_INVALID, "NULL text");
  for (uint32_t g = 0; g < ngroups; ++g) {
    const uint64_t r0 = group_row_off[g], r1 = group_row_off[g + 1];
    if (r1 == r0) continue;
    const uint64_t len = row_off[r0 + 1] - row_off[r0];
    for (uint64_t r = r0 + 1; r < r1; ++r)
      if (row_off[r + 1] - row_off[r] != len) return no(ARGS_INVALID, "rows of unequal length in group " + std::to_string(g));
    if (len > MAX_L) return no(ARGS_RANGE, "rows of " + std::to_string(len) + " bytes in group " + std::to_string(g) + ": the limit is " + std::to_string(MAX_L));
    if (r1 - r0 > MAX_ROWS) return no(ARGS_RANGE, std::to_string(r1 - r0) + " rows in group " + std::to_string(g) + ": the limit is " + std::to_string(MAX_ROWS));
  }
  return ARGS_OK;
}

// The groups as the kernel sees them, pair_off[ngroups + 1], and the packed text: every row at its 16-byte stride, zeros behind it.
// Arguments that passed check_args.
struct Packed {
  std::vector<Group> groups;
  std::vector<uint64_t> pair_off;
  std::vector<uint8_t> text;
};
inline void pack(uint32_t ngroups, const uint64_t *group_row_off, const uint64_t *row_off, const char *text, Packed &P) {
  P.groups.resize(ngroups); P.pair_off.assign((size_t)ngroups + 1, 0);
  uint64_t bytes = 0;
  for (uint32_t g = 0; g < ngroups; ++g) {
    const uint64_t r0 = group_row_off[g], n = group_row_off[g + 1] - r0;
    const uint32_t len = n ? (uint32_t)(row_off[r0 + 1] - row_off[r0]) : 0;
    P.groups[g] = Group{bytes, (uint32_t)n, len};
    P.pair_off[g + 1] = P.pair_off[g] + (n ? n * (n - 1) / 2 : 0);
    if (n > 1) bytes += n * pad16(len);                          // a group without a pair sends nothing
  }
  P.text.assign(bytes, 0);
  for (uint32_t g = 0; g < ngroups; ++g) {
    const Group &G = P.groups[g];
    if (G.n < 2 || !G.len) continue;
    const uint64_t stride = pad16(G.len), r0 = group_row_off[g];
    for (uint32_t r = 0; r < G.n; ++r) memcpy(P.text.data() + G.text_off + r * stride, text + row_off[r0 + r], G.len);
  }
}
inline uint64_t group_bytes(const Group &G) { return G.n > 1 ? (uint64_t)G.n * pad16(G.len) : 0; }

// One batch: pairs [p0, p0 + npairs) of the flat order, which lie in groups [g_lo, g_hi); the text of those groups is
// [text_lo, text_lo + text_bytes) of the packed text.  A group whose pairs do not fit is cut, and its text travels with every piece.
struct Batch { uint64_t p0 = 0, npairs = 0, text_lo = 0, text_bytes = 0; uint32_t g_lo = 0, g_hi = 0; };

// Fills `b` with the next pairs from `cursor` on whose text and outputs fit budget_bytes (always at least one pair); false at the end
inline bool next_batch(const Packed &P, uint64_t budget_bytes, uint64_t &cursor, Batch &b) {
  const uint32_t ngroups = (uint32_t)P.groups.size();
  const uint64_t total = P.pair_off[ngroups];
  if (cursor >= total) return false;
  uint32_t g = find_group(P.pair_off.data(), 0, ngroups, cursor);
  b = Batch();
  b.p0 = cursor; b.g_lo = g; b.text_lo = P.groups[g].text_off;
  uint64_t bytes = 0;
  for (; g < ngroups; ++g) {
    const uint64_t left = P.pair_off[g + 1] - (cursor > P.pair_off[g] ? cursor : P.pair_off[g]);
    if (!left) continue;
    const uint64_t tb = group_bytes(P.groups[g]);
    if (b.npairs && bytes + tb + PAIR_BYTES > budget_bytes) break;
    bytes += tb;
    uint64_t take = bytes < budget_bytes ? (budget_bytes - bytes) / PAIR_BYTES : 0;
    if (!take && !b.npairs) take = MIN_BATCH_PAIRS;
    if (take > left) take = left;
    b.npairs += take; bytes += take * PAIR_BYTES; cursor += take;
    b.g_hi = g + 1; b.text_bytes = P.groups[g].text_off + tb - b.text_lo;
    if (take < left) break;
  }
  return true;
}

}  // namespace aai
}  // namespace ckm
