// refdist_dev.h -- the geometry of the reference-distribution pass (kernels_refdist.hip), written once for the device and for the host
// executor of the CPU tests (tests/emu/refdist_emu.cpp), plus the host code both share: the scaffold join and the argument checks.
//
// CheckM's reference tables (gc_dist, cd_dist, td_dist) come from windows drawn at random positions of a genome joined into one
// scaffold: a window [s, s + w) starts at any byte and windows overlap.  The scaffold is cut into blocks of `block`
// positions and every block counts what STARTS in it: the bases of the two GC classes, or the canonical 4-mers (their last three bytes
// may lie in the next block).  An exclusive scan over the blocks gives prefix rows P[b] = the counts of blocks 0 .. b - 1, so the count
// of any range of starts [a, e) is P[b1] - P[b0] over the whole blocks inside it plus at most two edges of fewer than `block` bytes each,
// read directly.  For GC and CD the range of starts is the window; for TD it is [s, s + w - 3): a 4-mer counts iff its four bytes lie in
// the window.  A block and an edge are both a sw::Piece: the per-lane step is sw::lane_step (seqwin_dev.h), the load shape §17's.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>
#include "seqwin_dev.h"

namespace ckm {
namespace rd {

enum { STAT_GC = 0, STAT_CD = 1, STAT_TD = 2 };
constexpr uint32_t MIN_BLOCK = 16, DEFAULT_BLOCK = 256, MAX_BLOCK = 1u << 20;
constexpr uint32_t MAX_SEP = 1024;
constexpr uint64_t MAX_SCAFFOLD = 0x7FFFFFFEull;          // the prefix rows are uint32: a scaffold of 2^31 - 1 characters or more is refused
constexpr uint64_t MAX_WINDOWS = 0x7FFFFFFFull;
using ckm::NKMER;
constexpr int NTOTALS = 2 + NKMER;                         // gc, at, the 136 canonical columns
constexpr uint32_t TD_ROW_BYTES = NKMER * 4;

NS_HD uint32_t ncol_of(int stat) { return stat == STAT_TD ? (uint32_t)NKMER : 2u; }

// block b of a scaffold of L bytes as a piece: its bytes, and as halo what the scaffold holds behind it (at most 3)
NS_HD sw::Piece block_piece(uint64_t b, uint32_t block, uint64_t L) {
  const uint64_t a = b * block, z = a + block < L ? a + block : L, room = L - z;
  return sw::Piece{a, (uint32_t)(z - a), 0u, 0u, (uint32_t)(room < (uint64_t)sw::HALO ? room : (uint64_t)sw::HALO)};
}

// What a window is made of: prefix rows b0 < b1 (none when whole == false) and up to two edges.  An edge of a TD window carries a halo
// of three bytes: every start of the range lies at least three bytes in front of the window's end.
struct WindowGeom {
  bool whole;
  uint64_t b0, b1;
  sw::Piece edge[2];                                       // len == 0: no such edge
};
NS_HD WindowGeom window_geom(uint64_t s, uint64_t w, int stat, uint32_t block) {
  WindowGeom g;
  const bool td = stat == STAT_TD;
  const uint64_t e = td ? (w >= 4 ? s + w - 3 : s) : s + w;  // the starts are [s, e)
  const uint32_t halo = td ? 3u : 0u;
  g.b0 = (s + block - 1) / block; g.b1 = e / block;
  g.whole = g.b1 > g.b0;
  if (g.whole) {
    g.edge[0] = sw::Piece{s, (uint32_t)(g.b0 * block - s), 0u, 0u, halo};
    g.edge[1] = sw::Piece{g.b1 * block, (uint32_t)(e - g.b1 * block), 0u, 0u, halo};
  } else {
    g.edge[0] = sw::Piece{s, (uint32_t)(e - s), 0u, 0u, halo};
    g.edge[1] = sw::Piece{s, 0u, 0u, 0u, 0u};
  }
  return g;
}

// host side, shared by the library and the host executor --------------------------------------------------------------------------------

inline uint64_t scaffold_len(const uint64_t *seq_bytes, uint32_t nseq, uint32_t sep_len) {
  uint64_t n = 0;
  for (uint32_t s = 0; s < nseq; ++s) n += seq_bytes[s];
  return n + (nseq ? (uint64_t)(nseq - 1) * sep_len : 0);
}

// The sequences of a batch joined in file order with sep_len 'N' between them, as the upload buffer: the scaffold at offset 0, zeros
// up to a multiple of 16, 64 bytes of slack (an aligned word that holds a byte of a piece or its halo lies inside).  The case of the
// text is kept: every class below is taken after upper-casing.
inline void join_scaffold(const char *text, const uint64_t *seq_off, const uint64_t *seq_bytes, uint32_t nseq, uint32_t sep_len, std::vector<uint8_t> &out) {
  const uint64_t L = scaffold_len(seq_bytes, nseq, sep_len);
  out.assign((size_t)(((L + 15) & ~(uint64_t)15) + 64), 0);
  uint64_t pos = 0;
  for (uint32_t s = 0; s < nseq; ++s) {
    if (s) { memset(out.data() + pos, 'N', sep_len); pos += sep_len; }
    if (seq_bytes[s]) memcpy(out.data() + pos, text + seq_off[s], (size_t)seq_bytes[s]);
    pos += seq_bytes[s];
  }
}

// The arguments of a run against a scaffold of L bytes; empty when they are fine, otherwise the refusal.  block == 0 is the default.
inline std::string check_args(int stat, uint32_t sep_len, uint32_t block, uint64_t L, const int64_t *starts, const int64_t *sizes, uint64_t nwin) {
  if (stat != STAT_GC && stat != STAT_CD && stat != STAT_TD) return "stat must be 0 (gc), 1 (cd) or 2 (td)";
  if (sep_len > MAX_SEP) return "sep_len must be at most 1024";
  if (block != 0 && (block < MIN_BLOCK || block > MAX_BLOCK)) return "block must be between 16 and 2^20";
  if (L > MAX_SCAFFOLD) return "a scaffold of 2^31 - 1 characters or more is not supported: the prefix counts are 32 bits wide";
  if (nwin > MAX_WINDOWS) return "more than 2^31 - 1 windows in one call";
  if (nwin && (!starts || !sizes)) return "NULL argument";
  for (uint64_t x = 0; x < nwin; ++x) {
    if (sizes[x] < 1) return "window " + std::to_string(x) + ": the size must be at least 1";
    if (starts[x] < 0 || (uint64_t)starts[x] > L || (uint64_t)sizes[x] > L - (uint64_t)starts[x])
      return "window " + std::to_string(x) + " [" + std::to_string(starts[x]) + ", +" + std::to_string(sizes[x]) + ") does not lie inside the scaffold of " + std::to_string(L);
  }
  return std::string();
}
// a refusal of check_args as an error code of the C ABI: what is too large for the 32-bit rows is a range error, the rest an invalid argument
inline int refusal_code(uint64_t L, uint64_t nwin) { return L > MAX_SCAFFOLD || nwin > MAX_WINDOWS ? -7 /* CKM_ERANGE */ : -1 /* CKM_EINVAL */; }

}  // namespace rd
}  // namespace ckm
