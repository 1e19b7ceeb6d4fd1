// seqwin_dev.h -- the per-lane step of the sequence-window pass (kernels_seqwin.hip), written once for the device and for the host
// executor of the CPU tests (tests/emu/seqwin_emu.cpp), plus the host-side geometry both share: windows, pieces, batches.
//
// The plot commands of CheckM (gc_plot, gc_bias_plot, coding_plot, tetra_plot, dist_plot) walk every sequence in windows of w code
// points: window k = [k w, (k + 1) w) exists while (k + 1) w < L (checkm/plot/gcPlots.py:55-75), so a sequence of L > 0 has
// (L - 1) / w windows and what lies behind the last one (at least one base) is its tail.  Per window: baseCount (A, C, G, T+U after
// upper-casing, checkm/util/seqUtils.py:279-286) and the canonical 4-mers whose four bytes lie INSIDE the window
// (GenomicSignatures.seqSignature(seq[start:end]), checkm/genomicSignatures.py:131-149): a 4-mer across a window seam belongs to no
// window.  The tail is counted for the whole-sequence baseCount of gc_bias_plot only.
//
// A window is cut into pieces of at most piece_bytes; one wavefront owns a piece.  A 4-mer belongs to the piece where it starts: the
// piece reads up to three bytes behind its end (its halo), never beyond the window's end.  What one lane sees: an ALIGNED 16-byte chunk
// of the text and the three bytes after it; which of the chunk's bytes belong to the piece is a pair of indices, because a window starts
// at any byte.  base2, the upper-casing and the canonical table are those of nucstats_dev.h.
#pragma once
#include <cstdint>
#include <vector>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include "nucstats_dev.h"

namespace ckm {
namespace sw {

using ckm::LANE_BYTES;
using ckm::WAVE;
using ckm::WAVE_BYTES;
constexpr int HALO = 3;                          // bytes after the chunk a lane looks at: the rest of a 4-mer
using ckm::NKMER;
constexpr uint32_t ROW_BYTES = NKMER * 4;        // a window's 136 uint32 counts: scratch of a batch, never kept
constexpr uint32_t NO_ROW = 0xFFFFFFFFu;
constexpr uint32_t MIN_PIECE = 16, DEFAULT_PIECE = 4096;
constexpr uint64_t MAX_WINDOWS = 0x7FFFFFFFull;

struct Piece {
  uint64_t start;       // first byte of the piece in the text
  uint32_t len;         // its bytes
  uint32_t cnt_row;     // row of four uint32 (A, C, G, T+U) it adds to: a window's, or the tail's of its sequence
  uint32_t tet_row;     // row of the batch's 136-count scratch, NO_ROW for a tail (no 4-mers are counted there)
  uint32_t flags;       // bits 0-1: halo bytes (window bytes behind the piece's end, at most 3); bit 2: the row is this piece's alone
};

struct Lane {
  uint32_t cnt[4];      // A, C, G, T+U over the chunk bytes inside the piece
  uint32_t kmer_mask;   // bit j: a valid 4-mer of the piece's window starts at chunk byte j
  uint8_t code[LANE_BYTES];
};

// b[0 .. 15]: the chunk, b[16 .. 18]: the bytes after it.  Chunk bytes first .. end-1 belong to the piece (0 <= first, end <= 16) and
// b[k] with k < kend (<= 19) belongs to the piece or its halo.
NS_HD void lane_step(const uint8_t *b, int first, int end, int kend, Lane &o) {
  for (int k = 0; k < 4; ++k) o.cnt[k] = 0;
  uint32_t acgt = 0;
  uint8_t two[LANE_BYTES + HALO];
#pragma unroll
  for (int k = 0; k < LANE_BYTES + HALO; ++k) {
    const int x = (k >= first && k < kend) ? ns::base2(b[k]) : -1;
    two[k] = (uint8_t)(x & 3);
    if (x >= 0) acgt |= 1u << k;
  }
  uint32_t inside = 0;
#pragma unroll
  for (int j = 0; j < LANE_BYTES; ++j) {
    if (j < first || j >= end) continue;
    const uint32_t u = b[j] & 0xDFu;
    o.cnt[0] += u == 'A';
    o.cnt[1] += u == 'C';
    o.cnt[2] += u == 'G';
    o.cnt[3] += (u == 'T') | (u == 'U');
    inside |= 1u << j;
  }
  o.kmer_mask = acgt & (acgt >> 1) & (acgt >> 2) & (acgt >> 3) & inside;
#pragma unroll
  for (int j = 0; j < LANE_BYTES; ++j)
    o.code[j] = (uint8_t)((two[j] << 6) | (two[j + 1] << 4) | (two[j + 2] << 2) | two[j + 3]);
}

// where a lane's chunk lies against its piece: the wave walks 16-byte-aligned spans of 1 KiB from the aligned chunk that holds the piece's first byte
struct LaneGeom { uint64_t base; int first, end, kend; bool load; };
NS_HD LaneGeom lane_geom(const Piece &P, uint64_t step /* 16-byte-aligned start of the wave's 1 KiB span */, int lane) {
  LaneGeom g;
  g.base = step + (uint64_t)lane * LANE_BYTES;
  const int64_t a = (int64_t)P.start - (int64_t)g.base, z = a + (int64_t)P.len, kz = z + (int64_t)(P.flags & 3u);
  g.first = a < 0 ? 0 : a > LANE_BYTES ? LANE_BYTES : (int)a;
  g.end = z < 0 ? 0 : z > LANE_BYTES ? LANE_BYTES : (int)z;
  g.kend = kz < 0 ? 0 : kz > LANE_BYTES + HALO ? LANE_BYTES + HALO : (int)kz;
  g.load = a < LANE_BYTES && kz > 0;             // the chunk holds a byte of the piece or of its halo
  return g;
}

// host side, shared by the library and the host executor --------------------------------------------------------------------------------

// len(seq) of a Python str: UTF-8 bytes outside 0x80-0xBF
inline uint64_t code_points(const char *text, uint64_t off, uint64_t bytes) {
  uint64_t n = 0;
  for (uint64_t i = 0; i < bytes; ++i) n += ((uint8_t)text[off + i] & 0xC0u) != 0x80u;
  return n;
}
inline uint64_t windows_of(uint64_t len, uint64_t w) { return len ? (len - 1) / w : 0; }

// First window of every sequence from its code points (first[nseq] = all windows); false when there are more than MAX_WINDOWS.  The one
// numbering of the layout, the coding and the run entry points.
inline bool window_layout(const uint64_t *len, uint32_t nseq, uint64_t w, std::vector<uint64_t> &first) {
  first.assign((size_t)nseq + 1, 0);
  for (uint32_t s = 0; s < nseq; ++s) {
    first[s + 1] = first[s] + windows_of(len[s], w);
    if (first[s + 1] > MAX_WINDOWS) return false;
  }
  return true;
}

// one batch of windows: the pieces the count kernel takes, and per window of the batch the file whose bin signature it is compared with
struct Batch {
  std::vector<Piece> pieces;
  std::vector<uint32_t> win_file;
  uint64_t win0 = 0;                              // first window of the batch in the call's numbering
  uint32_t nwin = 0;
};
struct Cursor { uint32_t seq = 0; uint64_t k = 0, win = 0; };

// Fills `b` with the next at most max_windows windows (and the tails of the sequences that end in it); false when nothing is left.
// seq_len: code points; a sequence with skip[s] != 0 (its bytes are not its code points) keeps its windows in the numbering and gets no
// piece.  Tail rows follow the nwin_total window rows: row nwin_total + s.
inline bool next_batch(const uint64_t *seq_off, const uint64_t *seq_len, const uint8_t *skip, const uint32_t *seq_file, uint32_t nseq, uint64_t w,
                       uint32_t piece_bytes, uint64_t max_windows, uint64_t nwin_total, Cursor &c, Batch &b) {
  b.pieces.clear(); b.win_file.clear(); b.win0 = c.win; b.nwin = 0;
  auto cut = [&](uint64_t start, uint64_t len, uint64_t room /* window bytes from start */, uint32_t cnt_row, uint32_t tet_row) {
    for (uint64_t o = 0; o < len; o += piece_bytes) {
      const uint64_t n = len - o < piece_bytes ? len - o : piece_bytes;
      const uint64_t halo = room - o - n < (uint64_t)HALO ? room - o - n : (uint64_t)HALO;
      b.pieces.push_back(Piece{start + o, (uint32_t)n, cnt_row, tet_row, (uint32_t)halo | (len <= piece_bytes ? 4u : 0u)});
    }
  };
  while (c.seq < nseq) {
    const uint32_t s = c.seq;
    const uint64_t L = seq_len[s], nw = windows_of(L, w);
    while (c.k < nw && b.nwin < max_windows) {
      if (!skip[s]) cut(seq_off[s] + c.k * w, w, w, (uint32_t)c.win, b.nwin);
      b.win_file.push_back(seq_file[s]);
      ++c.k; ++c.win; ++b.nwin;
    }
    if (c.k < nw) return true;
    if (!skip[s] && L) cut(seq_off[s] + nw * w, L - nw * w, L - nw * w, (uint32_t)(nwin_total + s), NO_ROW);
    ++c.seq; c.k = 0;
  }
  return b.nwin > 0 || !b.pieces.empty();
}

// baseCount of every whole sequence: its windows' rows and its tail's
inline void seq_counts(const uint32_t *cnt /* [(nwin + nseq) * 4] */, const uint64_t *first /* [nseq + 1] */, uint32_t nseq, uint64_t *out /* [nseq * 4] */) {
  const uint64_t nwin = first[nseq];
  for (uint32_t s = 0; s < nseq; ++s)
    for (int k = 0; k < 4; ++k) {
      uint64_t t = cnt[(nwin + s) * 4 + k];
      for (uint64_t x = first[s]; x < first[s + 1]; ++x) t += cnt[x * 4 + k];
      out[(uint64_t)s * 4 + k] = t;
    }
}

}  // namespace sw
}  // namespace ckm
