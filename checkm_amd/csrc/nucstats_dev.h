// nucstats_dev.h -- the per-lane step of the nucleotide statistics pass (kernels_nucstats.hip), written once for the device and for the
// host executor of the CPU tests (tests/emu/nucstats_emu.cpp), plus the host-side assembly of contig pieces from the tile results.
//
// What one lane sees: 16 bytes of one sequence (the chunk), the byte in front of it and the 12 bytes after it (the halo; the kernel takes
// them from the neighbouring lanes).  What it reports for the chunk bytes that lie inside its tile:
//   - counts of A, C, G, T+U (either case: checkm/util/seqUtils.py:279-286 baseCount), upper-case N, lower-case n (binStatistics.py:230),
//     code points (UTF-8 bytes outside 0x80-0xBF: len(seq) of a Python str) and code points other than 'N' (len(contig.replace('N', ''))),
//   - the starts of runs of at least 10 'N' (a byte that is 'N', whose predecessor in the sequence is not, followed by 9 more 'N'):
//     scaffold.split('NNNNNNNNNN') cuts exactly there, and what lies between two such starts is one contig piece once its 'N' are
//     dropped (binStatistics.py:206-234).  A run crossing a tile seam is found from the halo alone: no run summary has to be combined.
//   - the 4-mer windows starting in the chunk whose four bytes are all A/C/G/T after upper-casing (genomicSignatures.py:131-149; U and
//     anything else is a KeyError there), as 8-bit codes A0 C1 G2 T3, first base most significant.
#pragma once
#include <cstdint>
#include <vector>
#include "wave_const.h"

#if defined(__HIPCC__)
#define NS_HD __host__ __device__ __forceinline__
#else
#define NS_HD inline
#endif

namespace ckm {
namespace ns {

using ckm::LANE_BYTES;
using ckm::WAVE;
using ckm::WAVE_BYTES;                           // one step of a wave over its tile
using ckm::NKMER;
constexpr int HALO = 12;                         // bytes after the chunk a lane looks at: 9 for a run of ten 'N', 3 for a 4-mer
constexpr int NCOUNT = 9;                        // per-tile counters, in this order:
enum { C_A = 0, C_C, C_G, C_TU, C_NU, C_NL, C_CP, C_NONN, C_EV };

struct Lane {
  uint32_t cnt[8];        // C_A .. C_NONN over the chunk bytes inside the tile
  uint32_t nonn_mask;     // bit j: chunk byte j is a code point other than 'N' (inside the tile)
  uint32_t ev_mask;       // bit j: a run of >= 10 'N' starts at chunk byte j
  uint32_t kmer_mask;     // bit j: a valid 4-mer window starts at chunk byte j
  uint8_t  code[LANE_BYTES];
};

NS_HD int base2(uint32_t c) {     // 0 A 1 C 2 G 3 T, -1 anything else (U is not a tetranucleotide base)
  c &= 0xDFu;
  return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : -1;
}

// b[0]: the byte in front of the chunk, b[1 .. 16]: the chunk, b[17 .. 28]: the halo.  nvalid: chunk bytes inside the tile (0..16);
// in_seq: bytes from the chunk's first byte to the end of its sequence (b[1 + i] with i >= in_seq is not part of the sequence);
// has_prev: b[0] is part of the sequence.
NS_HD void lane_step(const uint8_t *b, int nvalid, int64_t in_seq, bool has_prev, Lane &o) {
  for (int k = 0; k < 8; ++k) o.cnt[k] = 0;
  uint32_t isn = 0, acgt = 0;                    // bit k <-> b[k]
  uint8_t two[LANE_BYTES + HALO];
#pragma unroll
  for (int k = 0; k < 1 + LANE_BYTES + HALO; ++k) {
    const bool in = k == 0 ? has_prev : (int64_t)(k - 1) < in_seq;
    const uint32_t c = b[k];
    if (in && c == 'N') isn |= 1u << k;
    if (k >= 1) {
      const int x = in ? base2(c) : -1;
      two[k - 1] = (uint8_t)(x & 3);
      if (x >= 0) acgt |= 1u << (k - 1);
    }
  }
  const uint32_t valid = nvalid >= 32 ? 0xFFFFFFFFu : (1u << nvalid) - 1u;
  uint32_t nonn = 0;
#pragma unroll
  for (int j = 0; j < LANE_BYTES; ++j) {
    if (j >= nvalid) break;
    const uint32_t c = b[1 + j];
    const uint32_t u = c & 0xDFu;
    o.cnt[C_A] += u == 'A';
    o.cnt[C_C] += u == 'C';
    o.cnt[C_G] += u == 'G';
    o.cnt[C_TU] += (u == 'T') | (u == 'U');
    o.cnt[C_NU] += c == 'N';
    o.cnt[C_NL] += c == 'n';
    const uint32_t cp = (c & 0xC0u) != 0x80u;
    o.cnt[C_CP] += cp;
    if (cp && c != 'N') nonn |= 1u << j;
  }
  o.cnt[C_NONN] = (uint32_t)__builtin_popcount(nonn);
  o.nonn_mask = nonn;
  uint32_t run10 = isn;                          // bit k: b[k .. k+9] are all 'N'
#pragma unroll
  for (int s = 1; s < 10; ++s) run10 &= isn >> s;
  o.ev_mask = (run10 >> 1) & ~isn & valid & 0xFFFFu;   // chunk byte j = b[j + 1]; its predecessor b[j] is not 'N'
  o.kmer_mask = acgt & (acgt >> 1) & (acgt >> 2) & (acgt >> 3) & valid & 0xFFFFu;
#pragma unroll
  for (int j = 0; j < LANE_BYTES; ++j)
    o.code[j] = (uint8_t)((two[j] << 6) | (two[j + 1] << 4) | (two[j + 2] << 2) | two[j + 3]);
}

// index of every 4-mer code in _makeKmerColNames order (genomicSignatures.py:40-70): the canonical form is the smaller of the code and its
// reverse complement, and the canonical forms are listed in increasing order (AAAA, AAAC, ..., TTAA)
inline void canonical_table(uint8_t *t /* [256] */) {
  int rank[256];
  int n = 0;
  for (int c = 0; c < 256; ++c) {
    int rc = 0;
    for (int k = 0; k < 4; ++k) rc |= (3 - ((c >> (2 * k)) & 3)) << (2 * (3 - k));
    rank[c] = rc < c ? -1 : n++;
  }
  for (int c = 0; c < 256; ++c) {
    int rc = 0;
    for (int k = 0; k < 4; ++k) rc |= (3 - ((c >> (2 * k)) & 3)) << (2 * (3 - k));
    t[c] = (uint8_t)(rc < c ? rank[rc] : rank[c]);
  }
}

// A sequence's tiles cover it end to end, tile_bytes each (the last one shorter); a tile of a sequence of length 0 does not exist.
struct Tile {
  uint64_t start;       // first byte of the tile in the text
  uint64_t seq_start, seq_end;
  uint32_t len, seq;
};

// Contig pieces of one sequence from its event values (the count of non-'N' code points in front of each run start, ascending) and its
// total of non-'N' code points: the differences, zero-length pieces dropped.  Appends to `out`.
template <class V>
inline void pieces_of(const uint64_t *ev, uint64_t nev, uint64_t nonn_total, V &out) {
  uint64_t prev = 0;
  for (uint64_t k = 0; k <= nev; ++k) {
    const uint64_t at = k < nev ? ev[k] : nonn_total;
    if (at > prev) out.push_back(at - prev);
    prev = at;
  }
}

// host side, shared by the library and the host executor --------------------------------------------------------------------------------

inline std::vector<Tile> make_tiles(const uint64_t *seq_off, const uint64_t *seq_bytes, uint32_t nseq, uint32_t tile_bytes) {
  std::vector<Tile> t;
  for (uint32_t s = 0; s < nseq; ++s)
    for (uint64_t a = 0; a < seq_bytes[s]; a += tile_bytes) {
      const uint64_t n = seq_bytes[s] - a < tile_bytes ? seq_bytes[s] - a : tile_bytes;
      t.push_back(Tile{seq_off[s] + a, seq_off[s], seq_off[s] + seq_bytes[s], (uint32_t)n, s});
    }
  return t;
}

// count pass -> fill pass: the slots of every tile's run starts and the non-'N' code points of its sequence in front of it
inline void scan_tiles(const std::vector<Tile> &tiles, const uint32_t *tile_cnt, std::vector<uint64_t> &ev_off, std::vector<uint64_t> &nonn_base) {
  ev_off.assign(tiles.size() + 1, 0); nonn_base.assign(tiles.size(), 0);
  uint64_t before = 0;
  for (size_t t = 0; t < tiles.size(); ++t) {
    if (t == 0 || tiles[t].seq != tiles[t - 1].seq) before = 0;
    nonn_base[t] = before;
    before += tile_cnt[t * NCOUNT + C_NONN];
    ev_off[t + 1] = ev_off[t] + tile_cnt[t * NCOUNT + C_EV];
  }
}

// per-sequence counters [nseq * 8] and contig pieces (CSR) from the tile counters and the filled run starts
inline void assemble(const std::vector<Tile> &tiles, const uint32_t *tile_cnt, const std::vector<uint64_t> &ev_off, const uint64_t *ev, uint32_t nseq,
                     std::vector<uint64_t> &count, std::vector<uint64_t> &piece_off, std::vector<uint64_t> &piece_len) {
  count.assign((size_t)nseq * 8, 0);
  std::vector<uint64_t> seq_ev0(nseq, 0), seq_ev1(nseq, 0);
  for (size_t t = 0; t < tiles.size(); ++t) {
    const uint32_t s = tiles[t].seq;
    for (int k = 0; k < 8; ++k) count[(size_t)s * 8 + k] += tile_cnt[t * NCOUNT + k];
    if (t == 0 || tiles[t - 1].seq != s) seq_ev0[s] = ev_off[t];
    seq_ev1[s] = ev_off[t + 1];
  }
  piece_off.assign(nseq + 1, 0); piece_len.clear();
  for (uint32_t s = 0; s < nseq; ++s) {
    pieces_of(ev + seq_ev0[s], seq_ev1[s] - seq_ev0[s], count[(size_t)s * 8 + C_NONN], piece_len);
    piece_off[s + 1] = piece_len.size();
  }
}

}  // namespace ns
}  // namespace ckm
