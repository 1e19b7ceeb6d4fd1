// nucstats_emu.cpp -- TEST INFRASTRUCTURE: the tile logic of the nucleotide statistics pass (checkm_amd/csrc/nucstats_dev.h: the lane step,
// the tiling, the count -> scan -> fill assembly of contig pieces) compiled by g++ against a HOST executor, so that the CPU test suite can
// pin the tile seams (runs of 'N' and 4-mers crossing them) with tiles forced small.  The wavefront is restated as a loop over its 64
// lanes; the halo a lane takes from its neighbours in kernels_nucstats.hip is read from memory here.  Nothing in checkm_amd loads this.
#include <cstring>
#include <vector>
#include "../../checkm_amd/csrc/nucstats_dev.h"

using namespace ckm::ns;

static void lane_bytes(const uint8_t *text, const Tile &T, uint64_t off, int lane, uint8_t *b, int &nvalid, int64_t &in_seq, bool &has_prev) {
  const uint64_t base = T.start + off + (uint64_t)lane * LANE_BYTES;
  const int64_t rem = (int64_t)T.len - (int64_t)(off + (uint64_t)lane * LANE_BYTES);
  nvalid = rem <= 0 ? 0 : rem >= LANE_BYTES ? LANE_BYTES : (int)rem;
  in_seq = (int64_t)T.seq_end - (int64_t)base;
  has_prev = base > T.seq_start;
  b[0] = has_prev ? text[base - 1] : 0;
  for (int k = 0; k < LANE_BYTES + HALO; ++k) b[1 + k] = (int64_t)k < in_seq ? text[base + k] : 0;
}

extern "C" int emu_nucstats(const uint8_t *text, const uint64_t *seq_off, const uint64_t *seq_bytes, uint32_t nseq, uint32_t tile_bytes,
                            uint64_t *count /* [nseq*8] */, uint32_t *tetra /* [nseq*136] */, uint64_t *piece_off /* [nseq+1] */,
                            uint64_t *piece_len, uint64_t piece_cap) {
  uint8_t canon[256];
  canonical_table(canon);
  const std::vector<Tile> tiles = make_tiles(seq_off, seq_bytes, nseq, tile_bytes);
  std::vector<uint32_t> cnt(tiles.size() * NCOUNT, 0);
  memset(tetra, 0, (size_t)nseq * NKMER * 4);
  for (size_t t = 0; t < tiles.size(); ++t) {                  // count pass
    const Tile &T = tiles[t];
    uint32_t hist[NKMER] = {0};
    for (uint64_t off = 0; off < T.len; off += WAVE_BYTES)
      for (int lane = 0; lane < WAVE; ++lane) {
        uint8_t b[1 + LANE_BYTES + HALO]; int nvalid; int64_t in_seq; bool has_prev;
        lane_bytes(text, T, off, lane, b, nvalid, in_seq, has_prev);
        Lane o;
        lane_step(b, nvalid, in_seq, has_prev, o);
        for (int k = 0; k < 8; ++k) cnt[t * NCOUNT + k] += o.cnt[k];
        cnt[t * NCOUNT + C_EV] += (uint32_t)__builtin_popcount(o.ev_mask);
        for (int j = 0; j < LANE_BYTES; ++j) if (o.kmer_mask >> j & 1) ++hist[canon[o.code[j]]];
      }
    for (int k = 0; k < NKMER; ++k) tetra[(size_t)T.seq * NKMER + k] += hist[k];
  }
  std::vector<uint64_t> ev_off, nonn_base;
  scan_tiles(tiles, cnt.data(), ev_off, nonn_base);
  std::vector<uint64_t> ev(ev_off.empty() ? 0 : ev_off.back());
  for (size_t t = 0; t < tiles.size(); ++t) {                  // fill pass
    const Tile &T = tiles[t];
    uint64_t slot = ev_off[t], before = nonn_base[t];
    for (uint64_t off = 0; off < T.len; off += WAVE_BYTES)
      for (int lane = 0; lane < WAVE; ++lane) {
        uint8_t b[1 + LANE_BYTES + HALO]; int nvalid; int64_t in_seq; bool has_prev;
        lane_bytes(text, T, off, lane, b, nvalid, in_seq, has_prev);
        Lane o;
        lane_step(b, nvalid, in_seq, has_prev, o);
        for (int j = 0; j < LANE_BYTES; ++j) if (o.ev_mask >> j & 1) ev[slot++] = before + (uint64_t)__builtin_popcount(o.nonn_mask & ((1u << j) - 1u));
        before += (uint64_t)__builtin_popcount(o.nonn_mask);
      }
    if (slot != ev_off[t + 1]) return -1;
  }
  std::vector<uint64_t> c, po, pl;
  assemble(tiles, cnt.data(), ev_off, ev.data(), nseq, c, po, pl);
  if (pl.size() > piece_cap) return -2;
  memcpy(count, c.data(), c.size() * 8);
  memcpy(piece_off, po.data(), po.size() * 8);
  if (!pl.empty()) memcpy(piece_len, pl.data(), pl.size() * 8);
  return 0;
}
