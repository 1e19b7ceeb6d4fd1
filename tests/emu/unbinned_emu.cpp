// unbinned_emu.cpp -- TEST INFRASTRUCTURE: the per-word logic and the geometry of the selective base count of `checkm unbinned`
// (checkm_amd/csrc/unbinned_dev.h) compiled by g++ against a HOST executor, so that the CPU test suite runs the kernel's own arithmetic.
// The kernels of kernels_unbinned.hip are restated as loops over their wavefronts and lanes; the batches pack the kept tiles' text as
// ckm_unbinned_count does, into a buffer of exactly the batch's bytes.  Nothing in checkm_amd loads this.
#include <cstring>
#include <vector>
#include "../../checkm_amd/csrc/unbinned_dev.h"

using namespace ckm;

namespace {
// one wavefront over one tile: unbinned_count_kernel
void run_tile(const std::vector<uint8_t> &text, const ub::Tile &T, uint32_t *row) {
  uint32_t acc[ub::NCOUNT] = {0, 0, 0, 0, 0};
  for (int lane = 0; lane < ub::WAVE; ++lane)
    for (uint32_t off = (uint32_t)lane * ub::LANE_BYTES; off < T.len; off += ub::WAVE_BYTES) {
      uint32_t w[4];
      memcpy(w, &text.at(T.start + off + ub::LANE_BYTES - 1) - (ub::LANE_BYTES - 1), ub::LANE_BYTES);     // .at(): the chunk's last byte is in the batch
      const uint32_t rem = T.len - off;
      ub::lane_counts(w, rem >= (uint32_t)ub::LANE_BYTES ? ub::LANE_BYTES : (int)rem, acc);
    }
  for (int k = 0; k < ub::NCOUNT; ++k) row[k] = acc[k];
}
}  // namespace

// ckm_unbinned_count on the host.  tile_bytes: any multiple of 16.  info: kept, tiles, batches, bytes.  Returns 0, or -1 for a bad argument.
extern "C" int emu_unbinned_count(const char *text, const uint64_t *seq_off, const uint64_t *seq_bytes, uint32_t nseq, const uint8_t *keep, uint32_t tile_bytes,
                                  uint64_t budget_bytes, uint64_t *counts, uint64_t *info) {
  if (!tile_bytes || tile_bytes % ub::LANE_BYTES || !budget_bytes) return -1;
  memset(counts, 0, (size_t)nseq * ub::NCOUNT * 8);
  std::vector<ub::HostTile> tiles;
  std::vector<uint64_t> first_tile;
  std::vector<uint32_t> kept;
  ub::make_tiles(seq_off, seq_bytes, keep, nseq, tile_bytes, tiles, first_tile, kept);
  std::vector<uint32_t> rows(tiles.size() * ub::NCOUNT, 0xDEADBEEFu);
  std::vector<uint8_t> dev;
  ub::Batch B;
  uint64_t cursor = 0;
  info[2] = info[3] = 0;
  while (ub::next_batch(tiles, budget_bytes, cursor, B)) {
    dev.assign(B.bytes, 0xAA);
    for (const ub::Span &S : B.spans) memcpy(dev.data() + S.dst, text + S.src, S.bytes);
    for (size_t t = 0; t < B.tiles.size(); ++t) run_tile(dev, B.tiles[t], &rows[(B.t0 + t) * ub::NCOUNT]);
    info[2] += 1; info[3] += B.bytes;
  }
  for (size_t k = 0; k < kept.size(); ++k) ub::sum_rows(rows.data(), first_tile[k], first_tile[k + 1], counts + (size_t)kept[k] * ub::NCOUNT);
  info[0] = kept.size(); info[1] = tiles.size();
  return 0;
}
