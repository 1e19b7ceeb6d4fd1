// ckm_unbinned.hip -- C ABI of the selective base count of `checkm unbinned` (kernels_unbinned.hip): a batch read by ckm_nucseq_read and a
// keep flag per sequence in; A, C, G, T+U and the code points of every kept sequence out.  Only the tiles of kept sequences travel: their
// padded text is packed into batches of a byte budget, the tile rows of all batches stay on the device and are summed per sequence at the end.
#include <cstdlib>
#include <cstring>
#include <vector>
#include "ckm_host.h"
#include "nucstats_host.h"
#include "unbinned_dev.h"

namespace ckm {
void launch_unbinned_count(hipStream_t st, const uint8_t *text, const ub::Tile *tiles, uint32_t ntiles, uint32_t *rows);
void launch_unbinned_sum(hipStream_t st, const uint32_t *rows, const uint64_t *first_tile, uint32_t nkept, uint64_t *out);
}  // namespace ckm
using namespace ckm;

extern "C" int ckm_unbinned_count(ckm_ctx *ctx, const ckm_nucseq *b, const uint8_t *keep, uint32_t tile_bytes, uint64_t budget_bytes, uint64_t *counts,
                                  ckm_unbinned_timing *timing) {
  CallStream cs;
  return guarded([&] {
    if (!ctx || !b || !keep || !counts || !timing) throw Error(CKM_EINVAL, "NULL argument");
    if (tile_bytes == 0) tile_bytes = ub::DEFAULT_TILE;
    if (tile_bytes % ub::WAVE_BYTES || tile_bytes > ub::MAX_TILE) throw Error(CKM_EINVAL, "tile_bytes must be a multiple of 1024 and at most 1 MiB");
    budget_bytes = batch_budget(budget_bytes, "CKM_NUCSTATS_BATCH_MB", 1024);
    const WallClock t0;
    *timing = ckm_unbinned_timing{};
    const uint32_t nseq = (uint32_t)b->seq_off.size();
    if (nseq) memset(counts, 0, (size_t)nseq * ub::NCOUNT * 8);
    std::vector<ub::HostTile> tiles;
    std::vector<uint64_t> first_tile;
    std::vector<uint32_t> kept;
    ub::make_tiles(b->seq_off.data(), b->seq_bytes.data(), keep, nseq, tile_bytes, tiles, first_tile, kept);
    const uint32_t nkept = (uint32_t)kept.size();
    timing->kept = nkept; timing->tiles = tiles.size();
    if (!tiles.empty()) {
      cs.open(ctx->device);
      DevBuf d_text, d_tiles, d_rows, d_first, d_out;
      d_rows.ensure(tiles.size() * ub::NCOUNT * 4);
      std::vector<char> stage;
      ub::Batch B;
      uint64_t cursor = 0;
      while (ub::next_batch(tiles, budget_bytes, cursor, B)) {
        if (B.tiles.size() > 0x7FFFFFF0ull) throw Error(CKM_ERANGE, "too many tiles in one batch: use a larger tile_bytes or a smaller budget");
        const uint32_t nt = (uint32_t)B.tiles.size();
        // every chunk the kernel loads lies inside the packed text: a tile's padded end is at most the batch's bytes
        for (const ub::Tile &T : B.tiles)
          if (T.start % ub::LANE_BYTES || T.start + ub::pad16(T.len) > B.bytes) throw Error(CKM_EINVAL, "internal: a tile leaves its batch");
        const char *src = b->text.data() + B.spans[0].src;      // one run of the reader's text goes up as it lies
        const WallClock s0;
        if (B.spans.size() > 1) {
          stage.resize(B.bytes);
          for (const ub::Span &S : B.spans) memcpy(stage.data() + S.dst, b->text.data() + S.src, S.bytes);
          src = stage.data();
        }
        timing->ms_stage += s0.ms();
        cs.mark(0);
        cs.put(d_text, src, B.bytes);
        cs.put(d_tiles, B.tiles.data(), (size_t)nt * sizeof(ub::Tile));
        cs.mark(1);
        launch_unbinned_count(cs.st, d_text.as<uint8_t>(), d_tiles.as<ub::Tile>(), nt, d_rows.as<uint32_t>() + B.t0 * ub::NCOUNT);
        HIPCHK(hipGetLastError());
        cs.mark(2);
        HIPCHK(hipStreamSynchronize(cs.st));                        // the next batch reuses the text, the tiles and the staging buffer
        timing->ms_upload += cs.ms(0, 1);
        timing->ms_count += cs.ms(1, 2);
        timing->batches += 1; timing->bytes += B.bytes;
      }
      d_out.ensure((size_t)nkept * ub::NCOUNT * 8);
      std::vector<uint64_t> out((size_t)nkept * ub::NCOUNT);
      cs.put(d_first, first_tile.data(), first_tile.size() * 8);
      cs.mark(0);
      launch_unbinned_sum(cs.st, d_rows.as<uint32_t>(), d_first.as<uint64_t>(), nkept, d_out.as<uint64_t>());
      HIPCHK(hipGetLastError());
      cs.mark(1);
      HIPCHK(hipMemcpyAsync(out.data(), d_out.p, out.size() * 8, hipMemcpyDeviceToHost, cs.st));
      cs.mark(2);
      HIPCHK(hipStreamSynchronize(cs.st));
      timing->ms_sum = cs.ms(0, 1);
      timing->ms_download = cs.ms(1, 2);
      for (uint32_t k = 0; k < nkept; ++k) memcpy(counts + (size_t)kept[k] * ub::NCOUNT, &out[(size_t)k * ub::NCOUNT], ub::NCOUNT * 8);
    }
    timing->ms_total = t0.ms();
  });
}
