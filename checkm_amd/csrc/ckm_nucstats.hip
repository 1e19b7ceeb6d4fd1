// ckm_nucstats.hip -- C ABI of the nucleotide statistics pass (kernels_nucstats.hip): a batch read by ckm_nucseq_read in, per-sequence base
// counts, contig pieces and (optionally) canonical 4-mer counts out.  Count pass, scan of the per-tile run starts on the host, fill pass.
#include <memory>
#include <vector>
#include "ckm_host.h"
#include "nucstats_dev.h"
#include "nucstats_host.h"

namespace ckm {
void launch_nucstats_count(hipStream_t st, const uint8_t *text, const ns::Tile *tiles, uint32_t ntiles, const uint8_t *canon, uint32_t *tile_cnt, uint32_t *tetra);
void launch_nucstats_fill(hipStream_t st, const uint8_t *text, const ns::Tile *tiles, uint32_t ntiles, const uint64_t *ev_off, const uint64_t *nonn_base, uint64_t *ev);
}  // namespace ckm
using namespace ckm;

struct ckm_nucstats {
  uint32_t nseq = 0;
  std::vector<uint64_t> count, piece_off, piece_len;
  std::vector<uint32_t> tetra;
  uint64_t bytes = 0, tiles = 0, run_starts = 0;
  double ms_upload = 0, ms_count = 0, ms_fill = 0, ms_total = 0;
};

extern "C" int ckm_nucstats_run(ckm_ctx *ctx, const ckm_nucseq *b, int tetra, uint32_t tile_bytes, ckm_nucstats **out) {
  CallStream cs;
  return guarded([&] {
    if (!ctx || !b || !out) throw Error(CKM_EINVAL, "NULL argument");
    if (tile_bytes == 0) tile_bytes = 4096;                 // measured best of 4, 16, 64, 256 KiB (DESIGN.md section "Bin statistics")
    if (tile_bytes % ns::LANE_BYTES || tile_bytes > (1u << 20)) throw Error(CKM_EINVAL, "tile_bytes must be a multiple of 16 and at most 1 MiB");
    *out = nullptr;
    const WallClock t0;
    cs.open(ctx->device);
    const uint32_t nseq = (uint32_t)b->seq_off.size();
    std::unique_ptr<ckm_nucstats> o(new ckm_nucstats());
    o->nseq = nseq;
    const std::vector<ns::Tile> tiles = ns::make_tiles(b->seq_off.data(), b->seq_bytes.data(), nseq, tile_bytes);
    const uint32_t nt = (uint32_t)tiles.size();
    if (tiles.size() > 0xFFFFFFF0ull) throw Error(CKM_ERANGE, "too many tiles in one batch");
    uint8_t canon[256];
    ns::canonical_table(canon);
    DevBuf d_text, d_tiles, d_canon, d_cnt, d_tetra, d_evoff, d_base, d_ev;
    d_tiles.ensure(std::max<size_t>(1, nt) * sizeof(ns::Tile));
    d_cnt.ensure(std::max<size_t>(1, nt) * ns::NCOUNT * 4);
    if (tetra) d_tetra.ensure(std::max<size_t>(1, nseq) * ns::NKMER * 4);
    cs.mark(0);
    cs.put(d_text, b->text.data(), b->text.size());
    if (nt) HIPCHK(hipMemcpyAsync(d_tiles.p, tiles.data(), nt * sizeof(ns::Tile), hipMemcpyHostToDevice, cs.st));
    cs.put(d_canon, canon, 256);
    if (tetra) HIPCHK(hipMemsetAsync(d_tetra.p, 0, std::max<size_t>(1, nseq) * ns::NKMER * 4, cs.st));
    cs.mark(1);
    launch_nucstats_count(cs.st, d_text.as<uint8_t>(), d_tiles.as<ns::Tile>(), nt, d_canon.as<uint8_t>(), d_cnt.as<uint32_t>(), tetra ? d_tetra.as<uint32_t>() : nullptr);
    HIPCHK(hipGetLastError());
    cs.mark(2);
    std::vector<uint32_t> cnt((size_t)nt * ns::NCOUNT);
    if (nt) HIPCHK(hipMemcpyAsync(cnt.data(), d_cnt.p, cnt.size() * 4, hipMemcpyDeviceToHost, cs.st));
    if (tetra) {
      o->tetra.resize((size_t)nseq * ns::NKMER);
      if (nseq) HIPCHK(hipMemcpyAsync(o->tetra.data(), d_tetra.p, o->tetra.size() * 4, hipMemcpyDeviceToHost, cs.st));
    }
    HIPCHK(hipStreamSynchronize(cs.st));
    std::vector<uint64_t> ev_off, nonn_base;
    ns::scan_tiles(tiles, cnt.data(), ev_off, nonn_base);
    const uint64_t nev = ev_off.empty() ? 0 : ev_off.back();
    std::vector<uint64_t> evs(nev);
    float ms_fill = 0.f;
    if (nev) {
      d_ev.ensure(nev * 8);
      cs.put(d_evoff, ev_off.data(), ev_off.size() * 8);
      cs.put(d_base, nonn_base.data(), nonn_base.size() * 8);
      cs.mark(3);
      launch_nucstats_fill(cs.st, d_text.as<uint8_t>(), d_tiles.as<ns::Tile>(), nt, d_evoff.as<uint64_t>(), d_base.as<uint64_t>(), d_ev.as<uint64_t>());
      HIPCHK(hipGetLastError());
      cs.mark(4);
      HIPCHK(hipMemcpyAsync(evs.data(), d_ev.p, nev * 8, hipMemcpyDeviceToHost, cs.st));
      HIPCHK(hipStreamSynchronize(cs.st));
      ms_fill = cs.ms(3, 4);
    }
    ns::assemble(tiles, cnt.data(), ev_off, evs.data(), nseq, o->count, o->piece_off, o->piece_len);
    o->ms_upload = cs.ms(0, 1); o->ms_count = cs.ms(1, 2); o->ms_fill = ms_fill;
    o->bytes = b->text.size(); o->tiles = nt; o->run_starts = nev;
    o->ms_total = t0.ms();
    *out = o.release();
  });
}

extern "C" int ckm_nucstats_columns_get(const ckm_nucstats *r, ckm_nucstats_columns *c) {
  if (!r || !c) { set_last_error("NULL argument"); return CKM_EINVAL; }
  c->nseq = r->nseq; c->count = r->count.data(); c->piece_off = r->piece_off.data(); c->piece_len = r->piece_len.data();
  c->tetra = r->tetra.empty() ? nullptr : r->tetra.data();
  c->bytes = r->bytes; c->tiles = r->tiles; c->run_starts = r->run_starts;
  c->ms_upload = r->ms_upload; c->ms_count = r->ms_count; c->ms_fill = r->ms_fill; c->ms_total = r->ms_total;
  return CKM_OK;
}

extern "C" void ckm_nucstats_free(ckm_nucstats *r) { delete r; }
