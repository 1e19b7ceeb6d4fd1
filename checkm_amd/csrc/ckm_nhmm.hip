// ckm_nhmm.hip -- C ABI of the nucleotide model scan on the device (kernels_nhmm.hip): the text of the contigs and the image of every
// model go up once; the tiles then go in batches whose row buffer (8 bytes per owned row) stays inside the byte budget.  Per batch: one
// scan launch per model with tiles in it, the tiles' counts come back, the host scans them, and one fill launch writes the reported rows
// in (tile, row) order.  The hits are formed on the host from the few rows that survive.  No result depends on the budget.
#include <string>
#include <vector>
#include "ckm_host.h"
#include "nhmm_dev.h"
#include "nucstats_host.h"

namespace ckm {
nhmm::Args nhmm_args_of(const ckm_nhmm_args *a);
int nhmm_check_args(const ckm_nhmm_args *a, std::string &why);
void launch_nhmm_scan(hipStream_t st, int Q, const int32_t *image, int32_t tBM, const nhmm::TileDev *tiles, uint32_t ntiles, const uint8_t *text, long long *rowbuf, uint32_t *counts);
void launch_nhmm_fill(hipStream_t st, const long long *rowbuf, const nhmm::TileDev *tiles, const uint64_t *dst_off, uint32_t ntiles, uint32_t *o_tile, uint32_t *o_pos, uint32_t *o_start, int32_t *o_score);
}  // namespace ckm
using namespace ckm;


extern "C" int ckm_nhmm_run(ckm_ctx *ctx, const ckm_nhmm_args *a, const ckm_nucseq *b, uint64_t budget_bytes, ckm_nhmm_result **out, ckm_nhmm_info *info) {
  CallStream cs;
  return guarded([&] {
    if (!ctx || !a || !b || !out) throw Error(CKM_EINVAL, "NULL argument");
    *out = nullptr;
    std::string why;
    refuse(nhmm_check_args(a, why), why);
    const WallClock t0;
    const nhmm::Args A = nhmm_args_of(a);
    const nhmm::Seqs S = {b->text.data(), b->seq_off.data(), b->seq_bytes.data(), (uint32_t)b->seq_off.size()};
    bool too_long = false;
    const int64_t bad = nhmm::first_refused_seq(S, too_long);
    if (bad >= 0) {
      if (too_long) throw Error(CKM_ERANGE, "sequence " + b->ids[bad] + " has 2^31 - 1 bytes or more");
      throw Error(CKM_EINVAL, "sequence " + b->ids[bad] + " holds a byte beyond ASCII: the model scan reads A, C, G, T, U and ASCII placeholders");
    }
    budget_bytes = batch_budget(budget_bytes, "CKM_SSU_BATCH_MB", 256);
    ckm_nhmm_info I = {};
    std::unique_ptr<ckm_nhmm_result> R(new ckm_nhmm_result);
    std::vector<nhmm::Tile> tiles = A.nmodels ? nhmm::make_tiles(A, S) : std::vector<nhmm::Tile>();
    I.tiles = tiles.size();
    if (!tiles.empty()) {
      // the images of the models, one after the other
      std::vector<int> Q(A.nmodels);
      std::vector<size_t> img_off(A.nmodels + 1, 0);
      std::vector<int32_t> images;
      for (uint32_t m = 0; m < A.nmodels; ++m) {
        Q[m] = nhmm::q_of(A.M[m]);
        const std::vector<int32_t> img = nhmm::device_image(A, m, Q[m]);
        images.insert(images.end(), img.begin(), img.end());
        img_off[m + 1] = images.size();
      }
      I.ms_tables = t0.ms();
      cs.open(ctx->device);
      DevBuf d_text, d_img, d_tiles, d_rowbuf, d_counts, d_dst, d_otile, d_opos, d_ostart, d_oscore;
      cs.timed(I.ms_upload, [&] {
        cs.put(d_text, b->text.data(), b->text.size());
        cs.put(d_img, images.data(), images.size() * 4);
      });
      std::vector<nhmm::TileDev> td;
      std::vector<uint32_t> counts, h_tile, h_pos, h_start;
      std::vector<int32_t> h_score;
      std::vector<uint64_t> dst;
      for (size_t from = 0, to; from < tiles.size(); from = to) {
        uint64_t nrows = 0;
        to = nhmm::cut_batch(tiles, from, budget_bytes, nrows);
        const size_t nt = to - from;
        if (nt > 0xffffffffull) throw Error(CKM_ERANGE, "more than 2^32 tiles in a batch");
        td.resize(nt);
        for (size_t k = 0; k < nt; ++k) {
          const nhmm::Tile &t = tiles[from + k];
          td[k] = nhmm::TileDev{S.off[t.seq], t.out_off, (uint32_t)S.bytes[t.seq], t.first, t.own, t.last, t.strand, t.model, A.min_score[t.model], 0};
          I.cells += nhmm::tile_cells(A, t);
        }
        cs.timed(I.ms_upload, [&] { cs.put(d_tiles, td.data(), nt * sizeof(nhmm::TileDev)); });
        d_rowbuf.ensure(nrows * 8); d_counts.ensure(nt * 4);
        cs.timed(I.ms_scan, [&] {
          for (size_t k = 0, z; k < nt; k = z) {      // the tiles of one model are consecutive
            for (z = k; z < nt && td[z].model == td[k].model;) ++z;
            const uint32_t m = td[k].model;
            launch_nhmm_scan(cs.st, Q[m], d_img.as<int32_t>() + img_off[m], nhmm::tbm_of(A.M[m]), d_tiles.as<nhmm::TileDev>() + k, (uint32_t)(z - k), d_text.as<uint8_t>(),
                             d_rowbuf.as<long long>(), d_counts.as<uint32_t>() + k);
            ++I.launches;
          }
          HIPCHK(hipGetLastError());
        });
        counts.resize(nt); dst.resize(nt);
        uint64_t total = 0;
        cs.timed(I.ms_compact, [&] {
          HIPCHK(hipMemcpyAsync(counts.data(), d_counts.p, nt * 4, hipMemcpyDeviceToHost, cs.st));
          HIPCHK(hipStreamSynchronize(cs.st));
          for (size_t k = 0; k < nt; ++k) {
            if (counts[k] > td[k].last - td[k].own + 1) throw Error(CKM_EHIP, "the scan counted more rows in a tile than it owns");
            dst[k] = total; total += counts[k];
          }
          if (total) {
            cs.put(d_dst, dst.data(), nt * 8);
            d_otile.ensure(total * 4); d_opos.ensure(total * 4); d_ostart.ensure(total * 4); d_oscore.ensure(total * 4);
            launch_nhmm_fill(cs.st, d_rowbuf.as<long long>(), d_tiles.as<nhmm::TileDev>(), d_dst.as<uint64_t>(), (uint32_t)nt, d_otile.as<uint32_t>(), d_opos.as<uint32_t>(),
                             d_ostart.as<uint32_t>(), d_oscore.as<int32_t>());
            HIPCHK(hipGetLastError());
          }
        });
        if (total) {
          h_tile.resize(total); h_pos.resize(total); h_start.resize(total); h_score.resize(total);
          cs.timed(I.ms_download, [&] {
            HIPCHK(hipMemcpyAsync(h_tile.data(), d_otile.p, total * 4, hipMemcpyDeviceToHost, cs.st));
            HIPCHK(hipMemcpyAsync(h_pos.data(), d_opos.p, total * 4, hipMemcpyDeviceToHost, cs.st));
            HIPCHK(hipMemcpyAsync(h_start.data(), d_ostart.p, total * 4, hipMemcpyDeviceToHost, cs.st));
            HIPCHK(hipMemcpyAsync(h_score.data(), d_oscore.p, total * 4, hipMemcpyDeviceToHost, cs.st));
            HIPCHK(hipStreamSynchronize(cs.st));
          });
          nhmm::Rows &w = R->rows;
          for (uint64_t k = 0; k < total; ++k) {
            if (h_tile[k] >= nt) throw Error(CKM_EHIP, "the fill wrote a row of no tile of its batch");
            const nhmm::Tile &t = tiles[from + h_tile[k]];
            w.model.push_back(t.model); w.seq.push_back(t.seq); w.strand.push_back(t.strand); w.pos.push_back(h_pos[k]); w.start.push_back(h_start[k]); w.score.push_back(h_score[k]);
          }
        }
        ++I.batches;
      }
      const WallClock th;
      nhmm::hits_host(S, R->rows, R->hits);
      I.ms_hits = th.ms();
    }
    I.ms_total = t0.ms();
    if (info) *info = I;
    *out = R.release();
  });
}
