// ckm_markerset.hip -- C ABI of MarkerSetBuilder on the device (kernels_markerset.hip): a resident table of count classes and copy
// positions; the marker pass over a batch of queries (one flag byte per query and family); the co-location pass over a batch of queries
// (the reported marker pairs of every query in (i, j) order).  The co-location pass runs in rounds of whole queries whose packed entries
// and tile counts fit the byte budget -- pack, count, scan, then the fill pass in batches of whole rows whose output fits the budget --
// so the memory of a call does not grow with the number of queries or of reported pairs, and no result depends on the budget.
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>
#include "ckm_host.h"
#include "markerset_dev.h"
#include "pairs_host.h"

namespace ckm {
using ms::MsetOut;
using ms::MsetTableDev;
void launch_mset_markers(hipStream_t st, const MsetTableDev &T, uint32_t q0, uint32_t nq, const uint64_t *qg_off, const uint32_t *qg, const double *tU, const double *tS,
                         uint8_t *flag, uint32_t *counts);
void launch_mset_pack(hipStream_t st, const MsetTableDev &T, const ms::Query *queries, uint32_t nq, uint64_t nentries, const uint32_t *qg, const uint32_t *qm, ms::Entry *pk);
void launch_mset_tiles(hipStream_t st, bool fill, const MsetTableDev &T, const ms::Query *queries, const ms::Tile *tiles, uint32_t t_lo, uint32_t t_hi, const uint32_t *qg,
                       const uint32_t *qm, const ms::Entry *pk, int32_t D, double genome_threshold, uint32_t row_lo, uint32_t row_hi, uint32_t *tile_count, const MsetOut &out);
void launch_mset_scan(hipStream_t st, const ms::Query *queries, uint32_t nq, uint32_t nrows, uint32_t *tile_count, uint32_t *row_total);
}  // namespace ckm
using namespace ckm;

struct ckm_mset_table {
  int device = 0;
  uint32_t G = 0, C = 0;
  uint64_t npos = 0;
  DevBuf d_cls, d_off, d_pos;
  double ms_upload = 0;
  MsetTableDev dev() const { return MsetTableDev{d_cls.as<uint8_t>(), d_off.as<uint32_t>(), d_pos.as<int32_t>(), G, C}; }
};

struct ckm_mset_result {
  uint64_t nqueries = 0, nfamilies = 0, npairs = 0, nbatches = 0, nrounds = 0, tests = 0;
  bool has_counts = false;
  std::vector<uint8_t> flag;
  std::vector<uint32_t> counts;
  std::vector<uint64_t> pair_off;
  std::vector<uint32_t> pi, pj, count;
  double ms_upload = 0, ms_markers = 0, ms_pack = 0, ms_count = 0, ms_scan = 0, ms_fill = 0, ms_download = 0, ms_total = 0;
};

extern "C" int ckm_mset_table_create(ckm_ctx *ctx, uint32_t ngenomes, uint32_t nfamilies, const uint8_t *count_class, const uint64_t *pos_off, const int64_t *pos,
                                     double *ms_upload, ckm_mset_table **out) {
  CallStream cs;
  return guarded([&] {
    if (!ctx || !out) throw Error(CKM_EINVAL, "NULL argument");
    *out = nullptr;
    std::string why;
    refuse(ms::check_table(ngenomes, nfamilies, count_class, pos_off, pos, why), why);
    std::unique_ptr<ckm_mset_table> t(new ckm_mset_table());
    t->device = ctx->device; t->G = ngenomes; t->C = nfamilies;
    const uint64_t cells = (uint64_t)ngenomes * nfamilies;
    t->npos = pos_off[cells];
    std::vector<uint32_t> off(cells + 1);
    for (uint64_t k = 0; k <= cells; ++k) off[k] = (uint32_t)pos_off[k];
    std::vector<int32_t> p(t->npos);
    for (uint64_t k = 0; k < t->npos; ++k) p[k] = (int32_t)pos[k];
    cs.open(ctx->device);
    cs.timed(t->ms_upload, [&] {
      cs.put(t->d_cls, count_class, cells);
      cs.put(t->d_off, off.data(), (cells + 1) * 4);
      cs.put(t->d_pos, p.data(), t->npos * 4);
    });
    if (ms_upload) *ms_upload = t->ms_upload;
    *out = t.release();
  });
}

extern "C" void ckm_mset_table_free(ckm_mset_table *t) {
  if (!t) return;
  (void)hipSetDevice(t->device);
  delete t;
}

extern "C" int ckm_mset_markers(ckm_ctx *ctx, const ckm_mset_table *t, uint32_t nqueries, const uint64_t *qg_off, const uint32_t *qg, const double *ubiquity_threshold,
                                const double *single_copy_threshold, int want_counts, uint64_t budget_bytes, ckm_mset_result **out) {
  CallStream cs;
  return guarded([&] {
    if (!ctx || !t || !out || (nqueries && (!ubiquity_threshold || !single_copy_threshold))) throw Error(CKM_EINVAL, "NULL argument");
    *out = nullptr;
    if (t->device != ctx->device) throw Error(CKM_EINVAL, "the table lives on another device");
    std::string why;
    refuse(ms::check_queries(t->G, t->C, nqueries, qg_off, qg, nullptr, nullptr, why), why);
    const WallClock t0;
    budget_bytes = batch_budget(budget_bytes, "CKM_MSET_BATCH_MB", 256);
    std::unique_ptr<ckm_mset_result> o(new ckm_mset_result());
    o->nqueries = nqueries; o->nfamilies = t->C; o->has_counts = want_counts != 0;
    const uint64_t C = t->C, per_query = C * (want_counts ? 13 : 1);
    o->flag.resize((size_t)nqueries * C);
    if (want_counts) o->counts.resize((size_t)nqueries * C * 3);
    if (nqueries && C) {
      cs.open(ctx->device);
      DevBuf d_goff, d_g, d_tu, d_ts, d_flag, d_counts;
      cs.timed(o->ms_upload, [&] {
        cs.put(d_goff, qg_off, ((size_t)nqueries + 1) * 8);
        cs.put(d_g, qg, qg_off[nqueries] * 4);
        cs.put(d_tu, ubiquity_threshold, (size_t)nqueries * 8);
        cs.put(d_ts, single_copy_threshold, (size_t)nqueries * 8);
      });
      const uint32_t step = (uint32_t)std::min<uint64_t>(65535, std::max<uint64_t>(1, budget_bytes / per_query));
      d_flag.ensure((size_t)step * C);
      if (want_counts) d_counts.ensure((size_t)step * C * 12);
      for (uint32_t q0 = 0; q0 < nqueries; q0 += step) {
        const uint32_t n = std::min<uint32_t>(step, nqueries - q0);
        cs.timed(o->ms_markers, [&] {
          launch_mset_markers(cs.st, t->dev(), q0, n, d_goff.as<uint64_t>(), d_g.as<uint32_t>(), d_tu.as<double>(), d_ts.as<double>(), d_flag.as<uint8_t>(),
                              want_counts ? d_counts.as<uint32_t>() : nullptr);
          HIPCHK(hipGetLastError());
        });
        cs.timed(o->ms_download, [&] {
          HIPCHK(hipMemcpyAsync(o->flag.data() + (size_t)q0 * C, d_flag.p, (size_t)n * C, hipMemcpyDeviceToHost, cs.st));
          if (want_counts) HIPCHK(hipMemcpyAsync(o->counts.data() + (size_t)q0 * C * 3, d_counts.p, (size_t)n * C * 12, hipMemcpyDeviceToHost, cs.st));
        });
        o->nbatches += 1;
      }
    }
    o->ms_total = t0.ms();
    *out = o.release();
  });
}

extern "C" int ckm_mset_colocated(ckm_ctx *ctx, const ckm_mset_table *t, uint32_t nqueries, const uint64_t *qg_off, const uint32_t *qg, const uint64_t *qm_off,
                                  const uint32_t *qm, double dist_threshold, double genome_threshold, uint64_t budget_bytes, ckm_mset_result **out) {
  CallStream cs;
  return guarded([&] {
    if (!ctx || !t || !out || !qm_off) throw Error(CKM_EINVAL, "NULL argument");
    *out = nullptr;
    if (t->device != ctx->device) throw Error(CKM_EINVAL, "the table lives on another device");
    std::string why;
    refuse(ms::check_dist(dist_threshold, why), why);
    refuse(ms::check_queries(t->G, t->C, nqueries, qg_off, qg, qm_off, qm, why), why);
    const WallClock t0;
    budget_bytes = batch_budget(budget_bytes, "CKM_MSET_BATCH_MB", 256);
    const uint64_t cap_pairs = ms::budget_pairs(budget_bytes);
    const int32_t D = (int32_t)dist_threshold;
    std::unique_ptr<ckm_mset_result> o(new ckm_mset_result());
    o->nqueries = nqueries; o->nfamilies = t->C;
    o->pair_off.assign((size_t)nqueries + 1, 0);
    uint64_t work = 0;
    for (uint32_t q = 0; q < nqueries; ++q) {
      const uint64_t ng = qg_off[q + 1] - qg_off[q], nm = qm_off[q + 1] - qm_off[q];
      const uint64_t tests = nm ? ng * (nm * (nm - 1) / 2) : 0;
      o->tests += tests; work += ms::query_tiles(ng, nm);
    }
    if (work) {
      cs.open(ctx->device);
      const MsetTableDev T = t->dev();
      DevBuf d_g, d_m, d_q, d_tiles, d_pk, d_cnt;
      PairBatches pb;
      cs.timed(o->ms_upload, [&] {
        cs.put(d_g, qg, qg_off[nqueries] * 4);
        cs.put(d_m, qm, qm_off[nqueries] * 4);
      });
      ms::Round R;
      auto take = [&](const void *h_out, uint64_t n) {
        const uint32_t *hi = static_cast<const uint32_t *>(h_out);
        o->pi.insert(o->pi.end(), hi, hi + n); o->pj.insert(o->pj.end(), hi + n, hi + 2 * n); o->count.insert(o->count.end(), hi + 2 * n, hi + 3 * n);
        o->npairs += n; o->nbatches += 1;
      };
      for (uint32_t q0 = 0; q0 < nqueries;) {
        const uint32_t q1 = ms::next_round(nqueries, qg_off, qm_off, budget_bytes, q0);
        ms::build_round(qg_off, qm_off, q0, q1, R);
        const uint32_t nq = q1 - q0, nrows = R.rows, ntiles = (uint32_t)R.tiles.size();
        if (ntiles) {
          o->nrounds += 1;
          d_pk.ensure(R.entries * sizeof(ms::Entry)); d_cnt.ensure(R.counts * 4);
          cs.timed(o->ms_upload, [&] {
            cs.put(d_q, R.queries.data(), (size_t)nq * sizeof(ms::Query));
            cs.put(d_tiles, R.tiles.data(), (size_t)ntiles * sizeof(ms::Tile));
          });
          const ms::Query *dq = d_q.as<ms::Query>();
          const ms::Tile *dt = d_tiles.as<ms::Tile>();
          cs.timed(o->ms_pack, [&] { launch_mset_pack(cs.st, T, dq, nq, R.entries, d_g.as<uint32_t>(), d_m.as<uint32_t>(), d_pk.as<ms::Entry>()); HIPCHK(hipGetLastError()); });
          const MsetOut none = {nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr};
          cs.timed(o->ms_count, [&] {
            launch_mset_tiles(cs.st, false, T, dq, dt, 0, ntiles, d_g.as<uint32_t>(), d_m.as<uint32_t>(), d_pk.as<ms::Entry>(), D, genome_threshold, 0, nrows,
                              d_cnt.as<uint32_t>(), none);
            HIPCHK(hipGetLastError());
          });
          pb.run(cs, 0, nrows, cap_pairs, ms::PAIR_BYTES, o->ms_scan, o->ms_fill, o->ms_download,
                 [&](uint32_t *d_total) { launch_mset_scan(cs.st, dq, nq, nrows, d_cnt.as<uint32_t>(), d_total); },
                 [&](const pc::Group &g, void *d_out, uint64_t n) {
                   uint32_t *di = static_cast<uint32_t *>(d_out);
                   const MsetOut mo = {pb.d_base.as<uint64_t>(), pb.d_total.as<uint32_t>(), g.base, n, di, di + n, di + 2 * n};
                   const ms::TileRange tr = ms::tile_range(g, R.tiles);
                   launch_mset_tiles(cs.st, true, T, dq, dt, tr.t_lo, tr.t_hi, d_g.as<uint32_t>(), d_m.as<uint32_t>(), d_pk.as<ms::Entry>(), D, genome_threshold, g.row_lo, g.row_hi,
                                     d_cnt.as<uint32_t>(), mo);
                 },
                 take);
          const WallClock s0;
          for (uint32_t q = q0; q < q1; ++q) {
            const ms::Query &Q = R.queries[q - q0];
            uint64_t n = 0;
            for (uint32_t k = 0; k < Q.nrows; ++k) n += pb.row_total[Q.row_off + k];
            o->pair_off[q + 1] = o->pair_off[q] + n;
          }
          o->ms_scan += s0.ms();
        } else {
          for (uint32_t q = q0; q < q1; ++q) o->pair_off[q + 1] = o->pair_off[q];
        }
        q0 = q1;
      }
    }
    o->ms_total = t0.ms();
    *out = o.release();
  });
}

extern "C" int ckm_mset_columns_get(const ckm_mset_result *r, ckm_mset_columns *c) {
  if (!r || !c) { set_last_error("NULL argument"); return CKM_EINVAL; }
  c->nqueries = r->nqueries; c->nfamilies = r->nfamilies; c->npairs = r->npairs; c->nbatches = r->nbatches; c->nrounds = r->nrounds; c->tests = r->tests;
  c->flag = r->flag.data(); c->counts = r->has_counts ? r->counts.data() : nullptr;
  c->pair_off = r->pair_off.data(); c->i = r->pi.data(); c->j = r->pj.data(); c->count = r->count.data();
  c->ms_upload = r->ms_upload; c->ms_markers = r->ms_markers; c->ms_pack = r->ms_pack; c->ms_count = r->ms_count; c->ms_scan = r->ms_scan; c->ms_fill = r->ms_fill;
  c->ms_download = r->ms_download; c->ms_total = r->ms_total;
  return CKM_OK;
}

extern "C" void ckm_mset_result_free(ckm_mset_result *r) { delete r; }
