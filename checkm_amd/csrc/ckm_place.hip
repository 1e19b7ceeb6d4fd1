// ckm_place.hip -- C ABI of the phylogenetic placement on the device (kernels_place.hip): the tree, the coded alignment and queries and
// the caller's tables of exponentials go up once and become transition matrices there; the sites then go in chunks of a multiple of 64
// within the byte budget.  Per chunk: the upward and the downward sweep level by level, the edge tables, the scan, whose (query, edge)
// products stay on the device between chunks.  Then the best edges of every query, and a second walk over the chunks for the grid of
// every kept pair (the partials are recomputed; a call of one chunk keeps them).  No result depends on the budget.
#include <string>
#include <vector>
#include "ckm_host.h"
#include "place_dev.h"

namespace ckm {
place::Args place_args_of(const ckm_place_args *a);
int place_check_args(const ckm_place_args *a, place::Schedule &sch, std::string &why);
void launch_place_pmat(hipStream_t st, const double *U, const double *Ui, const double *ex, double *P, uint64_t nmat);
void launch_place_fill(hipStream_t st, double *m, long long *e, uint64_t n);
void launch_place_up(hipStream_t st, const place::PlaceDev &T, const uint32_t *nodes, uint32_t count, uint32_t s0, uint32_t c);
void launch_place_down(hipStream_t st, const place::PlaceDev &T, const uint32_t *nodes, uint32_t count, uint32_t c);
void launch_place_root(hipStream_t st, const place::PlaceDev &T, uint32_t c);
void launch_place_table(hipStream_t st, const place::PlaceDev &T, uint32_t c);
void launch_place_scan(hipStream_t st, const place::PlaceDev &T, uint32_t s0, uint32_t c);
void launch_place_topk(hipStream_t st, const place::PlaceDev &T);
void launch_place_refine(hipStream_t st, const place::PlaceDev &T, uint32_t s0, uint32_t c);
void launch_place_best(hipStream_t st, const place::PlaceDev &T);
}  // namespace ckm
using namespace ckm;


extern "C" int ckm_place_run(ckm_ctx *ctx, const ckm_place_args *a, uint64_t budget_bytes, const ckm_place_out *out, ckm_place_info *info) {
  CallStream cs;
  return guarded([&] {
    if (!ctx || !a || !out) throw Error(CKM_EINVAL, "NULL argument");
    std::string why;
    place::Schedule sch;
    refuse(place_check_args(a, sch, why), why);
    const uint32_t N = a->nnodes, R = a->nrates, S = a->nsites, NQy = a->nqueries, F = a->nfrac, G = a->npend, KP_ = a->max_pitches, E = N - 1;
    const uint32_t Keff = std::min(KP_, E);
    const size_t nout = (size_t)NQy * KP_;
    if (nout && (!out->top_edge || !out->scan_m || !out->scan_e || !out->ref_m || !out->ref_e || !out->ref_f || !out->ref_g)) throw Error(CKM_EINVAL, "NULL argument");
    const WallClock t0;
    budget_bytes = batch_budget(budget_bytes, "CKM_PLACE_BATCH_MB", 2048);
    const uint32_t C = place::chunk_sites(S, N, R, budget_bytes);
    ckm_place_info I = {};
    I.nchunks = (S + C - 1) / C; I.chunk_sites = C; I.nlevels_up = sch.up_off.size() - 1; I.nlevels_down = sch.down_off.size() - 1;
    for (size_t k = 0; k < nout; ++k) { out->top_edge[k] = -1; out->scan_m[k] = out->ref_m[k] = 0.0; out->scan_e[k] = out->ref_e[k] = 0; out->ref_f[k] = out->ref_g[k] = -1; }
    if (NQy) {
      std::vector<uint8_t> rowcode((size_t)a->nrows * S), qcode((size_t)NQy * S);
      for (uint32_t k = 0; k < a->nrows; ++k) for (uint32_t s = 0; s < S; ++s) rowcode[(size_t)k * S + s] = place::code_of(a->rows[a->row_off[k] + s]);
      for (uint32_t k = 0; k < NQy; ++k) for (uint32_t s = 0; s < S; ++s) qcode[(size_t)k * S + s] = place::code_of(a->queries[a->q_off[k] + s]);
      I.ms_pack = t0.ms();
      cs.open(ctx->device);
      DevBuf d_coff, d_child, d_parent, d_leafrow, d_rowcode, d_qcode, d_w, d_pi, d_U, d_Ui, d_elen, d_ehalf, d_edist, d_epend, d_up, d_down, d_edges;
      DevBuf d_Plen, d_Phalf, d_Pdist, d_Ppend, d_D, d_X, d_T, d_dexp, d_xexp, d_texp, d_accm, d_acce, d_raccm, d_racce, d_top, d_sm, d_se, d_rm, d_re, d_rf, d_rg, d_rootv, d_rootexp;
      cs.timed(I.ms_upload, [&] {
        cs.put(d_coff, a->child_off, ((size_t)N + 1) * 8);
        cs.put(d_child, a->child, (size_t)E * 4);
        cs.put(d_parent, sch.parent.data(), (size_t)N * 4);
        cs.put(d_leafrow, sch.leaf_row.data(), (size_t)N * 4);
        cs.put(d_rowcode, rowcode.data(), rowcode.size());
        cs.put(d_qcode, qcode.data(), qcode.size());
        cs.put(d_w, a->weights, (size_t)R * 8);
        cs.put(d_pi, a->pi, place::NS * 8);
        cs.put(d_U, a->U, place::PM * 8);
        cs.put(d_Ui, a->Uinv, place::PM * 8);
        cs.put(d_elen, a->exp_len, (size_t)N * R * place::NS * 8);
        cs.put(d_ehalf, a->exp_half, (size_t)N * R * place::NS * 8);
        cs.put(d_edist, a->exp_dist, (size_t)N * F * 2 * R * place::NS * 8);
        cs.put(d_epend, a->exp_pend, ((size_t)G + 1) * R * place::NS * 8);
        cs.put(d_up, sch.up_nodes.data(), (size_t)N * 4);
        cs.put(d_down, sch.down_nodes.data(), (size_t)E * 4);
        cs.put(d_edges, sch.edges.data(), (size_t)E * 4);
      });
      const size_t part = (size_t)N * R * place::NS * C, npairs = (size_t)NQy * Keff;
      d_Plen.ensure((size_t)N * R * place::PM * 8); d_Phalf.ensure((size_t)N * R * place::PM * 8); d_Pdist.ensure((size_t)N * F * 2 * R * place::PM * 8);
      d_Ppend.ensure(((size_t)G + 1) * R * place::PM * 8);
      d_D.ensure(part * 8); d_X.ensure(part * 8); d_T.ensure((size_t)N * place::NQ * C * 8);
      d_rootv.ensure((size_t)C * 8); d_rootexp.ensure((size_t)C * 4);
      d_dexp.ensure((size_t)N * C * 4); d_xexp.ensure((size_t)N * C * 4); d_texp.ensure((size_t)N * C * 4);
      d_accm.ensure((size_t)N * NQy * 8); d_acce.ensure((size_t)N * NQy * 8); d_raccm.ensure(npairs * F * G * 8); d_racce.ensure(npairs * F * G * 8);
      d_top.ensure(nout * 4); d_sm.ensure(nout * 8); d_se.ensure(nout * 8); d_rm.ensure(nout * 8); d_re.ensure(nout * 8); d_rf.ensure(nout * 4); d_rg.ensure(nout * 4);
      place::PlaceDev T = {};
      T.child_off = d_coff.as<uint64_t>(); T.child = d_child.as<uint32_t>(); T.parent = d_parent.as<int32_t>(); T.leaf_row = d_leafrow.as<int32_t>();
      T.root = sch.root; T.N = N; T.R = R; T.S = S; T.NQy = NQy; T.F = F; T.G = G; T.K = KP_; T.Keff = Keff; T.E = E;
      T.rowcode = d_rowcode.as<uint8_t>(); T.qcode = d_qcode.as<uint8_t>();
      T.weights = d_w.as<double>(); T.pi = d_pi.as<double>(); T.Plen = d_Plen.as<double>(); T.Phalf = d_Phalf.as<double>(); T.Pdist = d_Pdist.as<double>(); T.Ppend = d_Ppend.as<double>();
      T.edges = d_edges.as<uint32_t>();
      T.D = d_D.as<double>(); T.X = d_X.as<double>(); T.T = d_T.as<double>(); T.dexp = d_dexp.as<int32_t>(); T.xexp = d_xexp.as<int32_t>(); T.texp = d_texp.as<int32_t>();
      T.rootv = d_rootv.as<double>(); T.rootexp = d_rootexp.as<int32_t>();
      T.acc_m = d_accm.as<double>(); T.acc_e = d_acce.as<long long>(); T.racc_m = d_raccm.as<double>(); T.racc_e = d_racce.as<long long>();
      T.top_edge = d_top.as<int32_t>(); T.scan_m = d_sm.as<double>(); T.scan_e = d_se.as<long long>(); T.ref_m = d_rm.as<double>(); T.ref_e = d_re.as<long long>();
      T.ref_f = d_rf.as<int32_t>(); T.ref_g = d_rg.as<int32_t>();
      cs.timed(I.ms_matrices, [&] {
        launch_place_pmat(cs.st, d_U.as<double>(), d_Ui.as<double>(), d_elen.as<double>(), d_Plen.as<double>(), (uint64_t)N * R);
        launch_place_pmat(cs.st, d_U.as<double>(), d_Ui.as<double>(), d_ehalf.as<double>(), d_Phalf.as<double>(), (uint64_t)N * R);
        launch_place_pmat(cs.st, d_U.as<double>(), d_Ui.as<double>(), d_edist.as<double>(), d_Pdist.as<double>(), (uint64_t)N * F * 2 * R);
        launch_place_pmat(cs.st, d_U.as<double>(), d_Ui.as<double>(), d_epend.as<double>(), d_Ppend.as<double>(), ((uint64_t)G + 1) * R);
        launch_place_fill(cs.st, T.acc_m, T.acc_e, (uint64_t)N * NQy);
        launch_place_fill(cs.st, T.racc_m, T.racc_e, (uint64_t)npairs * F * G);
        HIPCHK(hipGetLastError());
      });
      auto sweeps = [&](uint32_t s0, uint32_t c) {
        cs.timed(I.ms_sweeps, [&] {
          for (size_t lv = 0; lv + 1 < sch.up_off.size(); ++lv) launch_place_up(cs.st, T, d_up.as<uint32_t>() + sch.up_off[lv], sch.up_off[lv + 1] - sch.up_off[lv], s0, c);
          launch_place_root(cs.st, T, c);
          for (size_t lv = 0; lv + 1 < sch.down_off.size(); ++lv) launch_place_down(cs.st, T, d_down.as<uint32_t>() + sch.down_off[lv], sch.down_off[lv + 1] - sch.down_off[lv], c);
          HIPCHK(hipGetLastError());
        });
      };
      for (uint32_t s0 = 0; s0 < S; s0 += C) {
        const uint32_t c = std::min(C, S - s0);
        sweeps(s0, c);
        cs.timed(I.ms_tables, [&] { launch_place_table(cs.st, T, c); HIPCHK(hipGetLastError()); });
        cs.timed(I.ms_scan, [&] { launch_place_scan(cs.st, T, s0, c); HIPCHK(hipGetLastError()); });
      }
      cs.timed(I.ms_topk, [&] { launch_place_topk(cs.st, T); HIPCHK(hipGetLastError()); });
      for (uint32_t s0 = 0; s0 < S; s0 += C) {
        const uint32_t c = std::min(C, S - s0);
        if (C < S) sweeps(s0, c);
        cs.timed(I.ms_refine, [&] { launch_place_refine(cs.st, T, s0, c); HIPCHK(hipGetLastError()); });
      }
      cs.timed(I.ms_refine, [&] { launch_place_best(cs.st, T); HIPCHK(hipGetLastError()); });
      cs.timed(I.ms_download, [&] {
        // rows of Keff entries into the caller's rows of max_pitches: the device arrays have the caller's layout, the tail is never written
        std::vector<int32_t> h_top(nout), h_rf(nout), h_rg(nout);
        std::vector<double> h_sm(nout), h_rm(nout);
        std::vector<long long> h_se(nout), h_re(nout);
        HIPCHK(hipMemcpyAsync(h_top.data(), d_top.p, nout * 4, hipMemcpyDeviceToHost, cs.st));
        HIPCHK(hipMemcpyAsync(h_sm.data(), d_sm.p, nout * 8, hipMemcpyDeviceToHost, cs.st));
        HIPCHK(hipMemcpyAsync(h_se.data(), d_se.p, nout * 8, hipMemcpyDeviceToHost, cs.st));
        HIPCHK(hipMemcpyAsync(h_rm.data(), d_rm.p, nout * 8, hipMemcpyDeviceToHost, cs.st));
        HIPCHK(hipMemcpyAsync(h_re.data(), d_re.p, nout * 8, hipMemcpyDeviceToHost, cs.st));
        HIPCHK(hipMemcpyAsync(h_rf.data(), d_rf.p, nout * 4, hipMemcpyDeviceToHost, cs.st));
        HIPCHK(hipMemcpyAsync(h_rg.data(), d_rg.p, nout * 4, hipMemcpyDeviceToHost, cs.st));
        HIPCHK(hipStreamSynchronize(cs.st));
        for (uint32_t q = 0; q < NQy; ++q)
          for (uint32_t k = 0; k < Keff; ++k) {
            const size_t at = (size_t)q * KP_ + k;
            out->top_edge[at] = h_top[at]; out->scan_m[at] = h_sm[at]; out->scan_e[at] = h_se[at]; out->ref_m[at] = h_rm[at]; out->ref_e[at] = h_re[at];
            out->ref_f[at] = h_rf[at]; out->ref_g[at] = h_rg[at];
          }
      });
    }
    I.ms_total = t0.ms();
    if (info) *info = I;
  });
}
