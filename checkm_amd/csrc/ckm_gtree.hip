// ckm_gtree.hip -- C ABI of the genome tree on the device (kernels_gtree.hip): the alignment goes up once and is encoded there; the trees
// of a call (the alignment itself, the replicates, or the caller's matrices) are cut into batches whose encoded alignments, counts,
// matrices and join state fit the byte budget.  A batch is gathered, counted, turned into distances and joined by launches on the call's
// stream -- the join loop is queued whole, the host waits once per batch -- and only its merge rows come back, at the batch's first tree
// in the caller's arrays, so no result depends on the budget.
#include <string>
#include <vector>
#include "ckm_host.h"
#include "gtree_dev.h"

namespace ckm {
void launch_gt_encode(hipStream_t st, const uint8_t *text, uint32_t N, uint32_t L, uint8_t *enc);
void launch_gt_gather(hipStream_t st, const uint8_t *enc, const uint32_t *cols, uint32_t N, uint32_t L, uint32_t trees, uint8_t *out);
void launch_gt_counts(hipStream_t st, const uint8_t *enc, uint64_t tree_stride, uint32_t N, uint32_t L, uint32_t trees, uint32_t *cmp, uint32_t *dif);
void launch_gt_dist(hipStream_t st, const uint32_t *cmp, const uint32_t *dif, uint32_t N, uint32_t trees, int model, double max_dist, double *D);
uint64_t launch_gt_join(hipStream_t st, double *D, uint32_t N, uint32_t trees, double *R, uint32_t *list_a, uint32_t *list_b, double *row_q, uint32_t *row_b, uint32_t *merge_ij,
                        double *merge_len);
gtree::Args gtree_args_of(const ckm_gtree_args *a);
int gtree_check_args(const ckm_gtree_args *a, std::string &why);
}  // namespace ckm
using namespace ckm;

extern "C" int ckm_gtree_run(ckm_ctx *ctx, const ckm_gtree_args *a, uint64_t budget_bytes, const ckm_gtree_out *out, ckm_gtree_info *info) {
  CallStream cs;
  return guarded([&] {
    if (!ctx || !a || !out) throw Error(CKM_EINVAL, "NULL argument");
    std::string why;
    refuse(gtree_check_args(a, why), why);
    if ((out->compared && !out->differ) || (out->merge_ij && !out->merge_len)) throw Error(CKM_EINVAL, "NULL argument");
    const WallClock t0;
    budget_bytes = batch_budget(budget_bytes, "CKM_GTREE_BATCH_MB", 2048);
    const bool from_matrix = a->matrix != nullptr;
    const uint32_t N = a->nrows, L = from_matrix ? 0 : a->ncols, T = gtree::trees_of(gtree_args_of(a));
    const uint64_t NN = (uint64_t)N * N, enc_bytes = (uint64_t)N * gtree::padded(L);
    ckm_gtree_info I = {};
    I.ntrees = T;
    cs.open(ctx->device);
    DevBuf d_text, d_enc, d_cols, d_rep, d_cmp, d_dif, d_D, d_R, d_la, d_lb, d_rq, d_rb, d_ij, d_len;
    if (!from_matrix) {
      cs.timed(I.ms_upload, [&] {
        d_enc.ensure(enc_bytes);
        cs.put(d_text, a->text, a->ntext_bytes);
        launch_gt_encode(cs.st, d_text.as<uint8_t>(), N, L, d_enc.as<uint8_t>());
        HIPCHK(hipGetLastError());
      });
      if (out->compared || out->dist) {
        d_cmp.ensure(NN * 4); d_dif.ensure(NN * 4);
        cs.timed(I.ms_counts, [&] { launch_gt_counts(cs.st, d_enc.as<uint8_t>(), 0, N, L, 1, d_cmp.as<uint32_t>(), d_dif.as<uint32_t>()); HIPCHK(hipGetLastError()); });
        if (out->dist) {
          d_D.ensure(NN * 8);
          cs.timed(I.ms_dist, [&] { launch_gt_dist(cs.st, d_cmp.as<uint32_t>(), d_dif.as<uint32_t>(), N, 1, a->model, a->max_dist, d_D.as<double>()); HIPCHK(hipGetLastError()); });
        }
        cs.timed(I.ms_download, [&] {
          if (out->compared) {
            HIPCHK(hipMemcpyAsync(out->compared, d_cmp.p, NN * 4, hipMemcpyDeviceToHost, cs.st));
            HIPCHK(hipMemcpyAsync(out->differ, d_dif.p, NN * 4, hipMemcpyDeviceToHost, cs.st));
          }
          if (out->dist) HIPCHK(hipMemcpyAsync(out->dist, d_D.p, NN * 8, hipMemcpyDeviceToHost, cs.st));
        });
      }
    }
    if (out->merge_ij) {
      for (uint32_t t0t = 0; t0t < T;) {
        const uint32_t nt = gtree::batch_trees(N, L, budget_bytes, T - t0t);
        d_D.ensure(NN * 8 * nt); d_R.ensure((uint64_t)N * 8 * nt); d_la.ensure((uint64_t)N * 4 * nt); d_lb.ensure((uint64_t)N * 4 * nt);
        d_rq.ensure((uint64_t)N * 8 * nt); d_rb.ensure((uint64_t)N * 4 * nt); d_ij.ensure((uint64_t)(N - 1) * 8 * nt); d_len.ensure((uint64_t)(N - 1) * 16 * nt);
        if (from_matrix) {
          cs.timed(I.ms_upload, [&] { HIPCHK(hipMemcpyAsync(d_D.p, a->matrix + (uint64_t)t0t * NN, NN * 8 * nt, hipMemcpyHostToDevice, cs.st)); });
        } else {
          // the batch's trees: the alignment itself first when the batch begins the call, then replicates r0 .. r0 + nr
          const uint32_t nb = (a->base && t0t == 0) ? 1u : 0u, nr = nt - nb, r0 = t0t + nb - a->base;
          d_cmp.ensure(NN * 4 * nt); d_dif.ensure(NN * 4 * nt);
          if (nr) {
            d_rep.ensure(enc_bytes * nr);
            cs.timed(I.ms_upload, [&] { cs.put(d_cols, a->cols + (uint64_t)r0 * L, (uint64_t)nr * L * 4); });
            cs.timed(I.ms_gather, [&] { launch_gt_gather(cs.st, d_enc.as<uint8_t>(), d_cols.as<uint32_t>(), N, L, nr, d_rep.as<uint8_t>()); HIPCHK(hipGetLastError()); });
          }
          cs.timed(I.ms_counts, [&] {
            launch_gt_counts(cs.st, d_enc.as<uint8_t>(), 0, N, L, nb, d_cmp.as<uint32_t>(), d_dif.as<uint32_t>());
            launch_gt_counts(cs.st, d_rep.as<uint8_t>(), enc_bytes, N, L, nr, d_cmp.as<uint32_t>() + NN * nb, d_dif.as<uint32_t>() + NN * nb);
            HIPCHK(hipGetLastError());
          });
          cs.timed(I.ms_dist, [&] { launch_gt_dist(cs.st, d_cmp.as<uint32_t>(), d_dif.as<uint32_t>(), N, nt, a->model, a->max_dist, d_D.as<double>()); HIPCHK(hipGetLastError()); });
        }
        cs.timed(I.ms_joins, [&] {
          I.launches += launch_gt_join(cs.st, d_D.as<double>(), N, nt, d_R.as<double>(), d_la.as<uint32_t>(), d_lb.as<uint32_t>(), d_rq.as<double>(), d_rb.as<uint32_t>(),
                                       d_ij.as<uint32_t>(), d_len.as<double>());
          HIPCHK(hipGetLastError());
        });
        cs.timed(I.ms_download, [&] {
          HIPCHK(hipMemcpyAsync(out->merge_ij + (uint64_t)t0t * (N - 1) * 2, d_ij.p, (uint64_t)(N - 1) * 8 * nt, hipMemcpyDeviceToHost, cs.st));
          HIPCHK(hipMemcpyAsync(out->merge_len + (uint64_t)t0t * (N - 1) * 2, d_len.p, (uint64_t)(N - 1) * 16 * nt, hipMemcpyDeviceToHost, cs.st));
        });
        I.nrounds += 1;
        t0t += nt;
      }
    }
    HIPCHK(hipStreamSynchronize(cs.st));
    I.ms_total = t0.ms();
    if (info) *info = I;
  });
}
