// ckm_select.hip -- C ABI of the marker-set selection's draws on the device (kernels_select.hip): the genomes, the keys and the marker sets
// of a call go up once; the draws (genome, replicate) are cut into rounds whose output rows, scratch rows and multiplicity rows fit the
// byte budget, one launch per round.  A round's results land in the caller's arrays at the round's first draw, so no result depends on
// the budget.  Nothing of a draw goes up: the kernel makes it from the call's seed.
#include <string>
#include <vector>
#include "ckm_host.h"
#include "select_dev.h"

namespace ckm {
void launch_select(hipStream_t st, const sel::SelectDev &T, uint32_t max_contigs, uint32_t d0, uint32_t nd, uint64_t row_base, double *truth, double *out, uint32_t *scratch,
                   uint16_t *rows);
sel::Args select_args_of(const ckm_select_args *a);
int select_check_args(const ckm_select_args *a, std::string &why);
}  // namespace ckm
using namespace ckm;

extern "C" int ckm_select_run(ckm_ctx *ctx, const ckm_select_args *a, uint64_t budget_bytes, const ckm_select_out *out, ckm_select_info *info) {
  CallStream cs;
  return guarded([&] {
    if (!ctx || !a) throw Error(CKM_EINVAL, "NULL argument");
    std::string why;
    refuse(select_check_args(a, why), why);
    const uint32_t G = a->ngenomes, R = a->nreplicates, S = a->nsets, U = a->nmarkers;
    const uint32_t D = G * R;
    if (D && (!out || !out->truth || (S && !out->out))) throw Error(CKM_EINVAL, "NULL argument");
    const WallClock t0;
    budget_bytes = batch_budget(budget_bytes, "CKM_SELECT_BATCH_MB", 256);
    ckm_select_info I = {};
    if (D) {
      sel::Packed P;
      sel::pack(select_args_of(a), P);
      const bool with_rows = out->rows != nullptr;
      I.ms_pack = t0.ms();
      cs.open(ctx->device);
      DevBuf d_len, d_nc, d_row, d_koff, d_key, d_scratch, d_truth, d_out, d_rows;
      SetsBufs d_sets;
      cs.timed(I.ms_upload, [&] {
        cs.put(d_len, a->genome_len, (size_t)G * 8);
        cs.put(d_nc, P.ncontigs.data(), (size_t)G * 4);
        cs.put(d_row, P.row_off.data(), P.row_off.size() * 8);
        cs.put(d_koff, P.key_off.data(), P.key_off.size() * 4);
        cs.put(d_key, P.key.data(), P.key.size() * 4);
        d_sets.upload(cs, P.sets);
      });
      const sel::SelectDev T = {d_len.as<int64_t>(), d_nc.as<uint32_t>(), d_row.as<uint64_t>(), d_koff.as<uint32_t>(), d_key.as<int32_t>(), d_sets.dev(), U, R, P.params};
      for (uint32_t d0 = 0; d0 < D;) {
        const uint32_t d1 = sel::next_round(P, R, U, S, with_rows, budget_bytes, d0), nd = d1 - d0;
        const uint64_t row_base = sel::row_at(P, R, d0), nrow = sel::row_at(P, R, d1) - row_base;
        if (U > sim::STAGE_COUNTS) d_scratch.ensure((size_t)nd * U * 4);
        d_truth.ensure((size_t)nd * 16);
        d_out.ensure((size_t)nd * S * sim::OUT_BYTES);
        if (with_rows) d_rows.ensure(nrow * 2);
        cs.timed(I.ms_kernel, [&] {
          launch_select(cs.st, T, P.max_contigs, d0, nd, row_base, d_truth.as<double>(), d_out.as<double>(), d_scratch.as<uint32_t>(), with_rows ? d_rows.as<uint16_t>() : nullptr);
          HIPCHK(hipGetLastError());
        });
        cs.timed(I.ms_download, [&] {
          HIPCHK(hipMemcpyAsync(out->truth + (size_t)d0 * 2, d_truth.p, (size_t)nd * 16, hipMemcpyDeviceToHost, cs.st));
          if (S) HIPCHK(hipMemcpyAsync(out->out + (size_t)d0 * S * 4, d_out.p, (size_t)nd * S * sim::OUT_BYTES, hipMemcpyDeviceToHost, cs.st));
          if (with_rows && nrow) HIPCHK(hipMemcpyAsync(out->rows + row_base, d_rows.p, nrow * 2, hipMemcpyDeviceToHost, cs.st));
        });
        I.nrounds += 1;
        d0 = d1;
      }
    }
    I.ms_total = t0.ms();
    if (info) *info = I;
  });
}
