// ckm_select.hip -- C ABI of the marker-set selection's draws on the device (kernels_select.hip): the genomes, the keys and the marker sets
// of a call go up once; the draws (genome, replicate) are cut into rounds whose output rows, scratch rows and multiplicity rows fit the
// byte budget, one launch per round.  A round's results land in the caller's arrays at the round's first draw, so no result depends on
// the budget.  Nothing of a draw goes up: the kernel makes it from the call's seed.
#include <chrono>
#include <string>
#include <vector>
#include "ckm_host.h"
#include "select_dev.h"

namespace ckm {
struct SelectDev {
  const int64_t *genome_len; const uint32_t *ncontigs; const uint64_t *row_off; const uint32_t *key_off; const int32_t *key;
  const uint32_t *ms_off, *cs_off, *cs_marker, *num_markers; uint32_t U, S, R; sel::Params P;
};
void launch_select(hipStream_t st, const SelectDev &T, uint32_t max_contigs, uint32_t d0, uint32_t nd, uint64_t row_base, double *truth, double *out, uint32_t *scratch,
                   uint16_t *rows);
sel::Args select_args_of(const ckm_select_args *a);
int select_check_args(const ckm_select_args *a, std::string &why);
}  // namespace ckm
using namespace ckm;

static void put(CallStream &cs, DevBuf &d, const void *src, size_t bytes) {
  d.ensure(bytes);
  if (bytes) HIPCHK(hipMemcpyAsync(d.p, src, bytes, hipMemcpyHostToDevice, cs.st));
}

extern "C" int ckm_select_run(ckm_ctx *ctx, const ckm_select_args *a, uint64_t budget_bytes, const ckm_select_out *out, ckm_select_info *info) {
  CallStream cs;
  return guarded([&] {
    if (!ctx || !a) throw Error(CKM_EINVAL, "NULL argument");
    std::string why;
    const int kind = select_check_args(a, why);
    if (kind != sim::ARGS_OK) throw Error(kind == sim::ARGS_RANGE ? CKM_ERANGE : CKM_EINVAL, why);
    const uint32_t G = a->ngenomes, R = a->nreplicates, S = a->nsets, U = a->nmarkers;
    const uint32_t D = G * R;
    if (D && (!out || !out->truth || (S && !out->out))) throw Error(CKM_EINVAL, "NULL argument");
    const auto t0 = std::chrono::steady_clock::now();
    budget_bytes = batch_budget(budget_bytes, "CKM_SELECT_BATCH_MB", 256);
    ckm_select_info I = {};
    if (D) {
      sel::Packed P;
      sel::pack(select_args_of(a), P);
      const bool with_rows = out->rows != nullptr;
      I.ms_pack = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      cs.open(ctx->device);
      DevBuf d_len, d_nc, d_row, d_koff, d_key, d_msoff, d_csoff, d_csm, d_num, d_scratch, d_truth, d_out, d_rows;
      cs.timed(I.ms_upload, [&] {
        put(cs, d_len, a->genome_len, (size_t)G * 8);
        put(cs, d_nc, P.ncontigs.data(), (size_t)G * 4);
        put(cs, d_row, P.row_off.data(), P.row_off.size() * 8);
        put(cs, d_koff, P.key_off.data(), P.key_off.size() * 4);
        put(cs, d_key, P.key.data(), P.key.size() * 4);
        put(cs, d_msoff, P.sets.ms_off.data(), P.sets.ms_off.size() * 4);
        put(cs, d_csoff, P.sets.cs_off.data(), P.sets.cs_off.size() * 4);
        put(cs, d_csm, P.sets.cs_marker.data(), P.sets.cs_marker.size() * 4);
        put(cs, d_num, P.sets.num_markers.data(), P.sets.num_markers.size() * 4);
      });
      const SelectDev T = {d_len.as<int64_t>(), d_nc.as<uint32_t>(), d_row.as<uint64_t>(), d_koff.as<uint32_t>(), d_key.as<int32_t>(), d_msoff.as<uint32_t>(),
                           d_csoff.as<uint32_t>(), d_csm.as<uint32_t>(), d_num.as<uint32_t>(), U, S, R, P.params};
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
    I.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (info) *info = I;
  });
}
