// ckm_nearid.hip -- C ABI of the near-identity pass on the device (kernels_nearid.hip): the text and the limits go up once; the row
// tiles are cut into bands whose bit rows fit what the byte budget leaves beside them (nearid::band_end, the host executor's cut).  A
// band's bit rows are cleared (the words left of the diagonal stay 0), one launch fills the words at and right of it, and the rows come
// back at the band's first row in the caller's matrix, so no result depends on the budget.
#include <string>
#include "ckm_host.h"
#include "nearid_dev.h"

namespace ckm {
uint64_t launch_ni_band(hipStream_t st, const uint8_t *text, const uint32_t *limit, uint32_t N, uint32_t L, uint32_t stride, uint32_t b0, uint32_t b1, uint64_t *near);
nearid::Args nearid_args_of(const ckm_nearid_args *a);
int nearid_check_args(const ckm_nearid_args *a, std::string &why);
}  // namespace ckm
using namespace ckm;

extern "C" int ckm_nearid_run(ckm_ctx *ctx, const ckm_nearid_args *a, uint64_t budget_bytes, const ckm_nearid_out *out, ckm_nearid_info *info) {
  CallStream cs;
  return guarded([&] {
    if (!ctx || !a || !out || !out->near) throw Error(CKM_EINVAL, "NULL argument");
    std::string why;
    refuse(nearid_check_args(a, why), why);
    const WallClock t0;
    budget_bytes = batch_budget(budget_bytes, "CKM_NEARID_BATCH_MB", 256);
    const nearid::Args A = nearid_args_of(a);
    const uint32_t N = A.n_rows, W = nearid::words_of(N), nt = nearid::tiles_of(N);
    ckm_nearid_info I = {};
    I.npairs = (uint64_t)N * (N - 1) / 2;
    cs.open(ctx->device);
    DevBuf d_text, d_limit, d_near;
    cs.timed(I.ms_upload, [&] {
      cs.put(d_text, A.text, (uint64_t)N * A.row_stride);
      cs.put(d_limit, A.limit, (uint64_t)N * 4);
    });
    for (uint32_t b0 = 0; b0 < nt;) {
      const uint32_t b1 = nearid::band_end(A, b0, budget_bytes);
      const uint64_t row0 = (uint64_t)b0 * nearid::TILE, row1 = (uint64_t)b1 * nearid::TILE < N ? (uint64_t)b1 * nearid::TILE : N;
      const uint64_t band_bytes = (row1 - row0) * W * 8;
      d_near.ensure(band_bytes);
      cs.timed(I.ms_kernel, [&] {
        HIPCHK(hipMemsetAsync(d_near.p, 0, band_bytes, cs.st));
        I.blocks += launch_ni_band(cs.st, d_text.as<uint8_t>(), d_limit.as<uint32_t>(), N, A.row_len, A.row_stride, b0, b1, d_near.as<uint64_t>());
        HIPCHK(hipGetLastError());
        I.launches += 1;
      });
      cs.timed(I.ms_download, [&] { HIPCHK(hipMemcpyAsync(out->near + row0 * W, d_near.p, band_bytes, hipMemcpyDeviceToHost, cs.st)); });
      I.nbands += 1;
      b0 = b1;
    }
    HIPCHK(hipStreamSynchronize(cs.st));
    I.ms_total = t0.ms();
    if (info) *info = I;
  });
}
