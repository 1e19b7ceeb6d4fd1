// ckm_sim.hip -- C ABI of the marker-set simulation on the device (kernels_sim.hip): the keys and the marker sets of a call go up once,
// the replicates in rounds of whole replicates whose starts, output rows and scratch rows fit the byte budget, one launch per round.  A
// round's results land in the caller's array at the round's first replicate, so no result depends on the budget.
#include <chrono>
#include <string>
#include <vector>
#include "ckm_host.h"
#include "sim_dev.h"

namespace ckm {
struct SimDev { const uint32_t *key_off; const int32_t *key; const uint32_t *ms_off, *cs_off, *cs_marker, *num_markers; uint32_t U, S; };
void launch_sim(hipStream_t st, const SimDev &T, uint32_t r0, uint32_t nr, const uint64_t *rs_off, uint64_t start_base, const int32_t *starts, const int32_t *contig_len,
                uint32_t *scratch, double *out);
int sim_check_args(const ckm_sim_args *a, std::string &why);
}  // namespace ckm
using namespace ckm;

static void put(CallStream &cs, DevBuf &d, const void *src, size_t bytes) {
  d.ensure(bytes);
  if (bytes) HIPCHK(hipMemcpyAsync(d.p, src, bytes, hipMemcpyHostToDevice, cs.st));
}

extern "C" int ckm_sim_run(ckm_ctx *ctx, const ckm_sim_args *a, uint64_t budget_bytes, double *out, ckm_sim_info *info) {
  CallStream cs;
  return guarded([&] {
    if (!ctx || !a) throw Error(CKM_EINVAL, "NULL argument");
    std::string why;
    const int kind = sim_check_args(a, why);
    if (kind != sim::ARGS_OK) throw Error(kind == sim::ARGS_RANGE ? CKM_ERANGE : CKM_EINVAL, why);
    const uint32_t R = a->nreplicates, S = a->nsets, U = a->nmarkers;
    if (R && S && !out) throw Error(CKM_EINVAL, "NULL argument");
    const auto t0 = std::chrono::steady_clock::now();
    budget_bytes = batch_budget(budget_bytes, "CKM_SIM_BATCH_MB", 256);
    ckm_sim_info I = {};
    if (R && S) {
      const sim::Args A = {U, a->key_off, a->key, S, a->ms_off, a->cs_off, a->cs_marker, R, a->rs_off, a->starts, a->contig_len};
      sim::Packed P;
      sim::pack(A, P);
      std::vector<int32_t> h_starts;
      I.ms_pack = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      cs.open(ctx->device);
      DevBuf d_koff, d_key, d_msoff, d_csoff, d_csm, d_num, d_rsoff, d_len, d_starts, d_scratch, d_out;
      cs.timed(I.ms_upload, [&] {
        put(cs, d_koff, P.key_off.data(), P.key_off.size() * 4);
        put(cs, d_key, P.key.data(), P.key.size() * 4);
        put(cs, d_msoff, P.ms_off.data(), P.ms_off.size() * 4);
        put(cs, d_csoff, P.cs_off.data(), P.cs_off.size() * 4);
        put(cs, d_csm, P.cs_marker.data(), P.cs_marker.size() * 4);
        put(cs, d_num, P.num_markers.data(), P.num_markers.size() * 4);
        put(cs, d_rsoff, a->rs_off, ((size_t)R + 1) * 8);
        put(cs, d_len, P.contig_len.data(), (size_t)R * 4);
      });
      const SimDev T = {d_koff.as<uint32_t>(), d_key.as<int32_t>(), d_msoff.as<uint32_t>(), d_csoff.as<uint32_t>(), d_csm.as<uint32_t>(), d_num.as<uint32_t>(), U, S};
      for (uint32_t r0 = 0; r0 < R;) {
        const uint32_t r1 = sim::next_round(R, a->rs_off, U, S, budget_bytes, r0), nr = r1 - r0;
        const uint64_t base = a->rs_off[r0], n = a->rs_off[r1] - base;
        const auto p0 = std::chrono::steady_clock::now();
        h_starts.resize(n);
        for (uint64_t k = 0; k < n; ++k) h_starts[k] = (int32_t)a->starts[base + k];
        I.ms_pack += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - p0).count();
        if (U > sim::STAGE_COUNTS) d_scratch.ensure((size_t)nr * U * 4);
        d_out.ensure((size_t)nr * S * sim::OUT_BYTES);
        cs.timed(I.ms_upload, [&] { put(cs, d_starts, h_starts.data(), n * 4); });
        cs.timed(I.ms_kernel, [&] {
          launch_sim(cs.st, T, r0, nr, d_rsoff.as<uint64_t>(), base, d_starts.as<int32_t>(), d_len.as<int32_t>(), d_scratch.as<uint32_t>(), d_out.as<double>());
          HIPCHK(hipGetLastError());
        });
        cs.timed(I.ms_download, [&] { HIPCHK(hipMemcpyAsync(out + (size_t)r0 * S * 4, d_out.p, (size_t)nr * S * sim::OUT_BYTES, hipMemcpyDeviceToHost, cs.st)); });
        I.nrounds += 1;
        r0 = r1;
      }
    }
    I.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (info) *info = I;
  });
}
