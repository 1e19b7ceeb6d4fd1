// ckm_sim.hip -- C ABI of the marker-set simulation on the device (kernels_sim.hip): the keys and the marker sets of a call go up once,
// the replicates in rounds of whole replicates whose starts, output rows and scratch rows fit the byte budget, one launch per round.  A
// round's results land in the caller's array at the round's first replicate, so no result depends on the budget.
#include <string>
#include <vector>
#include "ckm_host.h"
#include "sim_dev.h"

namespace ckm {
void launch_sim(hipStream_t st, const sim::SimDev &T, uint32_t r0, uint32_t nr, const uint64_t *rs_off, uint64_t start_base, const int32_t *starts, const int32_t *contig_len,
                uint32_t *scratch, double *out);
int sim_check_args(const ckm_sim_args *a, std::string &why);
}  // namespace ckm
using namespace ckm;

extern "C" int ckm_sim_run(ckm_ctx *ctx, const ckm_sim_args *a, uint64_t budget_bytes, double *out, ckm_sim_info *info) {
  CallStream cs;
  return guarded([&] {
    if (!ctx || !a) throw Error(CKM_EINVAL, "NULL argument");
    std::string why;
    refuse(sim_check_args(a, why), why);
    const uint32_t R = a->nreplicates, S = a->nsets, U = a->nmarkers;
    if (R && S && !out) throw Error(CKM_EINVAL, "NULL argument");
    const WallClock t0;
    budget_bytes = batch_budget(budget_bytes, "CKM_SIM_BATCH_MB", 256);
    ckm_sim_info I = {};
    if (R && S) {
      const sim::Args A = {U, a->key_off, a->key, S, a->ms_off, a->cs_off, a->cs_marker, R, a->rs_off, a->starts, a->contig_len};
      sim::Packed P;
      sim::pack(A, P);
      std::vector<int32_t> h_starts;
      I.ms_pack = t0.ms();
      cs.open(ctx->device);
      DevBuf d_koff, d_key, d_rsoff, d_len, d_starts, d_scratch, d_out;
      SetsBufs d_sets;
      cs.timed(I.ms_upload, [&] {
        cs.put(d_koff, P.key_off.data(), P.key_off.size() * 4);
        cs.put(d_key, P.key.data(), P.key.size() * 4);
        d_sets.upload(cs, P);
        cs.put(d_rsoff, a->rs_off, ((size_t)R + 1) * 8);
        cs.put(d_len, P.contig_len.data(), (size_t)R * 4);
      });
      const sim::SimDev T = {d_koff.as<uint32_t>(), d_key.as<int32_t>(), d_sets.dev(), U};
      for (uint32_t r0 = 0; r0 < R;) {
        const uint32_t r1 = sim::next_round(R, a->rs_off, U, S, budget_bytes, r0), nr = r1 - r0;
        const uint64_t base = a->rs_off[r0], n = a->rs_off[r1] - base;
        const WallClock p0;
        h_starts.resize(n);
        for (uint64_t k = 0; k < n; ++k) h_starts[k] = (int32_t)a->starts[base + k];
        I.ms_pack += p0.ms();
        if (U > sim::STAGE_COUNTS) d_scratch.ensure((size_t)nr * U * 4);
        d_out.ensure((size_t)nr * S * sim::OUT_BYTES);
        cs.timed(I.ms_upload, [&] { cs.put(d_starts, h_starts.data(), n * 4); });
        cs.timed(I.ms_kernel, [&] {
          launch_sim(cs.st, T, r0, nr, d_rsoff.as<uint64_t>(), base, d_starts.as<int32_t>(), d_len.as<int32_t>(), d_scratch.as<uint32_t>(), d_out.as<double>());
          HIPCHK(hipGetLastError());
        });
        cs.timed(I.ms_download, [&] { HIPCHK(hipMemcpyAsync(out + (size_t)r0 * S * 4, d_out.p, (size_t)nr * S * sim::OUT_BYTES, hipMemcpyDeviceToHost, cs.st)); });
        I.nrounds += 1;
        r0 = r1;
      }
    }
    I.ms_total = t0.ms();
    if (info) *info = I;
  });
}
