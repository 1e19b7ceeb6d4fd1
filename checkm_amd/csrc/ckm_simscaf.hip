// ckm_simscaf.hip -- C ABI of the scaffold simulation on the device (kernels_simscaf.hip): the resident tables and the marker sets of a
// call go up once, the replicates in rounds of whole replicates whose bit rows, output rows and scratch rows fit the byte budget, one launch
// per round.  A round's results land in the caller's array at the round's first replicate, so no result depends on the budget.
#include <string>
#include <vector>
#include "ckm_host.h"
#include "simscaf_dev.h"

namespace ckm {
void launch_simscaf(hipStream_t st, const simscaf::SimScafDev &T, uint32_t r0, uint32_t nr, const uint32_t *test, const uint32_t *cont, const uint64_t *bit_off, uint64_t bit_base,
                    const uint32_t *bits, uint32_t *scratch, double *out);
int simscaf_check_args(const ckm_simscaf_args *a, std::string &why);
}  // namespace ckm
using namespace ckm;

extern "C" int ckm_simscaf_run(ckm_ctx *ctx, const ckm_simscaf_args *a, uint64_t budget_bytes, double *out, ckm_simscaf_info *info) {
  CallStream cs;
  return guarded([&] {
    if (!ctx || !a) throw Error(CKM_EINVAL, "NULL argument");
    std::string why;
    refuse(simscaf_check_args(a, why), why);
    const uint32_t R = a->nreplicates, S = a->nsets, U = a->nmarkers, G = a->ngenomes;
    if (R && S && !out) throw Error(CKM_EINVAL, "NULL argument");
    const WallClock t0;
    budget_bytes = batch_budget(budget_bytes, "CKM_SIMSCAF_BATCH_MB", 256);
    ckm_simscaf_info I = {};
    if (R && S) {
      const simscaf::Args A = {G, a->nscaf, U, a->sc_off, a->sc, S, a->ms_off, a->cs_off, a->cs_marker, R, a->test, a->cont, a->bit_off, a->bits};
      simscaf::Packed P;
      simscaf::pack(A, P);
      I.ms_pack = t0.ms();
      cs.open(ctx->device);
      DevBuf d_nscaf, d_scoff, d_sc, d_test, d_cont, d_bitoff, d_bits, d_scratch, d_out;
      SetsBufs d_sets;
      cs.timed(I.ms_upload, [&] {
        cs.put(d_nscaf, a->nscaf, (size_t)G * 4);
        cs.put(d_scoff, P.sc_off.data(), P.sc_off.size() * 4);
        cs.put(d_sc, a->sc, (size_t)P.sc_off.back() * 4);
        d_sets.upload(cs, P.sets);
        cs.put(d_test, a->test, (size_t)R * 4);
        cs.put(d_cont, a->cont, (size_t)R * 4);
        cs.put(d_bitoff, a->bit_off, ((size_t)R + 1) * 8);
      });
      const simscaf::SimScafDev T = {d_nscaf.as<uint32_t>(), d_scoff.as<uint32_t>(), d_sc.as<uint32_t>(), d_sets.dev(), U};
      for (uint32_t r0 = 0; r0 < R;) {
        const uint32_t r1 = simscaf::next_round(R, a->bit_off, U, S, budget_bytes, r0), nr = r1 - r0;
        const uint64_t base = a->bit_off[r0], n = a->bit_off[r1] - base;
        if (U > simscaf::STAGE_COUNTS) d_scratch.ensure((size_t)nr * U * 4);
        d_out.ensure((size_t)nr * S * simscaf::OUT_BYTES);
        cs.timed(I.ms_upload, [&] { cs.put(d_bits, n ? a->bits + base : nullptr, n * 4); });
        cs.timed(I.ms_kernel, [&] {
          launch_simscaf(cs.st, T, r0, nr, d_test.as<uint32_t>(), d_cont.as<uint32_t>(), d_bitoff.as<uint64_t>(), base, d_bits.as<uint32_t>(), d_scratch.as<uint32_t>(),
                         d_out.as<double>());
          HIPCHK(hipGetLastError());
        });
        cs.timed(I.ms_download, [&] { HIPCHK(hipMemcpyAsync(out + (size_t)r0 * S * 4, d_out.p, (size_t)nr * S * simscaf::OUT_BYTES, hipMemcpyDeviceToHost, cs.st)); });
        I.nrounds += 1;
        r0 = r1;
      }
    }
    I.ms_total = t0.ms();
    if (info) *info = I;
  });
}
