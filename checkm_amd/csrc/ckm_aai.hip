// ckm_aai.hip -- C ABI of the all-pairs amino-acid identity of AminoAcidIdentity.run (kernels_aai.hip): the rows of every group in; per
// pair, in the reference's order, the mismatches, the compared columns and the identity out.  The group table and pair_off go up once;
// the packed text and the outputs travel in batches of a byte budget, so the memory of a call on the device does not grow with n^2.
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>
#include "ckm_host.h"
#include "aai_dev.h"

namespace ckm {
void launch_aai_pairs(hipStream_t st, const uint8_t *text, uint64_t text_lo, const aai::Group *groups, const uint64_t *pair_off, uint32_t g_lo, uint32_t g_hi, uint64_t p0,
                      uint32_t npairs, int32_t *out_mis, int32_t *out_cmp, double *out_aai);
}  // namespace ckm
using namespace ckm;

struct ckm_aai {
  uint64_t ngroups = 0, npairs = 0, nbatches = 0, bytes = 0;
  std::vector<uint64_t> pair_off;
  std::vector<int32_t> mismatches, compared;
  std::vector<double> identity;
  double ms_pack = 0, ms_upload = 0, ms_kernel = 0, ms_download = 0, ms_total = 0;
};

extern "C" int ckm_aai_run(ckm_ctx *ctx, uint32_t ngroups, const uint64_t *group_row_off, const uint64_t *row_off, const char *text, uint64_t budget_bytes, ckm_aai **out) {
  CallStream cs;
  return guarded([&] {
    if (!ctx || !out) throw Error(CKM_EINVAL, "NULL argument");
    *out = nullptr;
    std::string why;
    refuse(aai::check_args(ngroups, group_row_off, row_off, text, why), why);
    budget_bytes = batch_budget(budget_bytes, "CKM_AAI_BATCH_MB", 64);
    const WallClock t0;
    std::unique_ptr<ckm_aai> o(new ckm_aai());
    aai::Packed P;
    aai::pack(ngroups, group_row_off, row_off, text, P);
    o->ms_pack = t0.ms();
    o->ngroups = ngroups; o->npairs = P.pair_off[ngroups];
    o->mismatches.resize(o->npairs); o->compared.resize(o->npairs); o->identity.resize(o->npairs);
    if (o->npairs) {
      cs.open(ctx->device);
      DevBuf d_groups, d_off, d_text, d_out;
      PinnedBuf h_out;
      cs.timed(o->ms_upload, [&] {
        cs.put(d_groups, P.groups.data(), (size_t)ngroups * sizeof(aai::Group));
        cs.put(d_off, P.pair_off.data(), ((size_t)ngroups + 1) * 8);
      });
      aai::Batch B;
      uint64_t cursor = 0;
      while (aai::next_batch(P, budget_bytes, cursor, B)) {
        if (B.npairs > 0x7FFFFFF0ull) throw Error(CKM_ERANGE, "too many pairs in one batch: use a smaller budget");
        const uint32_t np = (uint32_t)B.npairs;
        // every chunk the kernel loads lies inside the batch's text: the rows of its groups end at or before text_lo + text_bytes
        if (B.g_hi > ngroups || B.g_lo >= B.g_hi || B.text_lo + B.text_bytes > P.text.size() || B.p0 < P.pair_off[B.g_lo] || B.p0 + B.npairs > P.pair_off[B.g_hi])
          throw Error(CKM_EINVAL, "internal: a batch leaves its groups");
        for (uint32_t g = B.g_lo; g < B.g_hi; ++g)
          if (P.groups[g].n > 1 && (P.groups[g].text_off < B.text_lo || P.groups[g].text_off + aai::group_bytes(P.groups[g]) > B.text_lo + B.text_bytes))
            throw Error(CKM_EINVAL, "internal: a group leaves its batch");
        // the outputs of a batch in one buffer: identity (8-byte values) first, then the two counts
        d_out.ensure((size_t)np * aai::PAIR_BYTES); h_out.ensure((size_t)np * aai::PAIR_BYTES);
        double *da = d_out.as<double>();
        int32_t *dm = reinterpret_cast<int32_t *>(da + np), *dc = dm + np;
        cs.mark(0);
        cs.put(d_text, P.text.data() + B.text_lo, B.text_bytes);
        cs.mark(1);
        launch_aai_pairs(cs.st, d_text.as<uint8_t>(), B.text_lo, d_groups.as<aai::Group>(), d_off.as<uint64_t>(), B.g_lo, B.g_hi, B.p0, np, dm, dc, da);
        HIPCHK(hipGetLastError());
        cs.mark(2);
        HIPCHK(hipMemcpyAsync(h_out.p, d_out.p, (size_t)np * aai::PAIR_BYTES, hipMemcpyDeviceToHost, cs.st));
        cs.mark(3);
        HIPCHK(hipStreamSynchronize(cs.st));                        // the next batch reuses the text and both output buffers
        o->ms_upload += cs.ms(0, 1);
        o->ms_kernel += cs.ms(1, 2);
        o->ms_download += cs.ms(2, 3);
        const double *ha = h_out.as<double>();
        const int32_t *hm = reinterpret_cast<const int32_t *>(ha + np), *hc = hm + np;
        memcpy(o->identity.data() + B.p0, ha, (size_t)np * 8);
        memcpy(o->mismatches.data() + B.p0, hm, (size_t)np * 4);
        memcpy(o->compared.data() + B.p0, hc, (size_t)np * 4);
        o->nbatches += 1; o->bytes += B.text_bytes;
      }
    }
    o->pair_off.swap(P.pair_off);
    o->ms_total = t0.ms();
    *out = o.release();
  });
}

extern "C" int ckm_aai_columns_get(const ckm_aai *r, ckm_aai_columns *c) {
  if (!r || !c) { set_last_error("NULL argument"); return CKM_EINVAL; }
  c->ngroups = r->ngroups; c->npairs = r->npairs; c->nbatches = r->nbatches; c->bytes = r->bytes;
  c->pair_off = r->pair_off.data();
  c->mismatches = r->mismatches.data(); c->compared = r->compared.data(); c->aai = r->identity.data();
  c->ms_pack = r->ms_pack; c->ms_upload = r->ms_upload; c->ms_kernel = r->ms_kernel; c->ms_download = r->ms_download; c->ms_total = r->ms_total;
  return CKM_OK;
}

extern "C" void ckm_aai_free(ckm_aai *r) { delete r; }
