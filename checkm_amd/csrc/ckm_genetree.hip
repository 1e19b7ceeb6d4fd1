// ckm_genetree.hip -- C ABI of the gene-tree tests on the device (kernels_genetree.hip): the offset arrays of the forest go up once; the
// trees are cut into rounds whose nodes, leaves, classes, pairs and groups fit the byte budget (genetree::round_end, the host executor's
// cut).  A round's arrays go up, three launches score it on the call's stream, and its results come back at the round's first class,
// pair and group in the caller's arrays, so no result depends on the budget.
#include <string>
#include <vector>
#include "ckm_host.h"
#include "genetree_dev.h"

namespace ckm {
uint32_t launch_gn_round(hipStream_t st, const genetree::Round &R, int what);
genetree::Args genetree_args_of(const ckm_genetree_args *a);
int genetree_check_args(const ckm_genetree_args *a, std::string &why);
int genetree_check_out(const ckm_genetree_args *a, const ckm_genetree_out *out, std::string &why);
}  // namespace ckm
using namespace ckm;

extern "C" int ckm_genetree_run(ckm_ctx *ctx, const ckm_genetree_args *a, uint64_t budget_bytes, const ckm_genetree_out *out, ckm_genetree_info *info) {
  CallStream cs;
  return guarded([&] {
    if (!ctx || !a || !out) throw Error(CKM_EINVAL, "NULL argument");
    std::string why;
    refuse(genetree_check_args(a, why), why);
    refuse(genetree_check_out(a, out, why), why);
    const WallClock t0;
    budget_bytes = batch_budget(budget_bytes, "CKM_GENETREE_BATCH_MB", 256);
    const genetree::Args A = genetree_args_of(a);
    const uint32_t T = A.ntrees;
    ckm_genetree_info I = {};
    I.ntrees = T;
    if (T) {
      const uint64_t NL = A.leaf_off[T], NG = A.group_off[T];
      cs.open(ctx->device);
      DevBuf d_noff, d_loff, d_coff, d_goff, d_poff, d_first, d_last, d_parent, d_len, d_int, d_lnode, d_species, d_lclass, d_total, d_pa, d_pb, d_cons, d_flag, d_gnode, d_gmixed;
      cs.timed(I.ms_upload, [&] {
        cs.put(d_noff, A.node_off, (uint64_t)(T + 1) * 4);
        cs.put(d_loff, A.leaf_off, (uint64_t)(T + 1) * 4);
        cs.put(d_coff, A.class_off, (3 * (uint64_t)T + 1) * 4);
        cs.put(d_goff, A.group_off, (uint64_t)(T + 1) * 4);
        cs.put(d_poff, A.gpair_off, (NG + 1) * 4);
      });
      std::vector<uint32_t> leaf_node;
      for (uint32_t ta = 0; ta < T;) {
        const uint32_t tb = genetree::round_end(A, ta, budget_bytes);
        genetree::Round R = {};
        R.t0 = ta; R.t1 = tb;
        R.node0 = A.node_off[ta]; R.leaf0 = A.leaf_off[ta]; R.class0 = A.class_off[3 * (uint64_t)ta]; R.group0 = A.group_off[ta]; R.pair0 = A.gpair_off[R.group0];
        const uint64_t nn = A.node_off[tb] - R.node0;
        R.nleaves = A.leaf_off[tb] - R.leaf0; R.nclasses = A.class_off[3 * (uint64_t)tb] - R.class0; R.ngroups = A.group_off[tb] - R.group0;
        R.npairs = A.gpair_off[A.group_off[tb]] - R.pair0;
        genetree::leaf_nodes_of(A, ta, tb, leaf_node);
        d_cons.ensure((uint64_t)R.nclasses * 8); d_flag.ensure(R.npairs); d_gnode.ensure((uint64_t)R.ngroups * 4); d_gmixed.ensure(R.ngroups);
        d_lclass.ensure((uint64_t)R.nleaves * 4 * genetree::RANKS);
        cs.timed(I.ms_upload, [&] {
          cs.put(d_first, A.first + R.node0, nn * 4);
          cs.put(d_last, A.last + R.node0, nn * 4);
          cs.put(d_parent, A.parent + R.node0, nn * 4);
          cs.put(d_len, A.length + R.node0, nn * 8);
          cs.put(d_int, A.internal + R.node0, nn);
          cs.put(d_lnode, leaf_node.data(), (uint64_t)R.nleaves * 4);
          cs.put(d_species, A.leaf_species + R.leaf0, (uint64_t)R.nleaves * 4);
          for (int r = 0; r < genetree::RANKS; ++r)
            HIPCHK(hipMemcpyAsync(d_lclass.as<uint32_t>() + (uint64_t)r * R.nleaves, A.leaf_class + (uint64_t)r * NL + R.leaf0, (uint64_t)R.nleaves * 4, hipMemcpyHostToDevice, cs.st));
          cs.put(d_total, A.class_total + R.class0, (uint64_t)R.nclasses * 4);
          cs.put(d_pa, A.pair_a + R.pair0, (uint64_t)R.npairs * 4);
          cs.put(d_pb, A.pair_b + R.pair0, (uint64_t)R.npairs * 4);
        });
        R.node_off = d_noff.as<uint32_t>(); R.leaf_off = d_loff.as<uint32_t>(); R.class_off = d_coff.as<uint32_t>(); R.group_off = d_goff.as<uint32_t>(); R.gpair_off = d_poff.as<uint32_t>();
        R.first = d_first.as<uint32_t>(); R.last = d_last.as<uint32_t>(); R.parent = d_parent.as<uint32_t>(); R.length = d_len.as<double>(); R.internal = d_int.as<uint8_t>();
        R.leaf_node = d_lnode.as<uint32_t>(); R.species = d_species.as<uint32_t>(); R.leaf_class = d_lclass.as<uint32_t>(); R.class_total = d_total.as<uint32_t>();
        R.pair_a = d_pa.as<uint32_t>(); R.pair_b = d_pb.as<uint32_t>();
        R.consistency = d_cons.as<double>(); R.pair_flag = d_flag.as<uint8_t>(); R.group_node = d_gnode.as<uint32_t>(); R.group_mixed = d_gmixed.as<uint8_t>();
        cs.timed(I.ms_consistency, [&] { I.launches += launch_gn_round(cs.st, R, 0); HIPCHK(hipGetLastError()); });
        cs.timed(I.ms_flags, [&] { I.launches += launch_gn_round(cs.st, R, 1); HIPCHK(hipGetLastError()); });
        cs.timed(I.ms_conspecific, [&] { I.launches += launch_gn_round(cs.st, R, 2); HIPCHK(hipGetLastError()); });
        cs.timed(I.ms_download, [&] {
          if (R.nclasses) HIPCHK(hipMemcpyAsync(out->consistency + R.class0, d_cons.p, (uint64_t)R.nclasses * 8, hipMemcpyDeviceToHost, cs.st));
          if (R.npairs) HIPCHK(hipMemcpyAsync(out->pair_flag + R.pair0, d_flag.p, R.npairs, hipMemcpyDeviceToHost, cs.st));
          if (R.ngroups) {
            HIPCHK(hipMemcpyAsync(out->group_node + R.group0, d_gnode.p, (uint64_t)R.ngroups * 4, hipMemcpyDeviceToHost, cs.st));
            HIPCHK(hipMemcpyAsync(out->group_mixed + R.group0, d_gmixed.p, R.ngroups, hipMemcpyDeviceToHost, cs.st));
          }
        });
        I.nrounds += 1;
        ta = tb;
      }
      HIPCHK(hipStreamSynchronize(cs.st));
    }
    I.ms_total = t0.ms();
    if (info) *info = I;
  });
}
