// kernels_cascade.hip -- the posterior domain heuristics of the device-driven cascade, gfx950 only.
// Replaces, inside the hmmsearch process launched at checkm/hmmer.py:70, the region scan of HMMER's domain definition
// ("p7_domaindef_ByPosteriorHeuristics": rt1 0.25 / rt2 0.10 / rt3 0.20 on the begin/end/occupancy posteriors) and the hand-over
// to envelope rescoring, which the host used to do between two device phases.  One wavefront per pair that passed the Forward
// filter: it turns the three decoding terms per residue the Backward parser left in the workspace into the running sums
// btot/etot (in place: the float prefix sums are part of the decision, so they are formed once, in residue order, exactly as the
// CPU restatement forms them), finds the regions, and for every region allocates the workspace of what comes next --
//   one envelope (FbWork, full = 1)             -> envelope queue of the model's register class
//   a multi-domain region (FbWork full = 2 + EnsWork) -> region queue: multihit Forward with M, I, D rows, then the trace ensemble
// and leaves a RegionRec for the host in pinned memory.  Float compares only: no transcendental.
#include <hip/hip_runtime.h>
#include "dev_types.h"
#include "cascade_dev.h"
#include "cascade_regions.h"

namespace ckm {



// set: the Backward queues (parser items of `fwork` whose decoding terms are complete) of one register class over all groups of a
// sequence part (queue_set.h); cds: the search's CascadeDev array.  What a region becomes goes to the tables, queues and counters of the
// group its pair came from.
__global__ void __launch_bounds__(64) region_kernel(QueueSet set, const FbWork *__restrict__ fwork, const CascadeDev *__restrict__ cds,
                                                   const DevModel *__restrict__ models, float *__restrict__ ws) {
  __shared__ uint32_t qpre[QS_MAX + 1];
  const int lane = threadIdx.x;
  const uint32_t n = queue_set_prefix(WorkQueue{nullptr, nullptr, 0}, set, qpre, lane);
  for (uint32_t k = blockIdx.x; k < n; k += gridDim.x) {
    uint32_t qi;
    const uint32_t item = queue_set_item(WorkQueue{nullptr, nullptr, 0}, set, qpre, k, qi);
    const FbWork w = fwork[item];
    region_scan<false>(cds[set.group[qi]], models[w.model], w, ws, lane);
  }
}

int launch_regions(hipStream_t stream, uint32_t nblocks, const QueueSet &set, const FbWork *fwork, const CascadeDev *cds, const DevModel *models, float *ws) {
  if (!set.n || set.n > QS_MAX || !cds) return -1;
  if (nblocks) hipLaunchKernelGGL(region_kernel, dim3(nblocks), dim3(64), 0, stream, set, fwork, cds, models, ws);
  return 0;
}

}  // namespace ckm
