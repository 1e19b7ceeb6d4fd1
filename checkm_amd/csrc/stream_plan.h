// stream_plan.h -- which stream of the per-device pool every logical stream of a search context uses, by the number of hardware queues
// the process runs with.  Pure host code without HIP: ckm_search.hip builds the pool from it and tests/test_stream_plan_host.py compiles
// it alone.
//
// A context has 1 main stream (fork / join of a search, uploads), up to 14 side streams -- the first `nss` carry the SSV launches, the
// next `nch` the chains: every group's filter chain (exact MSV, bias filter, Viterbi) behind its SSV launch, and once per sequence part
// and Forward class the float stages over the queue sets of all of the part's groups (queue_set.h), the classes going round the same
// handles -- and 1 stream for the trace ensembles.  Streams that share a hardware queue run one behind the other,
// and a hipStreamWaitEvent barrier holds everything queued behind it on its queue: with more streams than queues an SSV launch sits
// behind a chain that waits for ANOTHER SSV launch, and the device runs under-filled through the SSV phase.  So
// the pool never holds more streams than the budget, and below 16 queues
//   - an SSV handle carries SSV launches only: no chain, no ensemble, no main stream (they wait on other streams' events and run
//     persistent queue kernels);
//   - the filter chains of all groups, and of all contexts, share the chain handles in launch order -- their SSV launches finish in that
//     order; a part's float stages queue on them behind the part's last filter chain, in front of the next part's;
//   - up to 4 queues every handle but the one SSV handle is a chain handle, and the main stream and the ensembles use the last of them:
//     the chain kernels are latency-bound and their serial time exceeds the SSV launches', so what counts is how many run side by
//     side (measured at 4 queues, s per 1000-bin step: SSV 1 + chain 3: 12.5; 1 + 2 + a main: 13.1; 2 + 2: 13.2; 1 + 1 + two mains:
//     18.5; chains on the SSV handles, 4 + 0: 13.3, 3 + 0 + a main: 14.2; the streams before the pool: 15.8);
//   - then the main stream gets a handle of its own (5), then the ensembles (6: tens of ms per launch, not in front of a chain), then
//     SSV and chain handles grow towards the 4 + 10 of 16 queues.  Not measured between 5 and 15.
// The contexts of a device share the pool: the main handle carries nothing that outlasts a search's SSV phase (ckm_search.hip drains the
// chains on the ensembles' stream), so a second context's search starts behind the first one's SSV launches, as the baton orders anyway.
// At 16 queues or more a context has the streams it always had (main, 14 side = 4 SSV + 10 chain, ensembles); with 32 queues two
// contexts have 16 handles each, below that they share the 16.
#pragma once
#include <cstdlib>

namespace ckm {

constexpr int kPlanContexts = 3;       // context slots a plan holds (find() keeps two contexts in flight, three at the most)
constexpr int kPlanSide = 14;          // side streams of a context at the most

struct StreamPlan {
  int budget = 16, contexts = 1;
  int nhandles = 0;                    // streams of the pool, created in handle order
  int nss = 0, nch = 0;                // side[0 .. nss): SSV handles, side[nss .. nss + nch): chain handles (nch == 0: a chain follows its SSV launch)
  int main_h[kPlanContexts] = {0, 0, 0};
  int side_h[kPlanContexts][kPlanSide] = {};
  int ens_h[kPlanContexts] = {0, 0, 0};
};

// The hardware queues the process runs with: CKM_HW_QUEUES (a host that started HIP earlier with another value says so), else
// GPU_MAX_HW_QUEUES as the runtime reads it, else the 16 the library sets when nothing is inherited.  Clamped to 1 .. 32.
inline int parse_queue_budget(const char *ckm_hw_queues, const char *gpu_max_hw_queues) {
  const char *v = (ckm_hw_queues && *ckm_hw_queues) ? ckm_hw_queues : gpu_max_hw_queues;
  if (!v || !*v) return 16;
  char *end = nullptr;
  const long n = strtol(v, &end, 10);
  if (end == v) return 16;
  return (int)(n < 1 ? 1 : n > 32 ? 32 : n);
}

// One pool shared by all context slots: nss SSV handles, nch chain handles, the ensembles' handle if they have one, nmain main handles
// (handle order = creation order).  Without a handle of their own the ensembles and the mains use the last side handle.
inline void plan_layout(StreamPlan &p, int nss, int nch, int ens_own, int nmain) {
  p.nss = nss; p.nch = nch;
  const int ns = nss + nch, h_ens = ns, h_main = h_ens + ens_own;
  p.nhandles = h_main + nmain;
  for (int c = 0; c < kPlanContexts; ++c) {
    for (int k = 0; k < kPlanSide; ++k) p.side_h[c][k] = k % ns;
    p.ens_h[c] = ens_own ? h_ens : ns - 1;
    p.main_h[c] = nmain ? h_main + c % nmain : ns - 1;
  }
}

inline StreamPlan stream_plan(int budget, int contexts_in_flight) {
  StreamPlan p;
  const int B = budget < 1 ? 1 : budget > 32 ? 32 : budget;
  const int C = contexts_in_flight < 1 ? 1 : contexts_in_flight > kPlanContexts ? kPlanContexts : contexts_in_flight;
  p.budget = B; p.contexts = C;
  if (B >= 16) {
    // a context's streams in the order they were always created: main, side[0 .. 14), ensembles
    const int nslots = B / 16 < C ? B / 16 : C;
    p.nss = 4; p.nch = 10; p.nhandles = 16 * nslots;
    for (int c = 0; c < kPlanContexts; ++c) {
      const int base = 16 * (c % nslots);
      p.main_h[c] = base;
      for (int k = 0; k < kPlanSide; ++k) p.side_h[c][k] = base + 1 + k;
      p.ens_h[c] = base + 15;
    }
    return p;
  }
  int nss = 1, nch = B <= 4 ? B - 1 : 3, nmain = 0, ens_own = 0;
  int r = B - nss - nch;
  static const char grow[] = "MECSCCCSCCS";               // budgets 5 .. 15: main, ensembles, then chain and SSV handles
  for (const char *g = grow; *g && r > 0; ++g, --r) {
    if (*g == 'M') nmain = 1; else if (*g == 'E') ens_own = 1; else if (*g == 'S') ++nss; else ++nch;
  }
  plan_layout(p, nss, nch, ens_own, nmain);
  return p;
}

}  // namespace ckm

// C entry points for the CPU test (tests/test_stream_plan_host.py compiles this header into a shim with CKM_STREAM_PLAN_SHIM defined)
#ifdef CKM_STREAM_PLAN_SHIM
extern "C" int ckm_plan_queue_budget(const char *a, const char *b) { return ckm::parse_queue_budget(a, b); }
// out: nhandles, nss, nch, then per context slot (3 of them): main, 14 side, ens  ->  3 + 3 * 16 ints
extern "C" void ckm_plan_fill(int budget, int contexts, int *out) {
  const ckm::StreamPlan p = ckm::stream_plan(budget, contexts);
  int n = 0;
  out[n++] = p.nhandles; out[n++] = p.nss; out[n++] = p.nch;
  for (int c = 0; c < ckm::kPlanContexts; ++c) {
    out[n++] = p.main_h[c];
    for (int k = 0; k < ckm::kPlanSide; ++k) out[n++] = p.side_h[c][k];
    out[n++] = p.ens_h[c];
  }
}
#endif
