// queue_set.h -- a launch over SEVERAL work queues at once: the float stages of the device-driven cascade (parser Forward / Backward,
// regions, envelope Forward / Backward / OA, region Forward) run once per sequence part and Forward register class over the queues of
// all of the part's groups, instead of once per group.  The wavefronts of such a launch stride over FLAT item numbers 0 .. total: the
// concatenation of the queues' entries, each queue clamped to its capacity.  This header is the index arithmetic alone -- no HIP, no
// I/O -- compiled for the host (tests/native/queue_set_check.cpp) and for the device (cascade_dev.h forms the prefix by a wavefront
// scan and calls qs_locate).
#pragma once
#include <cstdint>
#include "dev_types.h"

#if defined(__HIPCC__)
#define CKM_QS_HD __host__ __device__
#else
#define CKM_QS_HD
#endif

namespace ckm {

constexpr uint32_t QS_MAX = 192;      // queues per set: at most one per group of the search (cascade_plan.h: kMaxGroups)

// queues[i] belongs to group group[i] (index into the search's CascadeDev array).  n == 0: no set -- the launch has its one queue.
struct QueueSet { const WorkQueue *queues; const uint32_t *group; uint32_t n; };

// entries of a queue that exist: a producer that found the queue full still counted
CKM_QS_HD inline uint32_t qs_clamp(uint32_t count, uint32_t cap) { return count < cap ? count : cap; }

// pre[0] = 0, pre[i + 1] = pre[i] + min(count[i], cap[i]): n + 1 entries; returns the total.  (The tables of a search hold fewer than
// 2^32 entries together, so the sums do not wrap.)
CKM_QS_HD inline uint32_t qs_prefix(const uint32_t *count, const uint32_t *cap, uint32_t n, uint32_t *pre) {
  uint32_t acc = 0;
  pre[0] = 0;
  for (uint32_t i = 0; i < n; ++i) { acc += qs_clamp(count[i], cap[i]); pre[i + 1] = acc; }
  return acc;
}

// Flat item k -> (queue, position in it): the queue q with pre[q] <= k < pre[q + 1] (never an empty one), by binary search.  False
// when k is not an item (k >= pre[n]); queue and pos are then left alone.
CKM_QS_HD inline bool qs_locate(const uint32_t *pre, uint32_t n, uint32_t k, uint32_t &queue, uint32_t &pos) {
  if (n == 0 || k >= pre[n]) return false;
  uint32_t lo = 0, hi = n;              // pre[lo] <= k < pre[hi]
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (pre[mid] <= k) lo = mid; else hi = mid;
  }
  queue = lo; pos = k - pre[lo];
  return true;
}

}  // namespace ckm
