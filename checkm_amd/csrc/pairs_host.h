// pairs_host.h -- the host driver of the count / scan / fill compaction of pairs_dev.h, behind a pass's count launch: the row scan and
// its totals, the split of the rows into output batches, then a fill launch and a download per batch.  Used by ckm_merge.hip and
// ckm_markerset.hip; the buffers live as long as the call and only grow.
#pragma once
#include <vector>
#include "ckm_host.h"
#include "pairs_dev.h"

namespace ckm {

struct PairBatches {
  DevBuf d_total, d_base, d_out;             // per row of the count pass: its pairs, the pairs of the rows before; the batch being filled
  PinnedBuf h_out;
  std::vector<uint32_t> row_total;           // what run() leaves to the caller: the pairs each row of the pass reported
  std::vector<uint64_t> row_base;
  std::vector<pc::Group> groups;

  // scan(d_total)          launches the pass's row scan over its tile counts
  // fill(group, d_out, n)  launches the pass's tile kernel over the rows of `group`, whose n pairs go to d_out
  // take(h_out, n)         receives the n pairs of a batch on the host, in order
  // The pass covers rows [row0, row0 + nrows): a group names its rows in that numbering.
  // Every phase is waited for (cs.timed): the host needs its result, or reuses its buffers, before the next one.  Returns the pairs of the pass.
  template <class Scan, class Fill, class Take>
  uint64_t run(CallStream &cs, uint32_t row0, uint32_t nrows, uint64_t cap_pairs, uint64_t pair_bytes, double &ms_scan, double &ms_fill, double &ms_download, Scan &&scan, Fill &&fill,
               Take &&take) {
    d_total.ensure((size_t)nrows * 4);
    row_total.resize(nrows); row_base.resize(nrows);
    cs.timed(ms_scan, [&] {
      scan(d_total.as<uint32_t>());
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(row_total.data(), d_total.p, (size_t)nrows * 4, hipMemcpyDeviceToHost, cs.st));
    });
    const WallClock s0;
    const uint64_t total = pc::row_prefix(row_total.data(), nrows, row_base.data());
    groups.clear();
    pc::plan_groups(row_total.data(), row0, row0 + nrows, cap_pairs, groups);
    ms_scan += s0.ms();
    if (!total) return 0;
    cs.timed(ms_scan, [&] { cs.put(d_base, row_base.data(), (size_t)nrows * 8); });
    for (const pc::Group &g : groups) {
      const uint64_t n = g.npairs;
      d_out.ensure(n * pair_bytes); h_out.ensure(n * pair_bytes);
      cs.timed(ms_fill, [&] { fill(g, d_out.p, n); HIPCHK(hipGetLastError()); });
      cs.timed(ms_download, [&] { HIPCHK(hipMemcpyAsync(h_out.p, d_out.p, n * pair_bytes, hipMemcpyDeviceToHost, cs.st)); });
      take(h_out.p, n);
    }
    return total;
  }
};

}  // namespace ckm
