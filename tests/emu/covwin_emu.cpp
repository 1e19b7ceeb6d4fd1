// covwin_emu.cpp -- TEST INFRASTRUCTURE: the device pass of CoverageWindows (checkm_amd/csrc/covwin_dev.h) and the library's BAM reader
// (bam_host.cpp) compiled by g++ against a HOST executor, so that the CPU test suite runs the record logic, the O(1) scatter into
// direct / diff, the reductions over runs inside a wavefront, the batching and the scan.  covwin_kernel is restated as loops over
// wavefronts and lanes as tests/emu/coverage_emu.cpp restates coverage_kernel; the scan keeps the three passes of kernels_covwin.hip
// (workgroup totals, an exclusive scan of the totals that carries across tiles, the workgroup scan plus its carry).  Built with
// -ffp-contract=off like the library.  Nothing in checkm_amd loads it.
#include <cstring>
#include <string>
#include <vector>
#include "../../checkm_amd/csrc/bam_host.h"
#include "../../checkm_amd/csrc/covwin_dev.h"

using namespace ckm;
using namespace ckm::cw;

namespace ckm { void set_last_error(const std::string &) {} }

namespace {

struct Accum {
  std::vector<uint64_t> counters, direct, diff;
  std::vector<int64_t> len, first;
  uint64_t slot = NO_ERROR, atomics = 0;
};

int run_end(uint64_t heads, int lane) {
  const uint64_t above = lane == WAVE - 1 ? 0 : heads & ~(((uint64_t)2 << lane) - 1);
  return above ? __builtin_ctzll(above) : WAVE;
}

// the segmented shuffle sum: sum[lane] := the sum over [lane, end[lane])
void run_sum(long long *sum, const int *end) {
  for (int d = 1; d < WAVE; d <<= 1) {
    long long up[WAVE];
    for (int lane = 0; lane < WAVE; ++lane) up[lane] = lane + d < WAVE ? sum[lane + d] : sum[lane];
    for (int lane = 0; lane < WAVE; ++lane) if (lane + d < end[lane]) sum[lane] += up[lane];
  }
}

// one wavefront of covwin_kernel
void wavefront(const uint8_t *data, const uint32_t *offsets, uint32_t nrec, uint32_t idx0, uint64_t first_ordinal, const Params &P, Accum &A) {
  RecOut o[WAVE];
  Scatter sc[WAVE];
  uint32_t g0[WAVE];
  for (int lane = 0; lane < WAVE; ++lane) {
    o[lane] = RecOut{-1, -1, 0, 0, 0};
    sc[lane] = Scatter{0, 0, 0, 0, 0};
    g0[lane] = NO_SLOT;
    const uint32_t idx = idx0 + (uint32_t)lane;
    if (idx < nrec) {
      classify(data + offsets[idx], P, o[lane]);
      if (o[lane].err) { const uint64_t v = (first_ordinal + idx) * 8u + o[lane].err; if (v < A.slot) A.slot = v; o[lane].ref = -1; }
    }
    if (o[lane].ref >= 0 && o[lane].cls == 7) {
      sc[lane] = scatter(o[lane].pos, o[lane].alen, A.len.at(o[lane].ref), P.window);
      if (sc[lane].span) g0[lane] = (uint32_t)A.first.at(o[lane].ref) + sc[lane].k0;
    }
  }
  // the nine counters over runs of equal refID
  uint64_t heads = 0, counted = 0, cls[NCLASS] = {0};
  for (int lane = 0; lane < WAVE; ++lane) {
    if (lane == 0 || o[lane - 1].ref != o[lane].ref) heads |= (uint64_t)1 << lane;
    if (o[lane].ref >= 0) { counted |= (uint64_t)1 << lane; if (o[lane].cls >= 0) cls[o[lane].cls] |= (uint64_t)1 << lane; }
  }
  int end[WAVE];
  long long sum[WAVE];
  for (int lane = 0; lane < WAVE; ++lane) { end[lane] = run_end(heads, lane); sum[lane] = (long long)sc[lane].span; }
  run_sum(sum, end);
  for (int lane = 0; lane < WAVE; ++lane) {
    if (!(heads >> lane & 1) || o[lane].ref < 0) continue;
    const uint64_t run = (end[lane] == WAVE ? ~(uint64_t)0 : (((uint64_t)1 << end[lane]) - 1)) & ~(((uint64_t)1 << lane) - 1);
    uint64_t add[NSLOT];
    add[SLOT_READS] = (uint64_t)__builtin_popcountll(counted & run);
    for (int c = 1; c < NCLASS; ++c) add[c] = (uint64_t)__builtin_popcountll(cls[c] & run);
    add[SLOT_NUMER] = (uint64_t)sum[lane];
    for (int k = 0; k < NSLOT; ++k) if (add[k]) { A.counters.at((uint64_t)o[lane].ref * NSLOT + k) += add[k]; ++A.atomics; }
  }
  // direct[k0] over runs of equal global slot
  heads = 0;
  for (int lane = 0; lane < WAVE; ++lane) if (lane == 0 || g0[lane - 1] != g0[lane]) heads |= (uint64_t)1 << lane;
  for (int lane = 0; lane < WAVE; ++lane) { end[lane] = run_end(heads, lane); sum[lane] = (long long)sc[lane].head; }
  run_sum(sum, end);
  for (int lane = 0; lane < WAVE; ++lane) {
    if ((heads >> lane & 1) && g0[lane] != NO_SLOT) { A.direct.at(g0[lane]) += (uint64_t)sum[lane]; ++A.atomics; }
    if (g0[lane] != NO_SLOT && sc[lane].k1 > sc[lane].k0) {
      const uint32_t g1 = g0[lane] + (sc[lane].k1 - sc[lane].k0);
      if (g1 >= (uint64_t)A.first.at(o[lane].ref + 1)) throw Error(CKM_EINVAL, "a read leaves its reference's slots");      // (never: e <= L)
      A.direct.at(g1) += (uint64_t)sc[lane].tail; ++A.atomics;
      if (sc[lane].k1 > sc[lane].k0 + 1) {
        A.diff.at(g0[lane] + 1) += (uint64_t)P.window;
        A.diff.at(g1) += (uint64_t)(-(long long)P.window);
        A.atomics += 2;
      }
    }
  }
}

// direct[k] += inclusive_prefix(diff)[k], in the three passes of the kernels
void scan(std::vector<uint64_t> &direct, const std::vector<uint64_t> &diff) {
  const uint64_t n = direct.size(), nb = (n + SCAN_BLOCK - 1) / SCAN_BLOCK;
  std::vector<long long> sums(nb, 0);
  for (uint64_t b = 0; b < nb; ++b)
    for (uint64_t k = b * SCAN_BLOCK; k < n && k < (b + 1) * SCAN_BLOCK; ++k) sums[b] += (long long)diff[k];
  long long carry = 0;
  for (uint64_t t0 = 0; t0 < nb; t0 += SCAN_THREADS) {
    long long total = 0;
    for (uint64_t i = t0; i < nb && i < t0 + SCAN_THREADS; ++i) { const long long v = sums[i]; sums[i] = carry + total; total += v; }
    carry += total;
  }
  for (uint64_t b = 0; b < nb; ++b) {
    long long run = sums[b];
    for (uint64_t k = b * SCAN_BLOCK; k < n && k < (b + 1) * SCAN_BLOCK; ++k) { run += (long long)diff[k]; direct[k] += (uint64_t)run; }
  }
}

void copy_text(const std::string &s, char *to, uint32_t cap) { if (cap) { strncpy(to, s.c_str(), cap - 1); to[cap - 1] = 0; } }

}  // namespace

// ckm_coverage_windows_run without a device.  out: [n_ref * 9]; first: [n_ref + 1]; sums: [cap_slots]; info: records, batches, atomic
// adds, error slot, slots.  0, or -1 with the reader's message (or the refusal of the arguments) in why, or -2 when the error slot is
// set (info[3] = ordinal * 8 + reason, why = the read's name).
extern "C" int emu_covwin(const char *path, double min_align_per, double max_edit_dist_per, int all_reads, int64_t window, uint64_t budget, int threads,
                          int64_t *out, uint64_t cap_refs, int64_t *first, int64_t *sums, uint64_t cap_slots, uint64_t *info, char *why, uint32_t cap) {
  try {
    info[0] = info[1] = info[2] = info[4] = 0; info[3] = NO_ERROR;
    if (min_align_per != min_align_per || max_edit_dist_per != max_edit_dist_per) { copy_text("a coverage threshold is not a number", why, cap); return -1; }
    if (window < 1 || window > MAX_WINDOW) { copy_text("the window size must be between 1 and 2^31 - 1", why, cap); return -1; }
    HostPool pool(threads);
    bam::Reader rd(path, &pool);
    const uint64_t n_ref = rd.ref_names().size();
    if (n_ref > cap_refs) { copy_text("more references than the caller allowed for", why, cap); return -1; }
    Accum A;
    A.len = rd.ref_lengths();
    A.first.assign(n_ref + 1, 0);
    for (uint64_t k = 0; k < n_ref; ++k) {
      A.first[k + 1] = A.first[k] + slots_of(A.len[k], window);
      if (A.first[k + 1] > MAX_SLOTS) { copy_text("more than 2^31 - 1 windows", why, cap); return -1; }
    }
    const uint64_t nslots = (uint64_t)A.first[n_ref];
    if (nslots > cap_slots) { copy_text("more windows than the caller allowed for", why, cap); return -1; }
    const Params P = {min_align_per, max_edit_dist_per, all_reads ? 1 : 0, (int32_t)n_ref, (uint32_t)window};
    A.counters.assign(n_ref * NSLOT, 0); A.direct.assign(nslots, 0); A.diff.assign(nslots, 0);
    info[4] = nslots;
    bam::Batch bt;
    budget = bam::batch_budget(budget);
    while (rd.next(budget, bt)) {
      const uint32_t nrec = (uint32_t)bt.offsets.size();
      std::vector<uint8_t> dev(bt.data, bt.data + bt.bytes);            // the bytes the device gets: nothing beyond them may be read
      for (uint32_t idx0 = 0; idx0 < (nrec + 255) / 256 * 256; idx0 += WAVE) wavefront(dev.data(), bt.offsets.data(), nrec, idx0, bt.first_ordinal, P, A);
      info[0] += nrec; info[1] += 1; info[2] = A.atomics;
      if (A.slot != NO_ERROR) {
        const uint8_t *rec = bt.data + bt.offsets[(A.slot >> 3) - bt.first_ordinal];
        copy_text(std::string(reinterpret_cast<const char *>(rec + FIXED), rec[12] ? rec[12] - 1 : 0), why, cap);
        info[3] = A.slot;
        return -2;
      }
    }
    for (uint64_t k = 0; k < n_ref; ++k) {                               // every reference's diff nets to zero: the scan needs no segment flags
      long long net = 0;
      for (int64_t s = A.first[k]; s < A.first[k + 1]; ++s) net += (long long)A.diff[s];
      if (net) { copy_text("the difference array of a reference does not net to zero", why, cap); return -1; }
    }
    scan(A.direct, A.diff);
    for (uint64_t k = 0; k < n_ref * NSLOT; ++k) out[k] = (int64_t)A.counters[k];
    for (uint64_t k = 0; k <= n_ref; ++k) first[k] = A.first[k];
    for (uint64_t k = 0; k < nslots; ++k) sums[k] = (int64_t)A.direct[k];
    return 0;
  } catch (const std::exception &e) {
    copy_text(e.what(), why, cap);
    return -1;
  }
}
