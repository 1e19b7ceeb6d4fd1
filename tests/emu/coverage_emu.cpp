// coverage_emu.cpp -- TEST INFRASTRUCTURE: the device pass of `checkm coverage` (checkm_amd/csrc/coverage_dev.h) and the library's BAM
// reader (bam_host.cpp) compiled by g++ against a HOST executor, so that the CPU test suite runs the record logic, the reduction over
// runs of equal refID and the batching of the library.  coverage_kernel is restated as loops over wavefronts and lanes: a ballot is a
// 64-bit word built lane by lane, a shuffle reads the other lane's value of the step before.  Built with -ffp-contract=off like the
// library.  Nothing in checkm_amd loads this.
#include <cstring>
#include <string>
#include <vector>
#include "../../checkm_amd/csrc/bam_host.h"
#include "../../checkm_amd/csrc/coverage_dev.h"

using namespace ckm;
using namespace ckm::cv;

namespace ckm { void set_last_error(const std::string &) {} }

namespace {

inline int popc(uint64_t x) { return __builtin_popcountll(x); }

// one wavefront of coverage_kernel; returns the atomic adds it issued
uint64_t wavefront(const uint8_t *data, const uint32_t *offsets, uint32_t nrec, uint32_t idx0, uint64_t first_ordinal, const Params &P, uint64_t *counters, uint64_t *err_slot) {
  RecOut o[WAVE];
  for (int lane = 0; lane < WAVE; ++lane) {
    o[lane] = RecOut{-1, -1, 0, 0};
    const uint32_t idx = idx0 + (uint32_t)lane;
    if (idx < nrec) {
      classify(data + offsets[idx], P, o[lane]);
      if (o[lane].err) { const uint64_t v = (first_ordinal + idx) * 8u + o[lane].err; if (v < *err_slot) *err_slot = v; o[lane].ref = -1; }
    }
  }
  uint64_t heads = 0, counted = 0, cls[NCLASS] = {0};
  for (int lane = 0; lane < WAVE; ++lane) {
    if (lane == 0 || o[lane - 1].ref != o[lane].ref) heads |= (uint64_t)1 << lane;
    if (o[lane].ref >= 0) { counted |= (uint64_t)1 << lane; if (o[lane].cls >= 0) cls[o[lane].cls] |= (uint64_t)1 << lane; }
  }
  int end[WAVE];
  for (int lane = 0; lane < WAVE; ++lane) {
    const uint64_t above = lane == WAVE - 1 ? 0 : heads & ~(((uint64_t)2 << lane) - 1);
    end[lane] = above ? __builtin_ctzll(above) : WAVE;
  }
  long long sum[WAVE];
  for (int lane = 0; lane < WAVE; ++lane) sum[lane] = o[lane].ref >= 0 && o[lane].cls == 7 ? (long long)o[lane].alen : 0;
  for (int d = 1; d < WAVE; d <<= 1) {
    long long up[WAVE];
    for (int lane = 0; lane < WAVE; ++lane) up[lane] = lane + d < WAVE ? sum[lane + d] : sum[lane];
    for (int lane = 0; lane < WAVE; ++lane) if (lane + d < end[lane]) sum[lane] += up[lane];
  }
  uint64_t atomics = 0;
  for (int lane = 0; lane < WAVE; ++lane) {
    if (!(heads >> lane & 1) || o[lane].ref < 0) continue;
    const uint64_t run = (end[lane] == WAVE ? ~(uint64_t)0 : (((uint64_t)1 << end[lane]) - 1)) & ~(((uint64_t)1 << lane) - 1);
    uint64_t add[NSLOT];
    add[SLOT_READS] = (uint64_t)popc(counted & run);
    for (int c = 1; c < NCLASS; ++c) add[c] = (uint64_t)popc(cls[c] & run);
    add[SLOT_NUMER] = (uint64_t)sum[lane];
    for (int k = 0; k < NSLOT; ++k) if (add[k]) { counters[(uint64_t)o[lane].ref * NSLOT + k] += add[k]; ++atomics; }
  }
  return atomics;
}

void copy_text(const std::string &s, char *to, uint32_t cap) { if (cap) { strncpy(to, s.c_str(), cap - 1); to[cap - 1] = 0; } }

}  // namespace

// ckm_coverage_run without a device.  out: [n_ref * 9]; info: records, batches, atomic adds, error slot.  0, or -1 with the reader's
// message in why, or -2 when the error slot is set (info[3] = ordinal * 8 + reason, why = the read's name).
extern "C" int emu_coverage(const char *path, double min_align_per, double max_edit_dist_per, double min_qc, int all_reads, uint64_t budget, int threads,
                            int64_t *out, uint64_t cap_refs, uint64_t *info, char *why, uint32_t cap) {
  try {
    HostPool pool(threads);
    bam::Reader rd(path, &pool);
    const uint64_t n_ref = rd.ref_names().size();
    if (n_ref > cap_refs) { copy_text("more references than the caller allowed for", why, cap); return -1; }
    const Params P = {min_align_per, max_edit_dist_per, min_qc, all_reads ? 1 : 0, (int32_t)n_ref};
    std::vector<uint64_t> counters(n_ref * NSLOT + 1, 0);
    uint64_t slot = NO_ERROR;
    info[0] = info[1] = info[2] = 0; info[3] = NO_ERROR;
    bam::Batch bt;
    budget = bam::batch_budget(budget);
    while (rd.next(budget, bt)) {
      const uint32_t nrec = (uint32_t)bt.offsets.size();
      std::vector<uint8_t> dev(bt.data, bt.data + bt.bytes);            // the bytes the device gets: nothing beyond them may be read
      for (uint32_t idx0 = 0; idx0 < (nrec + 255) / 256 * 256; idx0 += WAVE)
        info[2] += wavefront(dev.data(), bt.offsets.data(), nrec, idx0, bt.first_ordinal, P, counters.data(), &slot);
      info[0] += nrec; info[1] += 1;
      if (slot != NO_ERROR) {
        const uint8_t *rec = bt.data + bt.offsets[(slot >> 3) - bt.first_ordinal];
        copy_text(std::string(reinterpret_cast<const char *>(rec + FIXED), rec[12] ? rec[12] - 1 : 0), why, cap);
        info[3] = slot;
        return -2;
      }
    }
    for (uint64_t k = 0; k < n_ref * NSLOT; ++k) out[k] = (int64_t)counters[k];
    return 0;
  } catch (const std::exception &e) {
    copy_text(e.what(), why, cap);
    return -1;
  }
}

// header and record offsets by the library's reader: names joined by '\n' into names (cap_names bytes), lengths[cap_refs], offsets[cap_off]
extern "C" int emu_bam_scan(const char *path, uint64_t budget, int threads, char *names, uint32_t cap_names, int64_t *lengths, uint64_t cap_refs, uint64_t *offsets, uint64_t cap_off,
                            uint64_t *info /* n_ref, records, batches, header bytes */, char *why, uint32_t cap) {
  try {
    HostPool pool(threads);
    bam::Reader rd(path, &pool);
    std::string joined;
    for (size_t k = 0; k < rd.ref_names().size(); ++k) { joined += rd.ref_names()[k]; joined += '\n'; if (k < cap_refs) lengths[k] = rd.ref_lengths()[k]; }
    copy_text(joined, names, cap_names);
    info[0] = rd.ref_names().size(); info[3] = rd.header_bytes();
    uint64_t base = rd.header_bytes(), n = 0, nb = 0;
    bam::Batch bt;
    while (rd.next(budget ? budget : bam::batch_budget(0), bt)) {
      for (uint32_t o : bt.offsets) { if (n < cap_off) offsets[n] = base + o; ++n; }
      base += bt.bytes; ++nb;
    }
    info[1] = n; info[2] = nb;
    return 0;
  } catch (const std::exception &e) {
    copy_text(e.what(), why, cap);
    return -1;
  }
}
