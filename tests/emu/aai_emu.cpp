// aai_emu.cpp -- TEST INFRASTRUCTURE: the per-chunk logic, the pair decode and the batches of the all-pairs amino-acid identity
// (checkm_amd/csrc/aai_dev.h) compiled by g++ against a HOST executor, so that the CPU test suite runs the kernel's own arithmetic.
// aai_pairs_kernel of kernels_aai.hip is restated as a loop over its wavefronts and lanes; a batch gets a buffer of exactly its text,
// the padding behind every row filled with '-' and letters instead of zeros, so that a count that looks past a row's end shows.
// Nothing in checkm_amd loads this.
#include <cstring>
#include <vector>
#include "../../checkm_amd/csrc/aai_dev.h"

using namespace ckm;

namespace {
// one wavefront over one pair: aai_pairs_kernel
void run_pair(const std::vector<uint8_t> &text, const aai::Batch &B, const aai::Packed &P, uint64_t p, int32_t &out_mis, int32_t &out_cmp, double &out_aai) {
  const uint32_t g = aai::find_group(P.pair_off.data(), B.g_lo, B.g_hi, p);
  const aai::Group G = P.groups[g];
  uint32_t i, j;
  aai::decode_pair(p - P.pair_off[g], G.n, i, j);
  const int L = (int)G.len;
  const uint64_t stride = aai::pad16(G.len), ri = G.text_off - B.text_lo + i * stride, rj = G.text_off - B.text_lo + j * stride;
  aai::Chunk m[aai::WAVE][aai::CHUNKS];
  int first = aai::NO_COLUMN, last = -1;                       // the wave minimum and maximum
  for (int lane = 0; lane < aai::WAVE; ++lane)
    for (int c = 0; c < aai::CHUNKS; ++c) {
      const int off = c * aai::WAVE_BYTES + lane * aai::LANE_BYTES;
      uint32_t x[4] = {0, 0, 0, 0}, y[4] = {0, 0, 0, 0};
      if (off < L) {                                            // .at(): the chunk's last byte is in the batch
        memcpy(x, &text.at(ri + off + aai::LANE_BYTES - 1) - (aai::LANE_BYTES - 1), aai::LANE_BYTES);
        memcpy(y, &text.at(rj + off + aai::LANE_BYTES - 1) - (aai::LANE_BYTES - 1), aai::LANE_BYTES);
      }
      m[lane][c] = aai::chunk_masks(x, y, L - off);
      aai::chunk_span(m[lane][c], off, first, last);
    }
  int start, end, mis = 0, cmp = 0;
  aai::pair_span(first, last, L, start, end);
  for (int lane = 0; lane < aai::WAVE; ++lane)
    for (int c = 0; c < aai::CHUNKS; ++c) aai::chunk_count(m[lane][c], c * aai::WAVE_BYTES + lane * aai::LANE_BYTES, start, end, mis, cmp);
  out_mis = mis; out_cmp = cmp; out_aai = aai::identity(mis, cmp);
}
}  // namespace

// The argument tests of ckm_aai_run: 0, 1 (bad argument) or 2 (size limit)
extern "C" int emu_aai_check(uint32_t ngroups, const uint64_t *group_row_off, const uint64_t *row_off, const char *text) {
  std::string why;
  return aai::check_args(ngroups, group_row_off, row_off, text, why);
}

// ckm_aai_run on the host.  pair_off [ngroups + 1]; mis, cmp, val [npairs] (the caller sizes them from the group sizes); info: npairs,
// batches, bytes.  Returns what emu_aai_check returns.
extern "C" int emu_aai_run(uint32_t ngroups, const uint64_t *group_row_off, const uint64_t *row_off, const char *text, uint64_t budget_bytes, uint64_t *pair_off, int32_t *mis,
                           int32_t *cmp, double *val, uint64_t *info) {
  std::string why;
  const int kind = aai::check_args(ngroups, group_row_off, row_off, text, why);
  if (kind != aai::ARGS_OK || !budget_bytes) return kind ? kind : 1;
  aai::Packed P;
  aai::pack(ngroups, group_row_off, row_off, text, P);
  for (const aai::Group &G : P.groups)
    for (uint32_t r = 0; G.n > 1 && r < G.n; ++r)
      for (uint64_t k = G.len; k < aai::pad16(G.len); ++k) P.text[G.text_off + r * aai::pad16(G.len) + k] = "-Ax-"[(k + r) & 3];
  memcpy(pair_off, P.pair_off.data(), ((size_t)ngroups + 1) * 8);
  info[0] = P.pair_off[ngroups]; info[1] = info[2] = 0;
  std::vector<uint8_t> dev;
  aai::Batch B;
  uint64_t cursor = 0;
  while (aai::next_batch(P, budget_bytes, cursor, B)) {
    dev.assign(P.text.begin() + B.text_lo, P.text.begin() + B.text_lo + B.text_bytes);
    for (uint64_t s = 0; s < B.npairs; ++s) run_pair(dev, B, P, B.p0 + s, mis[B.p0 + s], cmp[B.p0 + s], val[B.p0 + s]);
    info[1] += 1; info[2] += B.text_bytes;
  }
  return 0;
}

// the decode alone: (i, j) of pair k of an n-row group
extern "C" void emu_aai_decode(uint64_t k, uint64_t n, uint32_t *ij) { aai::decode_pair(k, n, ij[0], ij[1]); }
