// kernels_aai.hip -- amino-acid identity between all pairs of copies of a multi-copy marker (checkm/aminoAcidIdentity.py:65-89 and
// :127-161): for every pair i < j of every group the mismatches, the compared columns and 1 - mismatches / compared.  gfx950 only.
//
//   aai_pairs_kernel  one wavefront per pair (four per block).  The flat pair index is decoded to (group, i, j) by a search over
//                     pair_off and the triangular decode of aai_dev.h, both in integers.  Every lane loads its aligned 16-byte chunks
//                     of both rows (at most CHUNKS = 4 each, all loads issued before the first use) and keeps their column masks in
//                     registers; a wave min and a wave max (xlane.h) give the ends of the compared span, a second walk over the masks
//                     counts inside it, two wave sums follow and lane 0 stores the pair's three values.  Every pair owns its output
//                     slot: no atomics.  The per-chunk logic is aai::chunk_masks / chunk_span / chunk_count, shared with the host
//                     executor of the CPU tests.
// Integers up to the last step; the quotient is formed in IEEE double (this file is built without fast-math and without contraction),
// so the result depends on neither the batches nor the launch geometry.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "aai_dev.h"
#include "xlane.h"

namespace ckm {
using namespace aai;

__global__ __launch_bounds__(256) void aai_pairs_kernel(const uint8_t *__restrict__ text /* of groups g_lo .. g_hi - 1 */, uint64_t text_lo, const Group *__restrict__ groups,
                                                        const uint64_t *__restrict__ pair_off, uint32_t g_lo, uint32_t g_hi, uint64_t p0, uint32_t npairs,
                                                        int32_t *__restrict__ out_mis, int32_t *__restrict__ out_cmp, double *__restrict__ out_aai) {
  const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x >> 6;
  const uint32_t slot = blockIdx.x * 4 + wv;      // wave-uniform: the whole wavefront leaves or stays
  if (slot >= npairs) return;
  const uint64_t p = p0 + slot;
  const uint32_t g = find_group(pair_off, g_lo, g_hi, p);
  const Group G = groups[g];
  uint32_t i, j;
  decode_pair(p - pair_off[g], G.n, i, j);
  const int L = (int)G.len;
  const uint64_t stride = pad16(G.len);
  const uint8_t *ri = text + (G.text_off - text_lo) + i * stride, *rj = text + (G.text_off - text_lo) + j * stride;

  // a chunk that starts inside a row ends inside the row's 16-byte padding, which the packed text holds
  uint4 x[CHUNKS], y[CHUNKS];
#pragma unroll
  for (int c = 0; c < CHUNKS; ++c) {
    const int off = c * WAVE_BYTES + lane * LANE_BYTES;
    x[c] = y[c] = make_uint4(0, 0, 0, 0);
    if (off < L) {
      x[c] = *reinterpret_cast<const uint4 *>(ri + off);
      y[c] = *reinterpret_cast<const uint4 *>(rj + off);
    }
  }
  Chunk m[CHUNKS];
  int first = NO_COLUMN, last = -1;
#pragma unroll
  for (int c = 0; c < CHUNKS; ++c) {
    const int off = c * WAVE_BYTES + lane * LANE_BYTES;
    const uint32_t xw[4] = {x[c].x, x[c].y, x[c].z, x[c].w}, yw[4] = {y[c].x, y[c].y, y[c].z, y[c].w};
    m[c] = chunk_masks(xw, yw, L - off);          // no valid column beyond the row: a chunk that was not loaded has none
    chunk_span(m[c], off, first, last);
  }
  int start, end;
  pair_span(wave_min(first), wave_max(last), L, start, end);
  int mis = 0, cmp = 0;
#pragma unroll
  for (int c = 0; c < CHUNKS; ++c) chunk_count(m[c], c * WAVE_BYTES + lane * LANE_BYTES, start, end, mis, cmp);
  mis = wave_sum(mis); cmp = wave_sum(cmp);
  if (lane == 0) {
    out_mis[slot] = mis; out_cmp[slot] = cmp; out_aai[slot] = identity(mis, cmp);
  }
}

void launch_aai_pairs(hipStream_t st, const uint8_t *text, uint64_t text_lo, const Group *groups, const uint64_t *pair_off, uint32_t g_lo, uint32_t g_hi, uint64_t p0,
                      uint32_t npairs, int32_t *out_mis, int32_t *out_cmp, double *out_aai) {
  if (npairs)
    hipLaunchKernelGGL(aai_pairs_kernel, dim3((npairs + 3) / 4), dim3(256), 0, st, text, text_lo, groups, pair_off, g_lo, g_hi, p0, npairs, out_mis, out_cmp, out_aai);
}

}  // namespace ckm
