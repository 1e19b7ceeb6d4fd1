// seqwin_wave.h -- one wavefront over one sw::Piece, device only: the loop shared by seqwin_count_kernel (kernels_seqwin.hip) and by the
// block and window kernels of kernels_refdist.hip.  The wave walks 16-byte-ALIGNED spans of 1 KiB from the chunk that holds the piece's
// first byte: every lane loads one aligned 128-bit word and masks the bytes in front of and behind the piece (sw::lane_geom); the three
// bytes a 4-mer needs behind a chunk come from the next lane, lane 63 reads them itself; the per-byte logic is sw::lane_step.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "seqwin_dev.h"

namespace ckm {
namespace sw {

__device__ __forceinline__ uint32_t wave_sum(uint32_t x) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) x += __shfl_xor(x, s);
  return x;
}

// P is the same for every lane of the wave.  Base counters (A, C, G, T+U) are added to the lane's acc; with kmers, every 4-mer of the
// piece adds one to hist[lcanon[code]], the wave's own histogram in LDS.  The caller's text starts at a 16-byte boundary and ends in 64
// bytes of slack behind a multiple of 16: an aligned word that holds a byte of the piece or its halo lies inside the buffer.
__device__ __forceinline__ void wave_piece(const uint8_t *__restrict__ text, const Piece &P, int lane, bool kmers, const uint8_t *lcanon, uint32_t *hist,
                                           uint32_t (&acc)[4]) {
  const uint64_t pend = P.start + P.len;
  for (uint64_t step = P.start & ~(uint64_t)(LANE_BYTES - 1); step < pend; step += WAVE_BYTES) {
    const LaneGeom g = lane_geom(P, step, lane);
    uint4 v = make_uint4(0, 0, 0, 0);
    if (g.load) v = *reinterpret_cast<const uint4 *>(text + g.base);
    uint32_t h = __shfl_down(v.x, 1);
    if (lane == WAVE - 1) h = g.kend > LANE_BYTES ? *reinterpret_cast<const uint32_t *>(text + g.base + LANE_BYTES) : 0u;
    const uint32_t w[5] = {v.x, v.y, v.z, v.w, h};
    uint8_t b[LANE_BYTES + HALO];
#pragma unroll
    for (int k = 0; k < LANE_BYTES + HALO; ++k) b[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
    Lane o;
    lane_step(b, g.first, g.end, g.kend, o);
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] += o.cnt[k];
    if (kmers) {
      uint32_t m = o.kmer_mask;
      while (m) {
        const int j = __builtin_ctz(m);
        m &= m - 1;
        atomicAdd(&hist[lcanon[o.code[j]]], 1u);
      }
    }
  }
}

}  // namespace sw
}  // namespace ckm
