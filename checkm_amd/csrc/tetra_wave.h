// tetra_wave.h -- device only: what the wavefronts of kernels_nucstats.hip, kernels_seqwin.hip and kernels_refdist.hip share.
//   wave_sum                              a uint32 summed over the wavefront
//   hist_stage / hist_count / hist_flush  the canonical 4-mer histogram of one wave in LDS: the table of canonical forms staged beside it,
//                                         one atomic per 4-mer of a lane, the 136 entries handed out at the end.  Each kernel declares its
//                                         own `hist[4][NKMER]` and `lcanon[256]` and keeps its own barriers.
//   sw::wave_piece                        one wavefront over one sw::Piece: the wave walks 16-byte-ALIGNED spans of 1 KiB from the chunk that
//                                         holds the piece's first byte: every lane loads one aligned 128-bit word and masks the bytes in front
//                                         of and behind the piece (sw::lane_geom); the three bytes a 4-mer needs behind a chunk come from the
//                                         next lane, lane 63 reads them itself; the per-byte logic is sw::lane_step.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "seqwin_dev.h"

namespace ckm {

__device__ __forceinline__ uint32_t wave_sum(uint32_t x) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) x += __shfl_xor(x, s);
  return x;
}

// every thread of a block of 256 copies one entry of canon; a wave clears its own row.  The caller's __syncthreads() follows.
__device__ __forceinline__ void hist_stage(const uint8_t *__restrict__ canon, uint8_t *lcanon, uint32_t *hist, int lane) {
  lcanon[threadIdx.x] = canon[threadIdx.x];
  for (int k = lane; k < NKMER; k += WAVE) hist[k] = 0;
}

// the 4-mers of one lane's chunk: bit j of m <-> a valid 4-mer with code[j] starts at chunk byte j
__device__ __forceinline__ void hist_count(uint32_t m, const uint8_t *code, const uint8_t *lcanon, uint32_t *hist) {
  while (m) {
    const int j = __builtin_ctz(m);
    m &= m - 1;
    atomicAdd(&hist[lcanon[code[j]]], 1u);
  }
}

// the 136 entries strided over the lanes: put(k) reads the wave's hist[k] and stores it, adds it where it is not zero, or stores it plus a
// prefix difference.  By value: a functor taken by reference changes the code the compiler emits for the loop.
template <class Put>
__device__ __forceinline__ void hist_flush(int lane, Put put) {
  for (int k = lane; k < NKMER; k += WAVE) put(k);
}

namespace sw {

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
    if (kmers) hist_count(o.kmer_mask, o.code, lcanon, hist);
  }
}

}  // namespace sw
}  // namespace ckm
