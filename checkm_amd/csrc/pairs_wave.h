// pairs_wave.h -- device only: the wavefront steps of the count / scan / fill compaction of pairs_dev.h, and the prefix loop under them.
//   wave_inclusive             inclusive prefix of a value over the lanes of a wavefront
//   row_scan                   a wavefront over a strided row: exclusive prefix in place with a carry across steps of 64, the total out
//   count_store / lanes_below  what a tile kernel does with the ballot of a row's reported pairs: count pass, fill pass (pair_slot)
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "pairs_dev.h"
#include "wave_const.h"

namespace ckm {

template <class T>
__device__ __forceinline__ T wave_inclusive(T v, int lane) {
#pragma unroll
  for (int d = 1; d < WAVE; d <<= 1) {
    const T up = __shfl_up(v, d, WAVE);
    if (lane >= d) v += up;
  }
  return v;
}

namespace pc {

// row[k * stride], k in [first, n), becomes the sum of those before it; every lane returns the sum of all.  Nothing outside [first, n) is
// read or written.
__device__ __forceinline__ uint32_t row_scan(uint32_t *row, uint32_t stride, uint32_t first, uint32_t n, int lane) {
  uint32_t carry = 0;
  for (uint32_t base = first; base < n; base += WAVE) {
    const uint32_t t = base + (uint32_t)lane;
    const uint32_t v = t < n ? row[(uint64_t)t * stride] : 0u;
    const uint32_t incl = wave_inclusive(v, lane);
    if (t < n) row[(uint64_t)t * stride] = carry + incl - v;
    carry += __shfl(incl, WAVE - 1, WAVE);
  }
  return carry;
}

// count pass: tile_count[at] = the pairs this row reports in this tile
__device__ __forceinline__ void count_store(uint64_t ballot, int lane, uint32_t *tile_count, uint64_t at) {
  if (lane == 0) tile_count[at] = (uint32_t)__popcll(ballot);
}

// fill pass: the reported pairs of this row and tile in the lanes below this one, pair_slot's `below`
__device__ __forceinline__ int lanes_below(uint64_t ballot) {
  return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
}

}  // namespace pc
}  // namespace ckm
