// kernels_nucstats.hip -- the nucleotide statistics of BinStatistics and the tetranucleotide counts of GenomicSignatures in one pass over
// the bytes (checkm/binStatistics.py:173-234, checkm/util/seqUtils.py:279-286, checkm/genomicSignatures.py:131-149).  gfx950 only.
//
// Every sequence is cut into tiles of a fixed size; one wavefront owns one tile (four per block) and walks it 1 KiB per step, 16 bytes per
// lane loaded as one 128-bit word.  The halo a lane needs (the byte in front of its chunk, the 12 after it) comes from its neighbours by
// cross-lane moves; only lane 0 and lane 63 read it from memory.  The per-byte logic is ns::lane_step (nucstats_dev.h), shared with the
// host executor of the CPU tests.
//
//   nucstats_count_kernel  per tile: the nine counters of ns::NCOUNT (integers, summed over the wave at the end of the tile) and, when
//                          asked, the 136 canonical 4-mer counts: each wave counts into a histogram of its own in LDS and adds it to the
//                          sequence's row with one atomic per non-zero entry when its tile is done (integer adds: the result does not
//                          depend on their order).
//   nucstats_fill_kernel   per tile that has run starts (the count pass counted them, the host scanned the counts): the number of
//                          non-'N' code points of the sequence in front of every run start, written in order at the tile's offset.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "nucstats_dev.h"
#include "pairs_wave.h"
#include "tetra_wave.h"

namespace ckm {
using namespace ns;

__device__ __forceinline__ void load_lane(const uint8_t *text, const Tile &T, uint64_t off, int lane, uint8_t *b, int &nvalid, int64_t &in_seq, bool &has_prev) {
  const uint64_t base = T.start + off + (uint64_t)lane * LANE_BYTES;
  const int64_t rem = (int64_t)T.len - (int64_t)(off + (uint64_t)lane * LANE_BYTES);
  nvalid = rem <= 0 ? 0 : rem >= LANE_BYTES ? LANE_BYTES : (int)rem;
  in_seq = (int64_t)T.seq_end - (int64_t)base;
  has_prev = base > T.seq_start;
  // the text has every sequence at a 16-byte boundary and 64 bytes of slack at its end: a load that starts inside a sequence stays
  // inside the buffer
  uint4 v = make_uint4(0, 0, 0, 0);
  if (in_seq > 0) v = *reinterpret_cast<const uint4 *>(text + base);
  uint32_t h0 = __shfl_down(v.x, 1), h1 = __shfl_down(v.y, 1), h2 = __shfl_down(v.z, 1);
  uint32_t prev = __shfl_up(v.w, 1) >> 24;
  if (lane == WAVE - 1) {
    h0 = h1 = h2 = 0;
    if (in_seq > LANE_BYTES) { const uint4 n = *reinterpret_cast<const uint4 *>(text + base + LANE_BYTES); h0 = n.x; h1 = n.y; h2 = n.z; }
  }
  if (lane == 0) prev = has_prev ? text[base - 1] : 0;
  const uint32_t w[7] = {v.x, v.y, v.z, v.w, h0, h1, h2};
  b[0] = (uint8_t)prev;
#pragma unroll
  for (int k = 0; k < 28; ++k) b[1 + k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
}

__global__ __launch_bounds__(256) void nucstats_count_kernel(const uint8_t *__restrict__ text, const Tile *__restrict__ tiles, uint32_t ntiles,
                                                              const uint8_t *__restrict__ canon, uint32_t *__restrict__ tile_cnt, uint32_t *__restrict__ tetra) {
  __shared__ uint32_t hist[4][NKMER];
  __shared__ uint8_t lcanon[256];
  const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x >> 6;
  const uint32_t t = blockIdx.x * 4 + wv;
  hist_stage(canon, lcanon, hist[wv], lane);
  __syncthreads();
  const bool active = t < ntiles;
  Tile T = {};
  if (active) T = tiles[t];
  uint32_t acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint32_t nev = 0;
  for (uint64_t off = 0; active && off < T.len; off += WAVE_BYTES) {
    uint8_t b[1 + LANE_BYTES + HALO];
    int nvalid; int64_t in_seq; bool has_prev;
    load_lane(text, T, off, lane, b, nvalid, in_seq, has_prev);
    Lane o;
    lane_step(b, nvalid, in_seq, has_prev, o);
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] += o.cnt[k];
    nev += (uint32_t)__builtin_popcount(o.ev_mask);
    if (tetra) hist_count(o.kmer_mask, o.code, lcanon, hist[wv]);
  }
  __syncthreads();
  if (!active) return;
#pragma unroll
  for (int k = 0; k < 8; ++k) acc[k] = wave_sum(acc[k]);
  nev = wave_sum(nev);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 8; ++k) tile_cnt[(uint64_t)t * NCOUNT + k] = acc[k];
    tile_cnt[(uint64_t)t * NCOUNT + C_EV] = nev;
  }
  if (tetra) {
    uint32_t *row = tetra + (uint64_t)T.seq * NKMER;
    hist_flush(lane, [=](int k) { const uint32_t v = hist[wv][k]; if (v) atomicAdd(row + k, v); });
  }
}

// ev_off[t] .. ev_off[t + 1]: the tile's slots in ev; nonn_base[t]: non-'N' code points of the tile's sequence in front of the tile
__global__ __launch_bounds__(256) void nucstats_fill_kernel(const uint8_t *__restrict__ text, const Tile *__restrict__ tiles, uint32_t ntiles,
                                                             const uint64_t *__restrict__ ev_off, const uint64_t *__restrict__ nonn_base, uint64_t *__restrict__ ev) {
  const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x >> 6;
  const uint32_t t = blockIdx.x * 4 + wv;
  if (t >= ntiles) return;
  uint64_t slot = ev_off[t];
  if (ev_off[t + 1] == slot) return;
  const Tile T = tiles[t];
  uint64_t before = nonn_base[t];
  for (uint64_t off = 0; off < T.len; off += WAVE_BYTES) {
    uint8_t b[1 + LANE_BYTES + HALO];
    int nvalid; int64_t in_seq; bool has_prev;
    load_lane(text, T, off, lane, b, nvalid, in_seq, has_prev);
    Lane o;
    lane_step(b, nvalid, in_seq, has_prev, o);
    const uint32_t nn = (uint32_t)__builtin_popcount(o.nonn_mask), ne = (uint32_t)__builtin_popcount(o.ev_mask);
    const uint32_t inc = wave_inclusive(nn | (ne << 16), lane);     // both at most 1024 per step: two 16-bit halves do not carry
    const uint32_t exc = inc - (nn | (ne << 16));
    uint64_t my_slot = slot + (exc >> 16);
    const uint64_t my_before = before + (exc & 0xFFFFu);
    uint32_t m = o.ev_mask;
    while (m) {
      const int j = __builtin_ctz(m);
      m &= m - 1;
      ev[my_slot++] = my_before + (uint32_t)__builtin_popcount(o.nonn_mask & ((1u << j) - 1u));
    }
    const uint32_t tot = __shfl(inc, WAVE - 1);
    slot += tot >> 16;
    before += tot & 0xFFFFu;
  }
}

void launch_nucstats_count(hipStream_t st, const uint8_t *text, const Tile *tiles, uint32_t ntiles, const uint8_t *canon, uint32_t *tile_cnt, uint32_t *tetra) {
  if (ntiles) hipLaunchKernelGGL(nucstats_count_kernel, dim3((ntiles + 3) / 4), dim3(256), 0, st, text, tiles, ntiles, canon, tile_cnt, tetra);
}
void launch_nucstats_fill(hipStream_t st, const uint8_t *text, const Tile *tiles, uint32_t ntiles, const uint64_t *ev_off, const uint64_t *nonn_base, uint64_t *ev) {
  if (ntiles) hipLaunchKernelGGL(nucstats_fill_kernel, dim3((ntiles + 3) / 4), dim3(256), 0, st, text, tiles, ntiles, ev_off, nonn_base, ev);
}

}  // namespace ckm
