// kernels_markerset.hip -- MarkerSetBuilder on the device (scripts/genometreeworkflow/markerSetBuilder.py of the reference: markerGenes
// :131-157, missingGenes :486-510, duplicateGenes :512-536, colocatedGenes :159-192).  gfx950 only.  The arithmetic is markerset_dev.h,
// shared with the host executor of the CPU tests; the one float operation per pair is an IEEE double division (the library's
// -ffp-contract=off -fno-fast-math).
//
//   mset_markers_kernel  a lane per (query, family).  The block stages the query's genome list in LDS, THREADS indices at a time; a lane
//                        reads cls[g * C + f], neighbouring lanes neighbouring bytes, and keeps ubiquity, single-copy and duplicate counts
//                        in registers.  One flag byte out, on request the three counts.
//   mset_pack_kernel     a thread per (genome, marker) entry of a round: the first copy and the number of copies, densely [ng][nm] per
//                        query, so that the tiles read rows of entries instead of chasing the table's offsets.
//   mset_tile_kernel     a block of four wavefronts per tile of 64 x 64 marker pairs of one query; the tiles of all queries of a round are
//                        one list (grid = its length).  A lane owns column j, a wavefront sixteen rows i: their counts live in registers.
//                        Per GCHUNK genomes the entries of the 64 row markers and the 64 column markers, and the genome indices, are
//                        staged in LDS (the row side is read by a whole wavefront at one address: a broadcast).  The single-copy case is a
//                        subtraction and a compare; more copies walk the table's own list.  Then a row at a time: the reference's test, a
//                        64-bit ballot, and the count or the fill step of pairs_wave.h: the output is in (query, i, j) order and no atomic
//                        decides a position.  In the fill pass a tile without a reported pair exits at once.
//   mset_scan_kernel     a wavefront per row of the round: pc::row_scan over the row's tile counts, the row's total out.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "markerset_dev.h"
#include "pairs_wave.h"

namespace ckm {
using namespace ms;

__global__ __launch_bounds__(THREADS) void mset_markers_kernel(MsetTableDev T, uint32_t q0, const uint64_t *__restrict__ qg_off, const uint32_t *__restrict__ qg,
                                                                const double *__restrict__ tU, const double *__restrict__ tS, uint8_t *__restrict__ flag,
                                                                uint32_t *__restrict__ counts) {
  __shared__ uint32_t sG[THREADS];
  const uint32_t q = q0 + blockIdx.y, f = blockIdx.x * (uint32_t)THREADS + threadIdx.x;
  const uint64_t g0 = qg_off[q], ng = qg_off[q + 1] - g0;
  const bool mine = f < T.C;
  uint32_t ubiquity = 0, single = 0, duplicate = 0;
  for (uint64_t k0 = 0; k0 < ng; k0 += THREADS) {
    const uint32_t kc = ng - k0 < (uint64_t)THREADS ? (uint32_t)(ng - k0) : (uint32_t)THREADS;
    __syncthreads();                                           // the readers of the chunk before
    if (threadIdx.x < kc) sG[threadIdx.x] = qg[g0 + k0 + threadIdx.x];
    __syncthreads();
    if (mine)
      for (uint32_t k = 0; k < kc; ++k) class_step(T.cls[(uint64_t)sG[k] * T.C + f], ubiquity, single, duplicate);
  }
  if (!mine) return;
  const uint64_t at = (uint64_t)blockIdx.y * T.C + f;          // the outputs of a call start at its first query
  flag[at] = family_flags(ubiquity, single, duplicate, (uint32_t)ng, tU[q], tS[q]);
  if (counts) { counts[at * 3] = ubiquity; counts[at * 3 + 1] = single; counts[at * 3 + 2] = duplicate; }
}

__global__ __launch_bounds__(THREADS) void mset_pack_kernel(MsetTableDev T, const Query *__restrict__ queries, uint32_t nq, uint64_t nentries,
                                                             const uint32_t *__restrict__ qg, const uint32_t *__restrict__ qm, Entry *__restrict__ pk) {
  const uint64_t e = (uint64_t)blockIdx.x * THREADS + threadIdx.x;
  if (e >= nentries) return;
  const Query Q = queries[find_query(nq, e, [&](uint32_t k) { return queries[k].pk_off; })];
  const uint64_t local = e - Q.pk_off;
  const uint32_t gi = (uint32_t)(local / Q.nm), mi = (uint32_t)(local % Q.nm);
  const uint64_t cell = (uint64_t)qg[Q.g_off + gi] * T.C + qm[Q.m_off + mi];
  const uint32_t o = T.pos_off[cell], n = T.pos_off[cell + 1] - o;
  pk[e] = Entry{n ? T.pos[o] : 0, n};
}

template <bool FILL>
__global__ __launch_bounds__(THREADS) void mset_tile_kernel(MsetTableDev T, const Query *__restrict__ queries, const Tile *__restrict__ tiles, const uint32_t *__restrict__ qg,
                                                             const uint32_t *__restrict__ qm, const Entry *__restrict__ pk, int32_t D, double genome_threshold,
                                                             uint32_t row_lo, uint32_t row_hi, uint32_t *__restrict__ tile_count, MsetOut out) {
  __shared__ Entry sI[GCHUNK * TILE], sJ[GCHUNK * TILE];
  __shared__ uint32_t sG[GCHUNK], sFi[TILE], sFj[TILE];
  const Tile tile = tiles[blockIdx.x];
  const Query Q = queries[tile.q];
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
  const uint32_t i0 = tile.ti * (uint32_t)TILE, j0 = tile.tj * (uint32_t)TILE, ntj = tiles_for(Q.nm);
  const Entry *qpk = pk + Q.pk_off;
  if (FILL) {                                                   // a tile none of whose rows reports a pair has nothing to fill
    bool any = false;
    const uint32_t i = i0 + threadIdx.x, row = Q.row_off + i;
    if (threadIdx.x < (uint32_t)TILE && i < Q.nm && row >= row_lo && row < row_hi)
      any = tile_pairs(tile_count + Q.cnt_off + (uint64_t)i * ntj, tile.tj, ntj, out.row_total[row]) != 0;
    if (!__syncthreads_or(any)) return;
  }
  if (threadIdx.x < (uint32_t)TILE) {
    sFi[threadIdx.x] = i0 + threadIdx.x < Q.nm ? qm[Q.m_off + i0 + threadIdx.x] : 0u;
    sFj[threadIdx.x] = j0 + threadIdx.x < Q.nm ? qm[Q.m_off + j0 + threadIdx.x] : 0u;
  }
  uint32_t cnt[ROWS_PER_WAVE];
#pragma unroll
  for (int r = 0; r < ROWS_PER_WAVE; ++r) cnt[r] = 0;
  for (uint32_t g0 = 0; g0 < Q.ng; g0 += GCHUNK) {
    const uint32_t gc = Q.ng - g0 < (uint32_t)GCHUNK ? Q.ng - g0 : (uint32_t)GCHUNK;
    __syncthreads();                                           // the readers of the chunk before
    for (uint32_t x = threadIdx.x; x < gc * (uint32_t)TILE; x += THREADS) {
      const uint32_t gg = x / (uint32_t)TILE, c = x % (uint32_t)TILE;
      const Entry *row = qpk + (uint64_t)(g0 + gg) * Q.nm;
      sI[x] = i0 + c < Q.nm ? row[i0 + c] : Entry{0, 0u};
      sJ[x] = j0 + c < Q.nm ? row[j0 + c] : Entry{0, 0u};
    }
    if (threadIdx.x < gc) sG[threadIdx.x] = qg[Q.g_off + g0 + threadIdx.x];
    __syncthreads();
    for (uint32_t gg = 0; gg < gc; ++gg) {
      const Entry ej = sJ[gg * TILE + lane];
#pragma unroll
      for (int r = 0; r < ROWS_PER_WAVE; ++r) {
        const int ri = wave * ROWS_PER_WAVE + r;
        const Entry ei = sI[gg * TILE + ri];
        cnt[r] += pair_step(ei, ej, D, [&] {
          const uint64_t cell = (uint64_t)sG[gg] * T.C;          // entries with n > 0 belong to markers of the query: sFi / sFj hold their families
          return near_any(T.pos + T.pos_off[cell + sFi[ri]], ei.n, T.pos + T.pos_off[cell + sFj[lane]], ej.n, D);
        });
      }
    }
  }
  const uint32_t j = j0 + (uint32_t)lane;
#pragma unroll
  for (int r = 0; r < ROWS_PER_WAVE; ++r) {
    const uint32_t i = i0 + (uint32_t)(wave * ROWS_PER_WAVE + r);            // the same for every lane of the wavefront
    const uint32_t row = Q.row_off + i;
    if (i >= Q.nm || row < row_lo || row >= row_hi) continue;
    const bool keep = j < Q.nm && j > i && reported(cnt[r], Q.ng, genome_threshold);
    const uint64_t ballot = __ballot(keep);
    const uint64_t at = Q.cnt_off + (uint64_t)i * ntj + tile.tj;
    if (!FILL) {
      pc::count_store(ballot, lane, tile_count, at);
    } else if (keep) {
      const int below = pc::lanes_below(ballot);
      const uint64_t slot = pair_slot(out.row_base[row], tile_count[at], below, out.batch_base);
      if (slot < out.cap) { out.pi[slot] = i; out.pj[slot] = j; out.count[slot] = cnt[r]; }
    }
  }
}

__global__ __launch_bounds__(THREADS) void mset_scan_kernel(const Query *__restrict__ queries, uint32_t nq, uint32_t nrows, uint32_t *__restrict__ tile_count,
                                                             uint32_t *__restrict__ row_total) {
  const int lane = threadIdx.x & (WAVE - 1);
  const uint32_t k = blockIdx.x * (uint32_t)WAVES + (threadIdx.x >> 6);
  if (k >= nrows) return;
  const Query Q = queries[find_query(nq, k, [&](uint32_t q) { return (uint64_t)queries[q].row_off; })];
  const uint32_t i = k - Q.row_off, ntj = tiles_for(Q.nm);
  const uint32_t total = pc::row_scan(tile_count + Q.cnt_off + (uint64_t)i * ntj, 1u, i / (uint32_t)TILE, ntj, lane);
  if (lane == 0) row_total[k] = total;
}

// queries [q0, q0 + nq) of the call; flag and counts start at q0
void launch_mset_markers(hipStream_t st, const MsetTableDev &T, uint32_t q0, uint32_t nq, const uint64_t *qg_off, const uint32_t *qg, const double *tU, const double *tS,
                         uint8_t *flag, uint32_t *counts) {
  if (!nq || !T.C) return;
  hipLaunchKernelGGL(mset_markers_kernel, dim3((T.C + THREADS - 1) / THREADS, nq), dim3(THREADS), 0, st, T, q0, qg_off, qg, tU, tS, flag, counts);
}
void launch_mset_pack(hipStream_t st, const MsetTableDev &T, const Query *queries, uint32_t nq, uint64_t nentries, const uint32_t *qg, const uint32_t *qm, Entry *pk) {
  if (!nentries) return;
  hipLaunchKernelGGL(mset_pack_kernel, dim3((uint32_t)((nentries + THREADS - 1) / THREADS)), dim3(THREADS), 0, st, T, queries, nq, nentries, qg, qm, pk);
}
// tiles [t_lo, t_hi) of the round's list, rows [row_lo, row_hi) of the round
void launch_mset_tiles(hipStream_t st, bool fill, const MsetTableDev &T, const Query *queries, const Tile *tiles, uint32_t t_lo, uint32_t t_hi, const uint32_t *qg,
                       const uint32_t *qm, const Entry *pk, int32_t D, double genome_threshold, uint32_t row_lo, uint32_t row_hi, uint32_t *tile_count, const MsetOut &out) {
  if (t_lo >= t_hi || row_lo >= row_hi) return;
  const dim3 grid(t_hi - t_lo);
  if (fill) hipLaunchKernelGGL(mset_tile_kernel<true>, grid, dim3(THREADS), 0, st, T, queries, tiles + t_lo, qg, qm, pk, D, genome_threshold, row_lo, row_hi, tile_count, out);
  else hipLaunchKernelGGL(mset_tile_kernel<false>, grid, dim3(THREADS), 0, st, T, queries, tiles + t_lo, qg, qm, pk, D, genome_threshold, row_lo, row_hi, tile_count, out);
}
void launch_mset_scan(hipStream_t st, const Query *queries, uint32_t nq, uint32_t nrows, uint32_t *tile_count, uint32_t *row_total) {
  if (nrows) hipLaunchKernelGGL(mset_scan_kernel, dim3((nrows + WAVES - 1) / WAVES), dim3(THREADS), 0, st, queries, nq, nrows, tile_count, row_total);
}

}  // namespace ckm
