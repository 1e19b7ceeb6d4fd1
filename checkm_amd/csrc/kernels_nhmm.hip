// kernels_nhmm.hip -- the nucleotide model scan of SSU_Finder on the device (gfx950), arithmetic and layout in nhmm_dev.h.
//
// nhmm_scan_kernel<Q>: a workgroup of four wavefronts, all on one model whose image (5 emission + 7 transition rows of Q * 64 words,
// 12 Q * 256 bytes: 96 KB at Q = 32) sits in LDS as [row][j][lane], so a row of the recurrence reads consecutive words.  One wavefront
// per tile.  Lane z keeps the M, I and D cells of the nodes z Q + 1 .. z Q + Q of the current row in 6 Q registers (a cell is an
// int64: score in the high word, ~start in the low one; adding a transition touches the high word only).  Per row:
//   - the cells (i-1, z Q) come from lane z - 1 by one cross-lane shift of three cells;
//   - M and I are updated in place from j = Q - 1 down to 0;
//   - the D chain of the chunk runs once from NEG and gives the chunk's map d -> best(c, d + T), T the (saturating) sum of its tDD;
//     the maps compose exactly in integers, a Kogge-Stone scan over the lanes gives every lane the D cell entering its chunk, and the
//     chain runs a second time from it;
//   - best_k M(i,k) is a butterfly over the lanes; lane 0 stores the row's cell when the tile owns it and counts it against the threshold.
// The 64 residues of the next rows are one register of the wavefront (lane l: row base + l), handed out by v_readlane.
// No atomics: a tile's rows go to its own slots of the batch's row buffer, its count to counts[tile]; after a host scan of the counts
// nhmm_fill_kernel writes the reported rows in (tile, row) order with a ballot and a prefix popcount per 64 rows.
#include <hip/hip_runtime.h>
#include "ckm_host.h"
#include "nhmm_dev.h"

namespace ckm {
using namespace nhmm;

__device__ __forceinline__ cell lane_up(cell c, int lane) {      // lane z <- lane z - 1, lane 0 <- NEG
  const cell o = __shfl_up(c, 1);
  return lane ? o : neg_cell();
}

template <int Q>
__global__ __launch_bounds__(256) void nhmm_scan_kernel(const int32_t *__restrict__ image, int32_t tBM, const TileDev *__restrict__ tiles, uint32_t ntiles,
                                                        const uint8_t *__restrict__ text, cell *__restrict__ rowbuf, uint32_t *__restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) int32_t lds[];
  for (int x = threadIdx.x; x < NIMG * Q * 64; x += 256) lds[x] = image[x];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const uint32_t ti = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (ti >= ntiles) return;
  const TileDev t = tiles[ti];
  const int32_t *tab = lds + lane;
#define TR(R, J) tab[((5 + (R)) * Q + (J)) * 64]
  cell M[Q], I[Q], D[Q];
#pragma unroll
  for (int j = 0; j < Q; ++j) M[j] = I[j] = D[j] = neg_cell();
  long long tsum = 0;
#pragma unroll
  for (int j = 0; j < Q; ++j) tsum += TR(T_DD, j);
  const int32_t T = (int32_t)(tsum < TSAT ? TSAT : tsum);
  uint32_t count = 0;
  for (uint32_t base = t.first; base <= t.last; base += 64) {
    const uint32_t r = base + lane;
    int code = 4;
    if (r <= t.last) {
      const uint8_t c = text[t.text_off + (t.strand ? (uint64_t)(t.L - r) : (uint64_t)(r - 1))];
      code = t.strand ? comp_of(code_of(c)) : code_of(c);
    }
    const int n = (int)min(64u, t.last - base + 1);
    for (int rr = 0; rr < n; ++rr) {
      const int cd = __builtin_amdgcn_readlane(code, rr);
      const int32_t *e = tab + cd * Q * 64;
      const uint32_t i = base + rr;
      const cell entry = mk(tBM, i);
      const cell mIn = lane_up(M[Q - 1], lane), iIn = lane_up(I[Q - 1], lane), dIn = lane_up(D[Q - 1], lane);
#pragma unroll
      for (int j = Q - 1; j >= 0; --j) {
        const cell pm = j ? M[j ? j - 1 : 0] : mIn, pi = j ? I[j ? j - 1 : 0] : iIn, pd = j ? D[j ? j - 1 : 0] : dIn;
        const cell ni = best(add(M[j], TR(T_MI, j)), add(I[j], TR(T_II, j)));
        const cell nm = best(best(entry, add(pm, TR(T_MM, j))), best(add(pi, TR(T_IM, j)), add(pd, TR(T_DM, j))));
        I[j] = ni;
        M[j] = add(nm, e[j * 64]);
      }
      // the D row: the chunk's map from NEG, the scan of the maps, the chain again from the cell that enters the chunk
      const cell mPrev = lane_up(M[Q - 1], lane);
      cell c = neg_cell();
#pragma unroll
      for (int j = 0; j < Q; ++j) c = best(add(j ? M[j ? j - 1 : 0] : mPrev, TR(T_MD, j)), add(c, TR(T_DD, j)));
      int32_t sT = T;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const cell oc = __shfl_up(c, off);
        const int32_t oT = __shfl_up(sT, off);
        if (lane >= off) {
          c = best(c, add(oc, sT));
          const int32_t s = sT + oT;      // both >= TSAT = -2^30: no overflow
          sT = s < TSAT ? TSAT : s;
        }
      }
      cell d = lane_up(c, lane);
#pragma unroll
      for (int j = 0; j < Q; ++j) { d = best(add(j ? M[j ? j - 1 : 0] : mPrev, TR(T_MD, j)), add(d, TR(T_DD, j))); D[j] = d; }
      cell rb = M[0];
#pragma unroll
      for (int j = 1; j < Q; ++j) rb = best(rb, M[j]);
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) rb = best(rb, __shfl_xor(rb, off));
      if (i >= t.own && lane == 0) {
        rowbuf[t.out_off + (i - t.own)] = rb;
        count += score_of(rb) >= t.thr ? 1u : 0u;
      }
    }
  }
#undef TR
  if (lane == 0) counts[ti] = count;
}

// one wavefront per tile: the rows at or above the tile's threshold, in row order, from dst_off[tile] on
__global__ __launch_bounds__(256) void nhmm_fill_kernel(const cell *__restrict__ rowbuf, const TileDev *__restrict__ tiles, const uint64_t *__restrict__ dst_off, uint32_t ntiles,
                                                        uint32_t *__restrict__ o_tile, uint32_t *__restrict__ o_pos, uint32_t *__restrict__ o_start, int32_t *__restrict__ o_score) {
  const int lane = threadIdx.x & 63;
  const uint32_t ti = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (ti >= ntiles) return;
  const TileDev t = tiles[ti];
  const uint32_t n = t.last - t.own + 1;
  uint64_t at = dst_off[ti];
  for (uint32_t base = 0; base < n; base += 64) {
    const uint32_t k = base + lane;
    const cell c = k < n ? rowbuf[t.out_off + k] : neg_cell();
    const bool keep = k < n && score_of(c) >= t.thr;
    const unsigned long long mask = __ballot(keep);
    if (keep) {
      const uint64_t w = at + __popcll(mask & ((1ull << lane) - 1ull));
      o_tile[w] = ti; o_pos[w] = t.own + k; o_start[w] = start_of(c); o_score[w] = score_of(c);
    }
    at += __popcll(mask);
  }
}

#define CKM_NHMM_QS(X) X(1) X(2) X(4) X(8) X(16) X(24) X(32)

void launch_nhmm_scan(hipStream_t st, int Q, const int32_t *image, int32_t tBM, const TileDev *tiles, uint32_t ntiles, const uint8_t *text, long long *rowbuf, uint32_t *counts) {
  if (!ntiles) return;
  const size_t bytes = (size_t)NIMG * Q * 64 * 4;
  const dim3 grid((ntiles + 3) / 4), block(256);
  switch (Q) {
#define X(QV) case QV: { if (bytes > 65536) (void)hipFuncSetAttribute((const void *)nhmm_scan_kernel<QV>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes); \
                         hipLaunchKernelGGL(nhmm_scan_kernel<QV>, grid, block, bytes, st, image, tBM, tiles, ntiles, text, rowbuf, counts); break; }
    CKM_NHMM_QS(X)
#undef X
    default: throw Error(CKM_ERANGE, "no scan kernel for " + std::to_string(Q) + " nodes per lane");
  }
}

void launch_nhmm_fill(hipStream_t st, const long long *rowbuf, const TileDev *tiles, const uint64_t *dst_off, uint32_t ntiles, uint32_t *o_tile, uint32_t *o_pos, uint32_t *o_start, int32_t *o_score) {
  if (!ntiles) return;
  hipLaunchKernelGGL(nhmm_fill_kernel, dim3((ntiles + 3) / 4), dim3(256), 0, st, rowbuf, tiles, dst_off, ntiles, o_tile, o_pos, o_start, o_score);
}

}  // namespace ckm
