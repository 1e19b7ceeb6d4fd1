// kernels_seqwin.hip -- per-window base counts, canonical 4-mer counts and tetranucleotide distance of the plot commands
// (checkm/plot/gcPlots.py:55-75, gcBiasPlots.py:51-66, codingDensityPlots.py:73-89, tetraDistPlots.py:63-79).  gfx950 only.  The per-byte
// logic is sw::lane_step (seqwin_dev.h), shared with the host executor of the CPU tests; the distance is ol::td_running / ol::td_combine
// (outlier_dev.h), the summation of outliers_td_kernel.
//
//   seqwin_count_kernel  a wavefront per piece (four per block), the loop sw::wave_piece (tetra_wave.h, shared with kernels_refdist.hip).
//                        A window starts at any byte, so the wave walks 16-byte-ALIGNED spans
//                        of 1 KiB from the chunk that holds its piece's first byte: every lane loads one aligned 128-bit word (1 KiB per
//                        instruction, consecutive lanes at consecutive 16-byte chunks) and
//                        masks the bytes in front of and behind its piece; the three bytes a 4-mer needs behind a chunk come from the
//                        next lane, lane 63 reads them itself.  Base counters are summed over the wave once per piece; 4-mers go into a
//                        histogram of the wave's own in LDS and from there into the window's row: a plain store when the window is this
//                        piece alone, otherwise one atomic add per non-zero entry (integers: the order does not matter).
//   seqwin_td_kernel     a wavefront per eight windows of the batch: lane = (window, running sum r of numpy's pairwise sum).  The eight
//                        lanes of a window sum its counts, divide (sig_i = double(c_i) / double(total); 0 / 0 = nan), and each lane keeps
//                        the elements its own running sums read in LDS.  Depends on -ffp-contract=off -fno-fast-math like outliers_td_kernel.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "outlier_dev.h"
#include "seqwin_dev.h"
#include "tetra_wave.h"

namespace ckm {
using namespace sw;

__global__ __launch_bounds__(256) void seqwin_count_kernel(const uint8_t *__restrict__ text, const Piece *__restrict__ pieces, uint32_t npieces,
                                                            const uint8_t *__restrict__ canon, uint32_t *__restrict__ cnt, uint32_t *__restrict__ tet) {
  __shared__ uint32_t hist[4][NKMER];
  __shared__ uint8_t lcanon[256];
  const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x >> 6;
  const uint32_t t = blockIdx.x * 4 + wv;
  hist_stage(canon, lcanon, hist[wv], lane);
  __syncthreads();
  const bool active = t < npieces;
  Piece P = {};
  if (active) P = pieces[t];
  const bool kmers = tet != nullptr && P.tet_row != NO_ROW;
  uint32_t acc[4] = {0, 0, 0, 0};
  if (active) wave_piece(text, P, lane, kmers, lcanon, hist[wv], acc);
  __syncthreads();
  if (!active) return;
#pragma unroll
  for (int k = 0; k < 4; ++k) acc[k] = wave_sum(acc[k]);
  const bool alone = (P.flags & 4u) != 0;
  if (lane == 0) {
    uint32_t *row = cnt + (uint64_t)P.cnt_row * 4;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (alone) row[k] = acc[k];
      else if (acc[k]) atomicAdd(row + k, acc[k]);
    }
  }
  if (kmers) {
    uint32_t *row = tet + (uint64_t)P.tet_row * NKMER;
    hist_flush(lane, [=](int k) {
      const uint32_t v = hist[wv][k];
      if (alone) row[k] = v;
      else if (v) atomicAdd(row + k, v);
    });
  }
}

// a lane's partner inside its group of eight: after the steps with partners 1 and 2 the lanes of each half hold the same sum, so lane
// z ^ 4 holds what ol::td_combine asks for
struct ShflPartner {
  __device__ __forceinline__ double operator()(double v, int p) const { return __shfl_xor(v, p); }
};

__global__ __launch_bounds__(256) void seqwin_td_kernel(uint32_t nwin, const uint32_t *__restrict__ tet, const uint32_t *__restrict__ win_file,
                                                         const double *__restrict__ bin_sig, double *__restrict__ td) {
  __shared__ double sig[4][ol::TD_SEQS][ol::NSIG];
  const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x >> 6, r = lane & (ol::TD_ACC - 1), grp = lane >> 3;
  const uint64_t wave = (uint64_t)blockIdx.x * 4u + wv;
  const uint64_t want = wave * ol::TD_SEQS + (uint64_t)grp;
  if (wave * ol::TD_SEQS >= nwin) return;                   // whole wavefronts only: the cross-lane moves below need every lane of a group
  const uint32_t x = want < nwin ? (uint32_t)want : nwin - 1;
  const uint32_t *row = tet + (uint64_t)x * ol::NSIG;
  uint32_t total = 0;                                       // at most w - 3 < 2^31
  for (int k = r; k < ol::NSIG; k += ol::TD_ACC) total += row[k];
  total += __shfl_xor(total, 1); total += __shfl_xor(total, 2); total += __shfl_xor(total, 4);
  double *mine = sig[wv][grp];                              // lane r writes and reads the elements r, r + 8, ...: no other lane's
  for (int k = r; k < ol::NSIG; k += ol::TD_ACC) mine[k] = ol::ratio((uint64_t)row[k], (uint64_t)total);
  const double *bin = bin_sig + (uint64_t)win_file[x] * ol::NSIG;
  const double first = ol::td_combine(ol::td_running(mine, bin, 0, ol::TD_SPLIT, r), ShflPartner());
  const double second = ol::td_combine(ol::td_running(mine, bin, ol::TD_SPLIT, ol::NSIG - ol::TD_SPLIT, r), ShflPartner());
  if (r == 0 && want < nwin) td[x] = first + second;
}

void launch_seqwin_count(hipStream_t st, const uint8_t *text, const Piece *pieces, uint32_t npieces, const uint8_t *canon, uint32_t *cnt, uint32_t *tet) {
  if (npieces) hipLaunchKernelGGL(seqwin_count_kernel, dim3((npieces + 3) / 4), dim3(256), 0, st, text, pieces, npieces, canon, cnt, tet);
}
void launch_seqwin_td(hipStream_t st, uint32_t nwin, const uint32_t *tet, const uint32_t *win_file, const double *bin_sig, double *td) {
  const uint32_t waves = (nwin + ol::TD_SEQS - 1) / ol::TD_SEQS;
  if (waves) hipLaunchKernelGGL(seqwin_td_kernel, dim3((waves + 3) / 4), dim3(256), 0, st, nwin, tet, win_file, bin_sig, td);
}

}  // namespace ckm
