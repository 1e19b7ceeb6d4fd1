// kernels_place.hip -- the phylogenetic placement on the device (what checkm/pplacer.py :70-87 asks of pplacer and guppy: the edge of the
// reference tree a bin's concatenated alignment attaches to).  gfx950 only.  The layout and the arithmetic are place_dev.h, shared with
// the host executor of the CPU tests: IEEE double +, * and comparisons in one written order, exact scaling, no exp and no log (the
// library's -ffp-contract=off -fno-fast-math).  Plain FP64 VALU; DESIGN section 23.
//
//   pmat_kernel        a thread per entry of a transition matrix P = U diag(e) U^-1 from a host-made table of exponentials.
//   up_level_kernel    a thread per (node of the level, site): a leaf's one-hot column, or the product of the children's messages; the
//   down_level_kernel  same for the edges of a depth, from the parent's proximal partial and the siblings.  Sites run along the lanes
//                      (the partials are site-fastest), so a wavefront reads one node's matrices at wave-uniform addresses.
//   root_kernel        a thread per site: the reference tree's own likelihood at the root, the factor of every unknown query site.
//   table_kernel       a thread per (edge, site): the 21 entries of the scan's table, attachment at the midpoint with the start pendant.
//   scan_kernel        a workgroup per (edge, 256 queries).  It takes the edge's table 256 sites at a time into LDS (21 x 256 doubles);
//                      each of its four wavefronts walks queries with the lanes over sites: a look-up by the query's code, the product
//                      of sixty-four sites by a fixed butterfly (xlane.h's moves; partners 1, 2, 4, 8, 16, 32), the blocks folded in site order into the
//                      (query, edge) product, which lives in global memory between tiles and chunks.  No atomics.
//   topk_kernel        a workgroup per query: maxPitches rounds of "the best edge after the previous pick", ties to the lower edge.
//   refine_kernel      a wavefront per kept (query, edge): every distal fraction x pendant length, the same site order as the scan.
//   best_kernel        a thread per kept pair: the first maximum in (distal, pendant) order.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "place_dev.h"
#include "xlane.h"

namespace ckm {
using namespace place;

constexpr int THREADS = 256;

__global__ __launch_bounds__(THREADS) void pmat_kernel(const double *__restrict__ U, const double *__restrict__ Ui, const double *__restrict__ ex, double *__restrict__ P, uint64_t nmat) {
  const uint64_t idx = (uint64_t)blockIdx.x * THREADS + threadIdx.x;
  if (idx >= nmat * PM) return;
  const uint64_t m = idx / PM;
  const int ij = (int)(idx % PM);
  P[idx] = pmat_entry(U, Ui, ex + m * NS, ij / NS, ij % NS);
}

__global__ __launch_bounds__(THREADS) void fill_one_kernel(double *__restrict__ m, long long *__restrict__ e, uint64_t n) {
  const uint64_t idx = (uint64_t)blockIdx.x * THREADS + threadIdx.x;
  if (idx >= n) return;
  const Sc o = one();
  m[idx] = o.m; e[idx] = o.e;
}

// (entry k of the list, site s) of a flat grid whose wavefronts stay inside one entry: Cpad = c rounded up to 64
__device__ __forceinline__ bool list_site(uint32_t count, uint32_t c, uint32_t &k, uint32_t &s) {
  const uint32_t cpad = (c + WAVE - 1) / WAVE * WAVE;
  const uint64_t idx = (uint64_t)blockIdx.x * THREADS + threadIdx.x;
  k = (uint32_t)(idx / cpad); s = (uint32_t)(idx % cpad);
  return k < count && s < c;
}

__global__ __launch_bounds__(THREADS) void up_level_kernel(PlaceDev T, const uint32_t *__restrict__ nodes, uint32_t count, uint32_t s0, uint32_t c) {
  uint32_t k, s;
  if (!list_site(count, c, k, s)) return;
  const uint32_t v = nodes[k];
  const int32_t row = T.leaf_row[v];
  if (row >= 0) leaf_site(T.D, T.dexp, v, T.R, c, s, T.rowcode[(uint64_t)row * T.S + s0 + s]);
  else up_site(T.D, T.dexp, v, T.child_off, T.child, T.Plen, T.R, c, s);
}

__global__ __launch_bounds__(THREADS) void down_level_kernel(PlaceDev T, const uint32_t *__restrict__ nodes, uint32_t count, uint32_t c) {
  uint32_t k, s;
  if (!list_site(count, c, k, s)) return;
  const uint32_t v = nodes[k], p = (uint32_t)T.parent[v];
  down_site(T.X, T.xexp, T.D, T.dexp, v, p, p == T.root, T.child_off, T.child, T.Plen, T.R, c, s);
}

__global__ __launch_bounds__(THREADS) void root_kernel(PlaceDev T, uint32_t c) {
  const uint32_t s = blockIdx.x * THREADS + threadIdx.x;
  if (s < c) root_site(T.rootv, T.rootexp, T.D, T.dexp, T.root, T.pi, T.weights, T.R, c, s);
}

__global__ __launch_bounds__(THREADS) void table_kernel(PlaceDev T, uint32_t c) {
  uint32_t k, s;
  if (!list_site(T.E, c, k, s)) return;
  table_site(T.T, T.texp, T.D, T.dexp, T.X, T.xexp, T.edges[k], T.Phalf, T.Ppend, T.pi, T.weights, T.rootv, T.R, c, s);
}

// A double and a 64-bit integer as their 32-bit halves through xlane.h's moves: `partner` of a lane under the DPP control, and the pair
// (own, partner) in some order after a v_permlane swap -- the order does not matter to a product or a sum.
template <int CTRL>
__device__ __forceinline__ double dpp_d(double v) {
  const int lo = __double2loint(v), hi = __double2hiint(v);
  return __hiloint2double(dpp_i<CTRL>(hi, hi), dpp_i<CTRL>(lo, lo));
}
template <int CTRL>
__device__ __forceinline__ long long dpp_ll(long long v) {
  const int lo = (int)(unsigned int)(unsigned long long)v, hi = (int)(unsigned int)((unsigned long long)v >> 32);
  return (long long)(((unsigned long long)(unsigned int)dpp_i<CTRL>(hi, hi) << 32) | (unsigned int)dpp_i<CTRL>(lo, lo));
}
template <bool HALF>
__device__ __forceinline__ void swap_pair(double m, long long e, double &ma, double &mb, long long &ea, long long &eb) {
  int x[4] = {__double2loint(m), __double2hiint(m), (int)(unsigned int)(unsigned long long)e, (int)(unsigned int)((unsigned long long)e >> 32)}, y[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    y[k] = x[k];
    if (HALF) swap32(x[k], y[k]); else swap16(x[k], y[k]);
  }
  ma = __hiloint2double(x[1], x[0]); mb = __hiloint2double(y[1], y[0]);
  ea = (long long)(((unsigned long long)(unsigned int)x[3] << 32) | (unsigned int)x[2]);
  eb = (long long)(((unsigned long long)(unsigned int)y[3] << 32) | (unsigned int)y[2]);
}

// the product of the sixty-four lanes' factors, in every lane (place_dev.h block_product): xlane.h's butterfly -- after the step with
// partner w all lanes of a 2w-group hold the same value, so the mirror moves pair exactly the operands the xor-4 / xor-8 steps pair
__device__ __forceinline__ Sc wave_product(Sc f) {
  double m = f.m;
  long long e = f.e;
#define PL_STEP(CTRL) { const double om = dpp_d<CTRL>(m); const long long oe = dpp_ll<CTRL>(e); m = m * om; e = e + oe; }
  PL_STEP(DPP_QUAD_XOR1) PL_STEP(DPP_QUAD_XOR2) PL_STEP(DPP_ROW_HALF_MIRROR) PL_STEP(DPP_ROW_MIRROR)
#undef PL_STEP
  { double ma, mb; long long ea, eb; swap_pair<false>(m, e, ma, mb, ea, eb); m = ma * mb; e = ea + eb; }
  { double ma, mb; long long ea, eb; swap_pair<true>(m, e, ma, mb, ea, eb); m = ma * mb; e = ea + eb; }
  Sc p = norm(m);
  if (p.m != 0.0) p.e += e;
  return p;
}

__global__ __launch_bounds__(WAVE * SCAN_WAVES) void scan_kernel(PlaceDev T, uint32_t s0, uint32_t c) {
  __shared__ double tile[NQ][SCAN_SITES];
  __shared__ int32_t tex[SCAN_SITES], rex[SCAN_SITES];
  const uint32_t e = T.edges[blockIdx.x], q0 = blockIdx.y * SCAN_QUERIES, q1 = min(T.NQy, q0 + SCAN_QUERIES);
  const uint32_t lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  for (uint32_t t0 = 0; t0 < c; t0 += SCAN_SITES) {
    __syncthreads();                                            // the previous tile's readers
    for (uint32_t idx = threadIdx.x; idx < NQ * SCAN_SITES; idx += WAVE * SCAN_WAVES) {
      const uint32_t q = idx / SCAN_SITES, s = idx % SCAN_SITES;
      tile[q][s] = t0 + s < c ? T.T[((uint64_t)e * NQ + q) * c + t0 + s] : 1.0;
    }
    for (uint32_t s = threadIdx.x; s < SCAN_SITES; s += WAVE * SCAN_WAVES) {
      tex[s] = t0 + s < c ? T.texp[(uint64_t)e * c + t0 + s] : 0;
      rex[s] = t0 + s < c ? T.rootexp[t0 + s] : 0;
    }
    __syncthreads();
    for (uint32_t q = q0 + wave; q < q1; q += SCAN_WAVES) {
      const uint64_t at = (uint64_t)e * T.NQy + q;
      Sc run;
      run.m = T.acc_m[at]; run.e = T.acc_e[at];
      for (uint32_t b = 0; b < SCAN_SITES && t0 + b < c; b += WAVE) {
        const uint32_t s = t0 + b + lane;
        const bool live = s < c;
        const uint32_t code = live ? T.qcode[(uint64_t)q * T.S + s0 + s] : 0u;
        run = mul(run, wave_product(lane_factor(live, tile[code][b + lane], code == (uint32_t)NS ? rex[b + lane] : tex[b + lane])));
      }
      if (lane == 0) { T.acc_m[at] = run.m; T.acc_e[at] = run.e; }
    }
  }
}

// a before b in the order of the kept list: the larger first, ties to the lower position (the lower edge number)
__device__ __forceinline__ bool before(Sc a, uint32_t apos, Sc b, uint32_t bpos) { return gt(a, b) || (!gt(b, a) && apos < bpos); }

__global__ __launch_bounds__(THREADS) void topk_kernel(PlaceDev T) {
  __shared__ double sm[THREADS];
  __shared__ long long se[THREADS];
  __shared__ uint32_t sp[THREADS];
  const uint32_t q = blockIdx.x, NONE = 0xffffffffu;
  Sc prev = one();
  uint32_t prev_pos = NONE;
  for (uint32_t k = 0; k < T.Keff; ++k) {
    Sc best = one();
    uint32_t best_pos = NONE;
    for (uint32_t pos = threadIdx.x; pos < T.E; pos += THREADS) {
      Sc v;
      v.m = T.acc_m[(uint64_t)T.edges[pos] * T.NQy + q]; v.e = T.acc_e[(uint64_t)T.edges[pos] * T.NQy + q];
      if (prev_pos != NONE && !before(prev, prev_pos, v, pos)) continue;
      if (best_pos == NONE || gt(v, best)) { best = v; best_pos = pos; }
    }
    sm[threadIdx.x] = best.m; se[threadIdx.x] = best.e; sp[threadIdx.x] = best_pos;
    __syncthreads();
    for (uint32_t d = THREADS / 2; d > 0; d >>= 1) {
      if (threadIdx.x < d && sp[threadIdx.x + d] != NONE) {
        Sc a, b;
        a.m = sm[threadIdx.x]; a.e = se[threadIdx.x]; b.m = sm[threadIdx.x + d]; b.e = se[threadIdx.x + d];
        if (sp[threadIdx.x] == NONE || before(b, sp[threadIdx.x + d], a, sp[threadIdx.x])) { sm[threadIdx.x] = b.m; se[threadIdx.x] = b.e; sp[threadIdx.x] = sp[threadIdx.x + d]; }
      }
      __syncthreads();
    }
    prev.m = sm[0]; prev.e = se[0]; prev_pos = sp[0];
    __syncthreads();                                            // everybody has the pick before the next round overwrites it
    if (threadIdx.x == 0) {
      const uint64_t at = (uint64_t)q * T.K + k;
      T.top_edge[at] = (int32_t)T.edges[prev_pos]; T.scan_m[at] = prev.m; T.scan_e[at] = prev.e;
    }
  }
}

__global__ __launch_bounds__(WAVE) void refine_kernel(PlaceDev T, uint32_t s0, uint32_t c) {
  __shared__ double val[MAX_PEND][WAVE];
  const uint32_t pair = blockIdx.x, q = pair / T.Keff, k = pair % T.Keff, lane = threadIdx.x;
  const uint32_t e = (uint32_t)T.top_edge[(uint64_t)q * T.K + k];
  for (uint32_t f = 0; f < T.F; ++f) {
    const double *Pd = T.Pdist + ((((uint64_t)e * T.F + f) * 2 + 0) * T.R) * PM, *Pp = T.Pdist + ((((uint64_t)e * T.F + f) * 2 + 1) * T.R) * PM;
    for (uint32_t b = 0; b < c; b += WAVE) {
      const uint32_t s = b + lane;
      const bool live = s < c;
      const int code = live ? T.qcode[(uint64_t)q * T.S + s0 + s] : 0;
      if (live && code == NS) {
        for (uint32_t g = 0; g < T.G; ++g) val[g][lane] = T.rootv[s];
      } else if (live) {
        for (uint32_t r = 0; r < T.R; ++r) {
          double ab[NS];
          attach_rate(T.D, T.X, e, T.R, r, c, s, Pd + (uint64_t)r * PM, Pp + (uint64_t)r * PM, T.pi, ab);
          for (uint32_t g = 0; g < T.G; ++g) {
            const double tv = T.weights[r] * tip_inner(ab, T.Ppend + ((uint64_t)(g + 1) * T.R + r) * PM, code);
            val[g][lane] = r == 0 ? tv : val[g][lane] + tv;
          }
        }
      }
      const int32_t ex = !live ? 0 : code == NS ? T.rootexp[s] : T.dexp[(uint64_t)e * c + s] + T.xexp[(uint64_t)e * c + s];
      for (uint32_t g = 0; g < T.G; ++g) {
        const Sc p = wave_product(lane_factor(live, live ? val[g][lane] : 0.0, ex));
        const uint64_t at = ((uint64_t)pair * T.F + f) * T.G + g;
        if (lane == 0) {
          Sc ra;
          ra.m = T.racc_m[at]; ra.e = T.racc_e[at];
          ra = mul(ra, p);
          T.racc_m[at] = ra.m; T.racc_e[at] = ra.e;
        }
      }
    }
  }
}

__global__ __launch_bounds__(THREADS) void best_kernel(PlaceDev T) {
  const uint64_t pair = (uint64_t)blockIdx.x * THREADS + threadIdx.x;
  if (pair >= (uint64_t)T.NQy * T.Keff) return;
  const uint32_t FG = T.F * T.G;
  uint32_t best = 0;
  Sc bv;
  bv.m = T.racc_m[pair * FG]; bv.e = T.racc_e[pair * FG];
  for (uint32_t fg = 1; fg < FG; ++fg) {
    Sc v;
    v.m = T.racc_m[pair * FG + fg]; v.e = T.racc_e[pair * FG + fg];
    if (gt(v, bv)) { bv = v; best = fg; }
  }
  const uint64_t at = (pair / T.Keff) * T.K + pair % T.Keff;
  T.ref_m[at] = bv.m; T.ref_e[at] = bv.e; T.ref_f[at] = (int32_t)(best / T.G); T.ref_g[at] = (int32_t)(best % T.G);
}

static uint32_t blocks_for(uint64_t n) { return (uint32_t)((n + THREADS - 1) / THREADS); }
static uint64_t padded(uint32_t count, uint32_t c) { return (uint64_t)count * ((c + WAVE - 1) / WAVE * WAVE); }

void launch_place_pmat(hipStream_t st, const double *U, const double *Ui, const double *ex, double *P, uint64_t nmat) {
  if (nmat) hipLaunchKernelGGL(pmat_kernel, dim3(blocks_for(nmat * PM)), dim3(THREADS), 0, st, U, Ui, ex, P, nmat);
}
void launch_place_fill(hipStream_t st, double *m, long long *e, uint64_t n) {
  if (n) hipLaunchKernelGGL(fill_one_kernel, dim3(blocks_for(n)), dim3(THREADS), 0, st, m, e, n);
}
void launch_place_up(hipStream_t st, const PlaceDev &T, const uint32_t *nodes, uint32_t count, uint32_t s0, uint32_t c) {
  if (count) hipLaunchKernelGGL(up_level_kernel, dim3(blocks_for(padded(count, c))), dim3(THREADS), 0, st, T, nodes, count, s0, c);
}
void launch_place_down(hipStream_t st, const PlaceDev &T, const uint32_t *nodes, uint32_t count, uint32_t c) {
  if (count) hipLaunchKernelGGL(down_level_kernel, dim3(blocks_for(padded(count, c))), dim3(THREADS), 0, st, T, nodes, count, c);
}
void launch_place_root(hipStream_t st, const PlaceDev &T, uint32_t c) {
  hipLaunchKernelGGL(root_kernel, dim3(blocks_for(c)), dim3(THREADS), 0, st, T, c);
}
void launch_place_table(hipStream_t st, const PlaceDev &T, uint32_t c) {
  hipLaunchKernelGGL(table_kernel, dim3(blocks_for(padded(T.E, c))), dim3(THREADS), 0, st, T, c);
}
void launch_place_scan(hipStream_t st, const PlaceDev &T, uint32_t s0, uint32_t c) {
  if (T.NQy) hipLaunchKernelGGL(scan_kernel, dim3(T.E, (T.NQy + SCAN_QUERIES - 1) / SCAN_QUERIES), dim3(WAVE * SCAN_WAVES), 0, st, T, s0, c);
}
void launch_place_topk(hipStream_t st, const PlaceDev &T) {
  if (T.NQy) hipLaunchKernelGGL(topk_kernel, dim3(T.NQy), dim3(THREADS), 0, st, T);
}
void launch_place_refine(hipStream_t st, const PlaceDev &T, uint32_t s0, uint32_t c) {
  if (T.NQy) hipLaunchKernelGGL(refine_kernel, dim3(T.NQy * T.Keff), dim3(WAVE), 0, st, T, s0, c);
}
void launch_place_best(hipStream_t st, const PlaceDev &T) {
  if (T.NQy) hipLaunchKernelGGL(best_kernel, dim3(blocks_for((uint64_t)T.NQy * T.Keff)), dim3(THREADS), 0, st, T);
}

}  // namespace ckm
