// Posterior-mean Pareto front on the device (gfx950): a mean-only posterior kernel and NSGA-II (Deb et al. 2002)
// whose generations stay on the device.  The reference samples the front of the surrogate's posterior mean with
// pygmo.nsga2 at every BO iteration (modules/pareto/sample.py:16-48, bo_loop.py:294-332, 480-520), its fitness
// BoTorchModel.batch_fitness (sample.py:138-144) or GPTestProblem.evaluate_true (gp_testproblem.py:76-97).
//
//   posterior_mean_kernel   mean[p][i] = y_mean_i + y_std_i (c_i + K(x_p, X_i) alpha_i).  One workgroup per
//                           (16 points, output): X_i (pre-scaled by 1 / lengthscale, as the cross stage stages it)
//                           and alpha_i in LDS, one wave per point, lane l the training points l, l + 64, ... as one
//                           fma chain, then wave_sum's fixed-order reduction.  No atomics: a point's bits depend on
//                           the point alone, not on P or on its row.
//   pareto_rank_kernel      one workgroup: dominator counts, the front peel (fast non-dominated sort), crowding
//                           distances by rank-in-front scans (no sort: a member's neighbours in (f_j, index) order
//                           are the largest key below and the smallest key above its own), and the survivor order
//                           by counting the keys (rank, -crowding, index) below a point's own.  Every loop is
//                           bounded by Q; phases meet at __syncthreads.
//   pareto_clear / dom / peel / crowd / order kernels: the same results for up to 16384 points from the caller's
//                           workspace, the per-point scans spread over the device (the wide path, below).
//   pareto_variation_kernel binary tournament, bounded simulated binary crossover (Deb & Agrawal 1995) and bounded
//                           polynomial mutation (Deb et al. 2002), one thread per (pair of children, coordinate),
//                           every random number read from the caller's uniforms (layout: include/dkg.h).
//   pareto_init / normalise / gather: the glue of dkg_pareto_nsga2.
// The three stages' arithmetic is compiled without FP contraction where a host restatement must give the same bits
// (crowding) or nearly so (variation).
#include <atomic>
#include <cstdarg>
#include <cstdio>

#include "dkg_pareto_dev.h"

namespace dkg {

constexpr int PM_WAVES = 4;   // waves per workgroup of posterior_mean_kernel
constexpr int PM_POINTS = 16; // points per workgroup (4 per wave, one after the other)

struct MeanArgs {
  Outputs outs;
  int m, d, P;
  const double* x;  // [P][d] model inputs
  double* mean;     // [P][m]
};

__host__ __device__ inline size_t mean_lds_bytes(int n, int d) { return (size_t)n * (d + 1) * sizeof(double); }

template <int DM>
__global__ __launch_bounds__(PM_WAVES* WAVE) void posterior_mean_kernel(MeanArgs a) {
  extern __shared__ __attribute__((aligned(16))) double pm_smem[];
  const dkg_output& o = a.outs.o[blockIdx.y];
  const int n = o.n, d = a.d;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double* xs = pm_smem;                // [n][d] training inputs / lengthscale
  double* als = pm_smem + (size_t)n * d;  // [n]
  for (int e = tid; e < n * d; e += PM_WAVES * WAVE) xs[e] = o.train_x[e] * o.inv_lengthscale[e % d];
  for (int e = tid; e < n; e += PM_WAVES * WAVE) als[e] = o.alpha[e];
  __syncthreads();
  const double os = o.outputscale;
  const int iters = (n + WAVE - 1) / WAVE;  // wave-uniform trip count
  const int p0 = blockIdx.x * PM_POINTS;
  for (int q = wave; q < PM_POINTS; q += PM_WAVES) {
    const int p = p0 + q;
    if (p >= a.P) break;  // wave-uniform
    double xr[DM];
#pragma unroll
    for (int k = 0; k < DM; ++k) {
      const int kk = min(k, d - 1);
      xr[k] = a.x[(size_t)p * d + kk] * o.inv_lengthscale[kk];
    }
    double acc = 0.0;
    auto chain = [&](auto kind_c) {
      constexpr int KIND = decltype(kind_c)::value;
      const const_dptr tab = psi_tab();
      for (int it = 0; it < iters; ++it) {
        const int j = lane + it * WAVE;
        const int jc = min(j, n - 1);
        const double kv = cross_kernel_term<DM, KIND>(xr, xs + (size_t)jc * d, d, os, tab);
        acc = fma((j < n) ? kv : 0.0, als[jc], acc);
      }
    };
    switch (o.kernel) {
      case DKG_MATERN12: chain(std::integral_constant<int, DKG_MATERN12>{}); break;
      case DKG_MATERN32: chain(std::integral_constant<int, DKG_MATERN32>{}); break;
      case DKG_RBF: chain(std::integral_constant<int, DKG_RBF>{}); break;
      default: chain(std::integral_constant<int, DKG_MATERN52>{}); break;
    }
    const double s = wave_sum(acc);
    if (lane == 0) a.mean[(size_t)p * a.m + blockIdx.y] = fma(o.y_std, o.mean_constant + s, o.y_mean);
  }
}

static hipError_t launch_mean(const MeanArgs& a, hipStream_t s) {
  int nmax = 1;
  for (int i = 0; i < a.m; ++i) nmax = std::max(nmax, (int)a.outs.o[i].n);
  const size_t lds = mean_lds_bytes(nmax, a.d);
  const dim3 grid((a.P + PM_POINTS - 1) / PM_POINTS, a.m), block(PM_WAVES * WAVE);
  auto go = [&](auto kern) {
    raise_lds_limit(reinterpret_cast<const void*>(kern), lds);
    hipLaunchKernelGGL(kern, grid, block, lds, s, a);
  };
  switch (dim_bucket(a.d)) {
    case 2: go(posterior_mean_kernel<2>); break;
    case 4: go(posterior_mean_kernel<4>); break;
    case 8: go(posterior_mean_kernel<8>); break;
    default: go(posterior_mean_kernel<16>); break;
  }
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------
// Ranks, crowding distances and survivor order of Q <= 2048 points in one workgroup (pareto_rank_body,
// dkg_pareto_dev.h).
template <int MB>
__global__ __launch_bounds__(1024) void pareto_rank_kernel(const double* __restrict__ F, int Q, int m, int keep,
                                                           int* __restrict__ rank, double* __restrict__ crowd,
                                                           int* __restrict__ order) {
  extern __shared__ __attribute__((aligned(16))) double pr_smem[];
  pareto_rank_body<MB>(F, Q, m, keep, rank, crowd, order, pr_smem);
}

static hipError_t launch_rank(const double* F, int Q, int m, int keep, int* rank, double* crowd, int* order,
                              hipStream_t s) {
  const size_t lds = rank_lds_bytes(Q, m);
  const int nt = rank_threads(Q);
  auto go = [&](auto kern) {
    raise_lds_limit(reinterpret_cast<const void*>(kern), lds);
    hipLaunchKernelGGL(kern, dim3(1), dim3(nt), lds, s, F, Q, m, keep, rank, crowd, order);
  };
  if (m <= 2) go(pareto_rank_kernel<2>);
  else if (m <= 4) go(pareto_rank_kernel<4>);
  else go(pareto_rank_kernel<8>);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------
// The wide path: the same ranks, crowding distances and order for Q <= 16384 points, the per-point work spread
// over the device.  Five stream-ordered launches, no workgroup waits on another:
//   pareto_clear_kernel   cnt = 0, rk = -2, order = -1, the scalars (every call: the workspace carries no state)
//   pareto_dom_kernel     grid (point tiles, k slices): a thread holds its point's row in registers, the slice's
//                         rows are LDS broadcasts, the partial dominator count goes to cnt[i] by an integer
//                         atomicAdd (an integer sum does not depend on the arrival order)
//   pareto_peel_kernel    one workgroup, the only sequential part: fronts from cnt until `keep` points are ranked
//   pareto_crowd_kernel   one wave per point: a front's min / max and a member's neighbours in (f_j, index) order
//                         are selections of input values, so the wave reduction gives the one-workgroup kernel's
//                         values; then its arithmetic
//   pareto_order_kernel   one wave per point: an integer wave sum of the keys below its own
// Scratch (the caller's workspace): cnt [Q], rk [Q] ints, 64 scalars' room.
constexpr int WR_MAXQ = 16384;
constexpr int PD_TILE = 256;   // points per workgroup of pareto_dom_kernel, one per thread
constexpr int PD_SLICE = 128;  // rows k per workgroup: Q = 2000 gives 8 x 16 workgroups
constexpr int WR_WAVES = 4;    // waves (points) per workgroup of the crowding and order kernels
constexpr size_t WR_LDS = 160 * 1024;

struct WideWs {
  size_t cnt, rk, scalars, total;
};
__host__ inline WideWs wide_ws(int Q) {
  WideWs w{};
  const size_t q = ((size_t)Q * sizeof(int) + 255) & ~(size_t)255;
  w.cnt = 0;
  w.rk = q;
  w.scalars = 2 * q;
  w.total = 2 * q + 256;
  return w;
}

// pareto_peel_kernel's LDS: the unranked dominator counts [Q], the front's member list [Q], two counters, and
// F [Q][m] where it fits beside them
__host__ __device__ inline size_t peel_list_bytes(int Q) {
  return (2 * (size_t)Q * sizeof(int) + 16 + 15) & ~(size_t)15;
}
__host__ __device__ inline bool peel_f_in_lds(int Q, int m) {
  return peel_list_bytes(Q) + (size_t)Q * m * sizeof(double) <= WR_LDS;
}

__global__ __launch_bounds__(256) void pareto_clear_kernel(int Q, int* __restrict__ cnt, int* __restrict__ rk,
                                                           int* __restrict__ scalars, int* __restrict__ order) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < Q) {
    cnt[i] = 0;
    rk[i] = -2;
    order[i] = -1;
  }
  if (i < 64) scalars[i] = 0;
}

template <int MB>
__global__ __launch_bounds__(PD_TILE) void pareto_dom_kernel(const double* __restrict__ F, int Q, int m,
                                                             int* __restrict__ cnt) {
  __shared__ __attribute__((aligned(16))) double rows[PD_SLICE * MB];  // the slice's rows, padded to MB as load_row
  const int tid = threadIdx.x;
  const int k0 = blockIdx.y * PD_SLICE, kn = min(PD_SLICE, Q - k0);
  for (int e = tid; e < kn * MB; e += PD_TILE) rows[e] = F[(size_t)(k0 + e / MB) * m + min(e % MB, m - 1)];
  __syncthreads();
  const int i = blockIdx.x * PD_TILE + tid;
  double own[MB];  // a thread past Q holds row Q - 1 and writes nothing
  load_row<MB>(F, min(i, Q - 1), m, own);
  int c = 0;
#pragma unroll 4
  for (int k = 0; k < kn; ++k) {
    double fk[MB];
#pragma unroll
    for (int j = 0; j < MB; ++j) fk[j] = rows[k * MB + j];
    c += dominates<MB>(fk, own) ? 1 : 0;
  }
  if (i < Q && c) atomicAdd(&cnt[i], c);
}

// One workgroup; thread t owns the points t, t + nt, ... (16 of them at Q = 16384), their unranked dominator
// counts in LDS: > 0 dominated, 0 a member of the next front, -1 ranked.  Per round: the members list
// themselves, `done >= keep` is tested, and only when the peel goes on are the members' dominations taken off
// the unranked counts (with keep = P of 2P points and a first front of >= P members the peel is one round with no
// scan).  LDSF: F is staged in LDS; otherwise its rows are read from global memory (<= 1 MiB, L2 resident).
template <int MB, bool LDSF>
__global__ __launch_bounds__(1024) void pareto_peel_kernel(const double* __restrict__ F, int Q, int m, int keep,
                                                           const int* __restrict__ cnt0, int* __restrict__ rk,
                                                           int* __restrict__ scalars) {
  extern __shared__ __attribute__((aligned(16))) double pp_smem[];
  int* cnt = reinterpret_cast<int*>(pp_smem);  // [Q]
  int* list = cnt + Q;                         // [Q] members of the front being peeled
  int* nmem = list + Q;                        // [2] members of the front of an even / odd round
  const double* f = F;
  const int tid = threadIdx.x, nt = blockDim.x;
  if constexpr (LDSF) {
    double* fs = reinterpret_cast<double*>(reinterpret_cast<char*>(pp_smem) + peel_list_bytes(Q));
    for (int e = tid; e < Q * m; e += nt) fs[e] = F[e];
    f = fs;
  }
  if (tid < 2) nmem[tid] = 0;
  for (int i = tid; i < Q; i += nt) cnt[i] = cnt0[i];
  __syncthreads();
  int done = 0, fronts = 0;
  for (int r = 0; r < Q; ++r) {
    int* mine = nmem + (r & 1);
    for (int i = tid; i < Q; i += nt)
      if (cnt[i] == 0) list[atomicAdd(mine, 1)] = i;  // any order: only counted over
    __syncthreads();
    const int nf = *mine;
    if (tid == 0) nmem[(r + 1) & 1] = 0;  // last read before the previous round's closing barrier
    done += nf;
    fronts += nf > 0 ? 1 : 0;
    const bool last = done >= keep || nf == 0;  // uniform
    for (int i = tid; i < Q; i += nt) {
      const int ci = cnt[i];  // the thread's own points: no other thread reads or writes them
      if (ci == 0) {
        rk[i] = r;
        cnt[i] = -1;
      } else if (ci > 0 && !last) {
        double own[MB];
        load_row<MB>(f, i, m, own);
        int c = 0;
#pragma unroll 4
        for (int q = 0; q < nf; ++q) {
          double fk[MB];
          load_row<MB>(f, list[q], m, fk);
          c += dominates<MB>(fk, own) ? 1 : 0;
        }
        cnt[i] = ci - c;
      }
    }
    if (last) break;
    __syncthreads();  // the list is free for the next round
  }
  if (tid == 0) {
    scalars[0] = fronts;
    scalars[1] = done;
  }
}

__global__ __launch_bounds__(WR_WAVES* WAVE) void pareto_crowd_kernel(const double* __restrict__ F, int Q, int m,
                                                                      const int* __restrict__ rk,
                                                                      int* __restrict__ rank,
                                                                      double* __restrict__ crowd) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * WR_WAVES + (threadIdx.x >> 6);
  if (i >= Q) return;  // wave-uniform, as every branch below
  const int ri = rk[i];
  if (ri < 0) {
    if (lane == 0) {
      rank[i] = -1;
      crowd[i] = 0.0;
    }
    return;
  }
  double cd = 0.0;
  for (int j = 0; j < m; ++j) {
    const double fi = F[(size_t)i * m + j];
    double fmin = fi, fmax = fi, prev = 0.0, next = 0.0;
    bool hp = false, hn = false;
#pragma unroll 2
    for (int k = lane; k < Q; k += WAVE) {
      const bool in = rk[k] == ri;
      const double fk = F[(size_t)k * m + j];
      fmin = (in && fk < fmin) ? fk : fmin;
      fmax = (in && fk > fmax) ? fk : fmax;
      const bool before = in && (fk < fi || (fk == fi && k < i));
      const bool after = in && (fk > fi || (fk == fi && k > i));
      prev = (before && (!hp || fk > prev)) ? fk : prev;
      next = (after && (!hn || fk < next)) ? fk : next;
      hp = hp || before;
      hn = hn || after;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double omin = __shfl_xor(fmin, off), omax = __shfl_xor(fmax, off);
      const double oprev = __shfl_xor(prev, off), onext = __shfl_xor(next, off);
      const bool ohp = __shfl_xor((int)hp, off) != 0, ohn = __shfl_xor((int)hn, off) != 0;
      fmin = omin < fmin ? omin : fmin;
      fmax = omax > fmax ? omax : fmax;
      prev = (ohp && (!hp || oprev > prev)) ? oprev : prev;
      next = (ohn && (!hn || onext < next)) ? onext : next;
      hp = hp || ohp;
      hn = hn || ohn;
    }
    if (!hp || !hn) {
      cd = cd + __builtin_inf();
    } else {
      const double range = fmax - fmin;
      const double num = next - prev;
      cd = cd + (range > 0.0 ? num / range : 0.0);
    }
  }
  if (lane == 0) {
    rank[i] = ri;
    crowd[i] = cd;
  }
}

// order[pos] = i, pos the number of ranked points whose key (rank, -crowding, index) is below i's: < Q whatever
// the values
__global__ __launch_bounds__(WR_WAVES* WAVE) void pareto_order_kernel(int Q, const int* __restrict__ rank,
                                                                      const double* __restrict__ crowd,
                                                                      int* __restrict__ order) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * WR_WAVES + (threadIdx.x >> 6);
  if (i >= Q) return;  // wave-uniform
  const int ri = rank[i];
  if (ri < 0) return;
  const double ci = crowd[i];
  int pos = 0;
#pragma unroll 2
  for (int k = lane; k < Q; k += WAVE) {
    const int rkk = rank[k];
    const double ck = crowd[k];
    const bool before = rkk >= 0 && (rkk < ri || (rkk == ri && (ck > ci || (ck == ci && k < i))));
    pos += before ? 1 : 0;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) pos += __shfl_xor(pos, off);
  if (lane == 0) order[pos] = i;
}

static hipError_t launch_rank_wide(const double* F, int Q, int m, int keep, int* rank, double* crowd, int* order,
                                   void* work, hipStream_t s) {
  const WideWs w = wide_ws(Q);
  char* ws = static_cast<char*>(work);
  int* cnt = reinterpret_cast<int*>(ws + w.cnt);
  int* rk = reinterpret_cast<int*>(ws + w.rk);
  int* scalars = reinterpret_cast<int*>(ws + w.scalars);
  hipError_t e;
  hipLaunchKernelGGL(pareto_clear_kernel, dim3((std::max(Q, 64) + 255) / 256), dim3(256), 0, s, Q, cnt, rk, scalars,
                     order);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  const dim3 dgrid((Q + PD_TILE - 1) / PD_TILE, (Q + PD_SLICE - 1) / PD_SLICE);
  if (m <= 2) hipLaunchKernelGGL(pareto_dom_kernel<2>, dgrid, dim3(PD_TILE), 0, s, F, Q, m, cnt);
  else if (m <= 4) hipLaunchKernelGGL(pareto_dom_kernel<4>, dgrid, dim3(PD_TILE), 0, s, F, Q, m, cnt);
  else hipLaunchKernelGGL(pareto_dom_kernel<8>, dgrid, dim3(PD_TILE), 0, s, F, Q, m, cnt);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  const bool in_lds = peel_f_in_lds(Q, m);
  const size_t lds = peel_list_bytes(Q) + (in_lds ? (size_t)Q * m * sizeof(double) : 0);
  const int nt = std::min(1024, (Q + 63) / 64 * 64);
  auto peel = [&](auto kern) {
    raise_lds_limit(reinterpret_cast<const void*>(kern), lds);
    hipLaunchKernelGGL(kern, dim3(1), dim3(nt), lds, s, F, Q, m, keep, (const int*)cnt, rk, scalars);
  };
  if (m <= 2) in_lds ? peel(pareto_peel_kernel<2, true>) : peel(pareto_peel_kernel<2, false>);
  else if (m <= 4) in_lds ? peel(pareto_peel_kernel<4, true>) : peel(pareto_peel_kernel<4, false>);
  else in_lds ? peel(pareto_peel_kernel<8, true>) : peel(pareto_peel_kernel<8, false>);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  const dim3 wgrid((Q + WR_WAVES - 1) / WR_WAVES), wblock(WR_WAVES * WAVE);
  hipLaunchKernelGGL(pareto_crowd_kernel, wgrid, wblock, 0, s, F, Q, m, (const int*)rk, rank, crowd);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(pareto_order_kernel, wgrid, wblock, 0, s, Q, (const int*)rank, (const double*)crowd, order);
  return hipGetLastError();
}

// Which path ranks Q <= 2048 points when the caller gave a workspace: mode -1 the measured rule, 0 never the wide
// path, 1 always (dkg_debug_pareto_wide).  The rule: the smallest Q of the sweep (tools/bench_pareto.py
// --rank-sweep; Q = 8 .. 2048, keep = Q / 2, late- and early-generation-like inputs) from which the wide path's
// median is below the one-workgroup kernel's minimum on both inputs, per objective bucket (DESIGN.md 8c,
// profiles/pareto_wide/rank_sweep.json): five launches cost 17 - 22 us whatever Q is, the one workgroup 7 - 20 us
// at Q = 8 and 21 - 66 us at Q = 32.
static std::atomic<int> g_pareto_wide_mode{-1};
static int wide_min_q(int m) { return m <= 4 ? 32 : 16; }
static bool rank_goes_wide(int Q, int m, const void* work) {
  if (!work) return false;
  if (Q > PR_MAXQ) return true;
  const int mode = g_pareto_wide_mode.load(std::memory_order_relaxed);
  return mode == 1 || (mode < 0 && Q >= wide_min_q(m));
}
static hipError_t launch_rank_any(const double* F, int Q, int m, int keep, int* rank, double* crowd, int* order,
                                  void* work, hipStream_t s) {
  return rank_goes_wide(Q, m, work) ? launch_rank_wide(F, Q, m, keep, rank, crowd, order, work, s)
                                    : launch_rank(F, Q, m, keep, rank, crowd, order, s);
}

// ---------------------------------------------------------------------------------------------------------------
// Variation: one thread per (pair of children, coordinate) of pareto_variation_body (dkg_pareto_dev.h).
__global__ __launch_bounds__(256) void pareto_variation_kernel(VarArgs a) {
  pareto_variation_body(a, blockIdx.x * blockDim.x + threadIdx.x);
}

static hipError_t launch_variation(const VarArgs& a, hipStream_t s) {
  const int total = a.P / 2 * a.d;
  hipLaunchKernelGGL(pareto_variation_kernel, dim3((total + 255) / 256), dim3(256), 0, s, a);
  return hipGetLastError();
}

// x[p][k] = lb[k] + u[p][k] (ub[k] - lb[k]), clipped into the bounds
__global__ __launch_bounds__(256) void pareto_init_kernel(const double* __restrict__ u, const double* __restrict__ lb,
                                                          const double* __restrict__ ub, int total, int d,
                                                          double* __restrict__ x) {
#pragma clang fp contract(off)
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int k = t % d;
  x[t] = clip(lb[k] + u[t] * (ub[k] - lb[k]), lb[k], ub[k]);
}

// xn = (x - lb) / (ub - lb): botorch's normalize (sample.py:129-130, 142)
__global__ __launch_bounds__(256) void pareto_normalise_kernel(const double* __restrict__ x,
                                                               const double* __restrict__ lb,
                                                               const double* __restrict__ ub, int total, int d,
                                                               double* __restrict__ xn) {
#pragma clang fp contract(off)
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int k = t % d;
  xn[t] = (x[t] - lb[k]) / (ub[k] - lb[k]);
}

struct GatherArgs {
  const int* order;     // [2 P], the first P entries the survivors
  const double *X2, *F2, *crowd2;
  const int* rank2;
  double *X, *F, *crowd;
  int* rank;
  int P, d, m;
};

// survivor r = point order[r] of [parents; children]
__global__ __launch_bounds__(256) void pareto_gather_kernel(GatherArgs a) {
  const int w = a.d + a.m + 2;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.P * w) return;
  const int r = t / w, c = t - r * w;
  const int src = a.order[r];
  if (src < 0 || src >= 2 * a.P) return;  // never for r < keep; keeps a bad order in bounds
  if (c < a.d) a.X[(size_t)r * a.d + c] = a.X2[(size_t)src * a.d + c];
  else if (c < a.d + a.m) a.F[(size_t)r * a.m + (c - a.d)] = a.F2[(size_t)src * a.m + (c - a.d)];
  else if (c == a.d + a.m) a.rank[r] = a.rank2[src];
  else a.crowd[r] = a.crowd2[src];
}

}  // namespace dkg

using namespace dkg;

namespace {

int pfail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  return report_error(code, buf);
}

int phip(hipError_t e, const char* what) {
  return e == hipSuccess ? DKG_OK : pfail(DKG_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}

size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

int check_model(const dkg_output* outs, int m, int d) {
  if (!outs) return pfail(DKG_ERR_ARG, "NULL pointer");
  if (m < 1) return pfail(DKG_ERR_ARG, "m=%d outputs", m);
  if (m > DKG_MAX_OUTPUTS) return pfail(DKG_ERR_UNSUPPORTED, "m=%d outputs (supported <= %d)", m, DKG_MAX_OUTPUTS);
  if (d < 1) return pfail(DKG_ERR_ARG, "d=%d", d);
  if (d > DKG_MAX_DIM) return pfail(DKG_ERR_UNSUPPORTED, "d=%d (supported 1..%d)", d, DKG_MAX_DIM);
  for (int i = 0; i < m; ++i) {
    if (outs[i].n < 1) return pfail(DKG_ERR_ARG, "output %d: n=%d training points", i, outs[i].n);
    if (outs[i].n > 1024) return pfail(DKG_ERR_UNSUPPORTED, "output %d: n=%d > 1024 training points", i, outs[i].n);
    if (outs[i].kernel < DKG_MATERN12 || outs[i].kernel > DKG_RBF)
      return pfail(DKG_ERR_ARG, "output %d: kernel id %d", i, outs[i].kernel);
    if (!outs[i].inv_lengthscale || !outs[i].train_x || !outs[i].alpha)
      return pfail(DKG_ERR_ARG, "output %d: NULL pointer", i);
  }
  return DKG_OK;
}

int check_population(int P) {
  if (P < 8 || P % 4) return pfail(DKG_ERR_ARG, "population P=%d (a multiple of 4, at least 8)", P);
  if (P > 1024) return pfail(DKG_ERR_UNSUPPORTED, "population P=%d (supported <= 1024)", P);
  return DKG_OK;
}

int check_params(const dkg_nsga2_params* p) {
  if (!p) return pfail(DKG_ERR_ARG, "NULL pointer");
  if (!(p->cr >= 0.0 && p->cr <= 1.0) || !(p->m >= 0.0 && p->m <= 1.0) || !(p->eta_c >= 0.0) || !(p->eta_m >= 0.0))
    return pfail(DKG_ERR_ARG, "nsga2 parameters cr=%g eta_c=%g m=%g eta_m=%g", p->cr, p->eta_c, p->m, p->eta_m);
  return DKG_OK;
}

MeanArgs mean_args(const dkg_output* outs, int m, int d, const double* x, int P, double* mean) {
  MeanArgs a{};
  for (int i = 0; i < m; ++i) a.outs.o[i] = outs[i];
  a.m = m;
  a.d = d;
  a.P = P;
  a.x = x;
  a.mean = mean;
  return a;
}

// dkg_pareto_nsga2's workspace carve
struct NsgaWs {
  size_t x2, f2, xn, crowd2, rank2, order, wide, total;
};
NsgaWs nsga_ws(int P, int d, int m) {
  NsgaWs w{};
  size_t off = 0;
  w.x2 = off;
  off = up256(off + 2 * (size_t)P * d * sizeof(double));
  w.f2 = off;
  off = up256(off + 2 * (size_t)P * m * sizeof(double));
  w.xn = off;
  off = up256(off + (size_t)P * d * sizeof(double));
  w.crowd2 = off;
  off = up256(off + 2 * (size_t)P * sizeof(double));
  w.rank2 = off;
  off = up256(off + 2 * (size_t)P * sizeof(int));
  w.order = off;
  off = up256(off + 2 * (size_t)P * sizeof(int));
  w.wide = off;  // the wide rank's scratch for the 2P points of a generation
  off = up256(off + wide_ws(2 * P).total);
  w.total = off;
  return w;
}

}  // namespace

extern "C" {

int dkg_posterior_mean(const dkg_output* outs, int m, int d, const double* x, int P, double* mean, void* stream) {
  int st = check_model(outs, m, d);
  if (st) return st;
  if (P < 0 || P > (1 << 24)) return pfail(DKG_ERR_ARG, "P=%d points", P);
  if (P == 0) return DKG_OK;
  if (!x || !mean) return pfail(DKG_ERR_ARG, "NULL pointer");
  return phip(launch_mean(mean_args(outs, m, d, x, P, mean), (hipStream_t)stream), "posterior_mean_kernel");
}

size_t dkg_pareto_rank_workspace(int Q, int m) {
  if (Q < 1 || Q > WR_MAXQ || m < 1 || m > DKG_MAX_OUTPUTS) return 0;
  return wide_ws(Q).total;
}

int dkg_pareto_rank(const double* F, int Q, int m, int keep, int* rank, double* crowd, int* order, void* work,
                    size_t work_bytes, void* stream) {
  if (Q < 1 || m < 1 || keep < 1 || keep > Q) return pfail(DKG_ERR_ARG, "Q=%d m=%d keep=%d", Q, m, keep);
  if (Q > (work ? WR_MAXQ : PR_MAXQ))
    return pfail(DKG_ERR_UNSUPPORTED, "Q=%d points (supported <= %d, <= %d with a workspace)", Q, PR_MAXQ, WR_MAXQ);
  if (m > DKG_MAX_OUTPUTS) return pfail(DKG_ERR_UNSUPPORTED, "m=%d objectives (supported <= %d)", m, DKG_MAX_OUTPUTS);
  if (!F || !rank || !crowd || !order) return pfail(DKG_ERR_ARG, "NULL pointer");
  if (work && work_bytes < wide_ws(Q).total)
    return pfail(DKG_ERR_WORKSPACE, "workspace %zu bytes < required %zu", work_bytes, wide_ws(Q).total);
  return phip(launch_rank_any(F, Q, m, keep, rank, crowd, order, work, (hipStream_t)stream), "dkg_pareto_rank");
}

int dkg_debug_pareto_wide(int mode) {
  if (mode < -1 || mode > 1) {
    pfail(DKG_ERR_ARG, "dkg_debug_pareto_wide: mode=%d (-1 the rule, 0 never below %d points, 1 always)", mode,
          PR_MAXQ + 1);
    return -2;
  }
  return g_pareto_wide_mode.exchange(mode, std::memory_order_relaxed);
}

size_t dkg_pareto_draws(int P, int d) {
  if (P < 2 || P % 2 || d < 1) return 0;
  const size_t H = P / 2;
  return 2 * (size_t)P + H + 3 * H * d + 2 * (size_t)P * d;
}

int dkg_pareto_variation(const double* X, const int* rank, const double* crowd, int P, int d, const double* lb,
                         const double* ub, const dkg_nsga2_params* prm, const double* uniforms, double* children,
                         void* stream) {
  int st = check_population(P);
  if (st) return st;
  if (d < 1) return pfail(DKG_ERR_ARG, "d=%d", d);
  if (d > DKG_MAX_DIM) return pfail(DKG_ERR_UNSUPPORTED, "d=%d (supported 1..%d)", d, DKG_MAX_DIM);
  if ((st = check_params(prm))) return st;
  if (!X || !rank || !crowd || !lb || !ub || !uniforms || !children) return pfail(DKG_ERR_ARG, "NULL pointer");
  VarArgs a{X, rank, crowd, lb, ub, uniforms, children, P, d, prm->cr, prm->eta_c, prm->m, prm->eta_m};
  return phip(launch_variation(a, (hipStream_t)stream), "pareto_variation_kernel");
}

size_t dkg_pareto_workspace(int P, int d, int m) {
  if (P < 8 || P % 4 || P > 1024 || d < 1 || d > DKG_MAX_DIM || m < 1 || m > DKG_MAX_OUTPUTS) return 0;
  return nsga_ws(P, d, m).total;
}

int dkg_pareto_nsga2(const dkg_output* outs, int m, int d, const double* lb, const double* ub, int P, int gens,
                     const dkg_nsga2_params* prm, const double* uniforms, double* X, double* F, int* rank,
                     double* crowd, void* work, size_t work_bytes, void* stream) {
  int st = check_model(outs, m, d);
  if (st) return st;
  if ((st = check_population(P))) return st;
  if (gens < 0 || gens > (1 << 20)) return pfail(DKG_ERR_ARG, "gens=%d generations", gens);
  if ((st = check_params(prm))) return st;
  if (!lb || !ub || !uniforms || !X || !F || !rank || !crowd || !work) return pfail(DKG_ERR_ARG, "NULL pointer");
  const NsgaWs w = nsga_ws(P, d, m);
  if (work_bytes < w.total) return pfail(DKG_ERR_WORKSPACE, "workspace %zu bytes < required %zu", work_bytes, w.total);
  hipStream_t s = (hipStream_t)stream;
  char* ws = static_cast<char*>(work);
  double* X2 = reinterpret_cast<double*>(ws + w.x2);
  double* F2 = reinterpret_cast<double*>(ws + w.f2);
  double* Xn = reinterpret_cast<double*>(ws + w.xn);
  double* crowd2 = reinterpret_cast<double*>(ws + w.crowd2);
  int* rank2 = reinterpret_cast<int*>(ws + w.rank2);
  int* order = reinterpret_cast<int*>(ws + w.order);
  void* wide = ws + w.wide;
  const int Pd = P * d, gb = (Pd + 255) / 256;
  const bool raw = prm->raw_inputs != 0;
  // evaluate `pts` (device [P][d], in the bounds) into `out` [P][m]
  auto evaluate = [&](const double* pts, double* out) -> int {
    const double* xin = pts;
    if (!raw) {
      hipLaunchKernelGGL(pareto_normalise_kernel, dim3(gb), dim3(256), 0, s, pts, lb, ub, Pd, d, Xn);
      int e = phip(hipGetLastError(), "pareto_normalise_kernel");
      if (e) return e;
      xin = Xn;
    }
    return phip(launch_mean(mean_args(outs, m, d, xin, P, out), s), "posterior_mean_kernel");
  };
  hipLaunchKernelGGL(pareto_init_kernel, dim3(gb), dim3(256), 0, s, uniforms, lb, ub, Pd, d, X);
  if ((st = phip(hipGetLastError(), "pareto_init_kernel")) || (st = evaluate(X, F)) ||
      (st = phip(launch_rank_any(F, P, m, P, rank, crowd, order, wide, s), "pareto_rank_kernel")))
    return st;
  const size_t draws = dkg_pareto_draws(P, d);
  GatherArgs g{order, X2, F2, crowd2, rank2, X, F, crowd, rank, P, d, m};
  const int gt = P * (d + m + 2);
  for (int gen = 0; gen < gens; ++gen) {
    double* Xc = X2 + (size_t)Pd;
    double* Fc = F2 + (size_t)P * m;
    VarArgs a{X, rank, crowd, lb, ub, uniforms + Pd + (size_t)gen * draws, Xc, P, d, prm->cr, prm->eta_c, prm->m,
              prm->eta_m};
    if ((st = phip(hipMemcpyAsync(X2, X, (size_t)Pd * sizeof(double), hipMemcpyDeviceToDevice, s), "hipMemcpyAsync")) ||
        (st = phip(hipMemcpyAsync(F2, F, (size_t)P * m * sizeof(double), hipMemcpyDeviceToDevice, s),
                   "hipMemcpyAsync")) ||
        (st = phip(launch_variation(a, s), "pareto_variation_kernel")) || (st = evaluate(Xc, Fc)) ||
        (st = phip(launch_rank_any(F2, 2 * P, m, P, rank2, crowd2, order, wide, s), "pareto_rank_kernel")))
      return st;
    hipLaunchKernelGGL(pareto_gather_kernel, dim3((gt + 255) / 256), dim3(256), 0, s, g);
    if ((st = phip(hipGetLastError(), "pareto_gather_kernel"))) return st;
  }
  return DKG_OK;
}

}  // extern "C"
