// Pareto fronts on the device (gfx950): a mean-only posterior kernel and NSGA-II (Deb et al. 2002) whose generations
// stay on the device, for one population on a GP's posterior mean and for S populations side by side on S sample
// paths.  The reference samples the front of the surrogate's posterior mean with pygmo.nsga2 at every BO iteration
// (modules/pareto/sample.py:16-48, bo_loop.py:294-332, 480-520), its fitness BoTorchModel.batch_fitness
// (sample.py:138-144) or GPTestProblem.evaluate_true (gp_testproblem.py:76-97); for joint entropy search it runs
// pymoo's NSGA-II on each sample path, one after the other, and prunes the fronts by repeated crowding distance
// (modules/pareto/jes_sample_pareto.py:101-232).  Both are one generation driver here (evolve): the fitness is an
// Evaluator, the posterior mean below or dkg_rff.hip's paths.  Specification: include/dkg.h; DESIGN.md 8c, 8e.
//
//   posterior_mean_kernel   mean[p][i] = y_mean_i + y_std_i (c_i + K(x_p, X_i) alpha_i).  One workgroup per
//                           (16 points, output): X_i (pre-scaled by 1 / lengthscale, as the cross stage stages it)
//                           and alpha_i in LDS, one wave per point, lane l the training points l, l + 64, ... as one
//                           fma chain, then wave_sum's fixed-order reduction.  No atomics: a point's bits depend on
//                           the point alone, not on P or on its row.  The points as given, or mapped to the unit
//                           cube with lb / ub.
//   pareto_rank_kernel      one workgroup per sample: dominator counts, the front peel (fast non-dominated sort),
//                           crowding distances by rank-in-front scans (no sort: a member's neighbours in (f_j, index)
//                           order are the largest key below and the smallest key above its own), and the survivor
//                           order by counting the keys (rank, -crowding, index) below a point's own.  Every loop is
//                           bounded by Q; phases meet at __syncthreads.
//   pareto_clear / dom / peel / crowd / order kernels: the same results for up to 16384 points from the caller's
//                           workspace, the per-point scans spread over the device (the wide path, below).
//   pareto_variation_kernel binary tournament, bounded simulated binary crossover (Deb & Agrawal 1995) and bounded
//                           polynomial mutation (Deb et al. 2002), one thread per (pair of children, coordinate),
//                           every random number read from the caller's uniforms (layout: include/dkg.h); in a
//                           generation it also copies the parents into [parents; children].
//   pareto_init / gather    the rest of a generation; blockIdx.y the sample, as in the variation.
//   pareto_prune_kernel     one workgroup per sample: duplicates, then the member of smallest (crowding, index)
//                           retired until k are left, the crowding by the rank's own arithmetic (front_crowding)
// The three stages' arithmetic is compiled without FP contraction where a host restatement must give the same bits
// (crowding) or nearly so (variation).
#include <algorithm>
#include <atomic>
#include <cstdio>

#include "dkg_acq.h"
#include "dkg_stages.h"

namespace dkg {

constexpr int PM_WAVES = 4;   // waves per workgroup of posterior_mean_kernel
constexpr int PM_POINTS = 16; // points per workgroup (4 per wave, one after the other)

struct MeanArgs {
  Outputs outs;
  int m, d, P;
  const double* x;        // [P][d]
  const double *lb, *ub;  // not NULL: the model input is unit_cube(x, lb, ub); NULL: x itself
  double* mean;           // [P][m]
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
      const double xv = a.x[(size_t)p * d + kk];
      xr[k] = (a.lb ? unit_cube(xv, a.lb[kk], a.ub[kk]) : xv) * o.inv_lengthscale[kk];
    }
    double acc = 0.0;
    with_kind(o.kernel, [&](auto kind_c) {
      constexpr int KIND = decltype(kind_c)::value;
      const const_dptr tab = psi_tab();
      for (int it = 0; it < iters; ++it) {
        const int j = lane + it * WAVE;
        const int jc = min(j, n - 1);
        const double kv = cross_kernel_term<DM, KIND>(xr, xs + (size_t)jc * d, d, os, tab);
        acc = fma((j < n) ? kv : 0.0, als[jc], acc);
      }
    });
    const double s = wave_sum(acc);
    if (lane == 0) a.mean[(size_t)p * a.m + blockIdx.y] = fma(o.y_std, o.mean_constant + s, o.y_mean);
  }
}

static hipError_t launch_mean(const MeanArgs& a, hipStream_t s) {
  int nmax = 1;
  for (int i = 0; i < a.m; ++i) nmax = std::max(nmax, (int)a.outs.o[i].n);
  const size_t lds = mean_lds_bytes(nmax, a.d);
  const dim3 grid((a.P + PM_POINTS - 1) / PM_POINTS, a.m), block(PM_WAVES * WAVE);
  by_dim(a.d, [&](auto dm) { launch_lds(posterior_mean_kernel<decltype(dm)::value>, grid, block, lds, s, a); });
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------
// Ranks, crowding distances and survivor order of Q <= 2048 points in one workgroup; thread t owns the points
// t and t + blockDim.x.  LDS: F [Q][m], then rk [Q] and the current front's member list [Q].
constexpr int PR_MAXQ = 2048;
constexpr int PR_PPT = 2;  // points per thread

__host__ __device__ inline size_t rank_lds_bytes(int Q, int m) {
  return (size_t)Q * m * sizeof(double) + 2 * (size_t)Q * sizeof(int) + 16;
}

// Row i of f [Q][m] in MB >= m registers; the entries j >= m repeat entry m - 1 (clamped loads, no branches), which
// changes no dominance test.
template <int MB>
__device__ __forceinline__ void load_row(const double* f, int i, int m, double (&r)[MB]) {
#pragma unroll
  for (int j = 0; j < MB; ++j) r[j] = f[(size_t)i * m + min(j, m - 1)];
}

// a dominates b: a >= b in every objective and a > b in at least one (all maximised)
template <int MB>
__device__ __forceinline__ bool dominates(const double (&fa)[MB], const double (&fb)[MB]) {
  bool ge = true, gt = false;
#pragma unroll
  for (int j = 0; j < MB; ++j) {
    ge = ge && (fa[j] >= fb[j]);
    gt = gt || (fa[j] > fb[j]);
  }
  return ge && gt;
}

// Crowding distance of member i of the front {k : rk[k] == ri} of f [Q][m], objectives in order; one subtraction,
// division and addition per step
__device__ __forceinline__ double front_crowding(const double* f, const int* rk, int Q, int m, int i, int ri) {
#pragma clang fp contract(off)
  double cd = 0.0;
  for (int j = 0; j < m; ++j) {
    const double fi = f[(size_t)i * m + j];
    double fmin = fi, fmax = fi, prev = 0.0, next = 0.0;
    bool hp = false, hn = false;
#pragma unroll 4
    for (int k = 0; k < Q; ++k) {
      const bool in = rk[k] == ri;
      const double fk = f[(size_t)k * m + j];
      fmin = (in && fk < fmin) ? fk : fmin;
      fmax = (in && fk > fmax) ? fk : fmax;
      // before / after i in (f_j, index) order: the predecessor is the largest f before, the successor the
      // smallest f after
      const bool before = in && (fk < fi || (fk == fi && k < i));
      const bool after = in && (fk > fi || (fk == fi && k > i));
      prev = (before && (!hp || fk > prev)) ? fk : prev;
      next = (after && (!hn || fk < next)) ? fk : next;
      hp = hp || before;
      hn = hn || after;
    }
    if (!hp || !hn) {
      cd = cd + __builtin_inf();
    } else {
      const double range = fmax - fmin;
      const double num = next - prev;
      cd = cd + (range > 0.0 ? num / range : 0.0);
    }
  }
  return cd;
}

// Grid: the samples; sample s ranks F + s Q m into rank, crowd and order + s Q.  MB: the objectives' register bucket
// (2, 4 or 8 >= m).  The scans over the Q points are branch-free and unrolled so that their LDS reads are in flight
// together: one workgroup's scans are bound by LDS latency, not arithmetic.
template <int MB>
__global__ __launch_bounds__(1024) void pareto_rank_kernel(const double* __restrict__ F, int Q, int m, int keep,
                                                           int* __restrict__ rank, double* __restrict__ crowd,
                                                           int* __restrict__ order) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) double pr_smem[];
  const size_t sample = blockIdx.x;
  F += sample * Q * m;
  rank += sample * Q;
  crowd += sample * Q;
  order += sample * Q;
  double* f = pr_smem;                                   // [Q][m]; after the crowding phase [Q] crowding distances
  int* rk = reinterpret_cast<int*>(pr_smem + (size_t)Q * m);  // [Q]: -2 not yet ranked, else the front
  int* list = rk + Q;                                    // [Q]: members of the front being peeled
  int* cnts = list + Q;                                  // [0] members of the front, [1] points ranked so far
  const int tid = threadIdx.x, nt = blockDim.x;
  for (int e = tid; e < Q * m; e += nt) f[e] = F[e];
  for (int e = tid; e < Q; e += nt) {
    rk[e] = -2;
    order[e] = -1;
  }
  if (tid < 2) cnts[tid] = 0;
  __syncthreads();
  // dominator counts of the thread's points
  int cnt[PR_PPT];
  double own[PR_PPT][MB];  // the thread's rows (a slot past Q holds row Q - 1 and is never used)
#pragma unroll
  for (int s = 0; s < PR_PPT; ++s) {
    load_row<MB>(f, min(tid + s * nt, Q - 1), m, own[s]);
    cnt[s] = 0;
  }
#pragma unroll 4
  for (int k = 0; k < Q; ++k) {
    double fk[MB];
    load_row<MB>(f, k, m, fk);
#pragma unroll
    for (int s = 0; s < PR_PPT; ++s) cnt[s] += dominates<MB>(fk, own[s]) ? 1 : 0;
  }
  // peel: front r = the unranked points no unranked point dominates; at most Q fronts
  for (int r = 0; r < Q; ++r) {
#pragma unroll
    for (int s = 0; s < PR_PPT; ++s) {
      const int i = tid + s * nt;
      if (i < Q && rk[i] == -2 && cnt[s] == 0) list[atomicAdd(&cnts[0], 1)] = i;  // any order: only counted over
    }
    __syncthreads();
    const int nf = cnts[0];
    const int done = cnts[1] + nf;
#pragma unroll
    for (int s = 0; s < PR_PPT; ++s) {
      const int i = tid + s * nt;
      if (i < Q && rk[i] == -2) {
        if (cnt[s] == 0) {
          cnt[s] = -1;  // ranked below, after every thread has read this round's rk
        } else {
          int c = 0;
#pragma unroll 4
          for (int q = 0; q < nf; ++q) {
            double fk[MB];
            load_row<MB>(f, list[q], m, fk);
            c += dominates<MB>(fk, own[s]) ? 1 : 0;
          }
          cnt[s] -= c;
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < PR_PPT; ++s) {
      const int i = tid + s * nt;
      if (i < Q && cnt[s] == -1) {
        rk[i] = r;
        cnt[s] = -3;
      }
    }
    if (tid == 0) {
      cnts[0] = 0;
      cnts[1] = done;
    }
    __syncthreads();
    if (done >= keep || nf == 0) break;  // uniform: read from LDS before the barrier above
  }
  // crowding within each ranked front
  double cd[PR_PPT];
#pragma unroll
  for (int s = 0; s < PR_PPT; ++s) {
    const int i = tid + s * nt;
    cd[s] = 0.0;
    if (i >= Q || rk[i] < 0) continue;
    cd[s] = front_crowding(f, rk, Q, m, i, rk[i]);
  }
  __syncthreads();  // every read of f as objectives is done: it now holds the crowding distances
#pragma unroll
  for (int s = 0; s < PR_PPT; ++s) {
    const int i = tid + s * nt;
    if (i < Q) {
      f[i] = cd[s];
      crowd[i] = cd[s];
      rank[i] = rk[i] < 0 ? -1 : rk[i];
    }
  }
  __syncthreads();
  // survivor order: a ranked point's position is the number of ranked points whose key (rank, -crowding, index)
  // is below its own; positions are < Q whatever the values
#pragma unroll
  for (int s = 0; s < PR_PPT; ++s) {
    const int i = tid + s * nt;
    if (i >= Q || rk[i] < 0) continue;
    const int ri = rk[i];
    const double ci = f[i];
    int pos = 0;
#pragma unroll 4
    for (int k = 0; k < Q; ++k) {
      const int rkk = rk[k];
      const double ck = f[k];
      const bool before = rkk >= 0 && (rkk < ri || (rkk == ri && (ck > ci || (ck == ci && k < i))));
      pos += before ? 1 : 0;
    }
    order[pos] = i;
  }
}

// Threads of the one-workgroup rank of Q points
__host__ inline int rank_threads(int Q) { return std::min(1024, std::max(64, (Q + 63) / 64 * 64)); }

// S samples of Q points each, one workgroup per sample
static hipError_t launch_rank(const double* F, int S, int Q, int m, int keep, int* rank, double* crowd, int* order,
                              hipStream_t s) {
  const size_t lds = rank_lds_bytes(Q, m);
  const int nt = rank_threads(Q);
  by_objectives(m, [&](auto mb) {
    launch_lds(pareto_rank_kernel<decltype(mb)::value>, dim3(S), dim3(nt), lds, s, F, Q, m, keep, rank, crowd, order);
  });
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
  Carve c;
  w.cnt = c.take((size_t)Q * sizeof(int));
  w.rk = c.take((size_t)Q * sizeof(int));
  w.scalars = c.take(256);
  w.total = c.total();
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
  int* cnt = at<int>(work, w.cnt);
  int* rk = at<int>(work, w.rk);
  int* scalars = at<int>(work, w.scalars);
  hipError_t e;
  hipLaunchKernelGGL(pareto_clear_kernel, dim3((std::max(Q, 64) + 255) / 256), dim3(256), 0, s, Q, cnt, rk, scalars,
                     order);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  const dim3 dgrid((Q + PD_TILE - 1) / PD_TILE, (Q + PD_SLICE - 1) / PD_SLICE);
  by_objectives(m, [&](auto mb) {
    hipLaunchKernelGGL(pareto_dom_kernel<decltype(mb)::value>, dgrid, dim3(PD_TILE), 0, s, F, Q, m, cnt);
  });
  if ((e = hipGetLastError()) != hipSuccess) return e;
  const bool in_lds = peel_f_in_lds(Q, m);
  const size_t lds = peel_list_bytes(Q) + (in_lds ? (size_t)Q * m * sizeof(double) : 0);
  const int nt = std::min(1024, (Q + 63) / 64 * 64);
  by_objectives(m, [&](auto mb) {
    constexpr int MB = decltype(mb)::value;
    launch_lds(in_lds ? pareto_peel_kernel<MB, true> : pareto_peel_kernel<MB, false>, dim3(1), dim3(nt), lds, s, F, Q,
               m, keep, (const int*)cnt, rk, scalars);
  });
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
                                    : launch_rank(F, 1, Q, m, keep, rank, crowd, order, s);
}

// ---------------------------------------------------------------------------------------------------------------
// Variation.  Draw layout (include/dkg.h): u[2 w], u[2 w + 1] the tournament of winner w; then per pair k < P / 2
// its crossover gate; then per (pair, coordinate) three numbers (cross this coordinate, the spread, swap); then per
// (child, coordinate) two (mutate, the perturbation).
struct VarArgs {
  const double* X;      // [P][d]
  const int* rank;      // [P]
  const double* crowd;  // [P]
  const double *lb, *ub;
  const double* u;
  double* child;  // [P][d]
  int P, d;
  double cr, eta_c, pm, eta_m;
};

__device__ __forceinline__ int tournament(const VarArgs& a, int w) {
  const int P = a.P;
  int i0 = (int)(a.u[2 * w] * P), i1 = (int)(a.u[2 * w + 1] * P);
  i0 = max(0, min(i0, P - 1));
  i1 = max(0, min(i1, P - 1));
  const int r0 = a.rank[i0], r1 = a.rank[i1];
  const bool second = r1 < r0 || (r1 == r0 && a.crowd[i1] > a.crowd[i0]);
  return second ? i1 : i0;
}

__device__ __forceinline__ double sbx_betaq(double u, double beta, double eta) {
#pragma clang fp contract(off)
  const double alpha = 2.0 - pow(beta, -(eta + 1.0));
  const double e = 1.0 / (eta + 1.0);
  return (u <= 1.0 / alpha) ? pow(u * alpha, e) : pow(1.0 / (2.0 - u * alpha), e);
}

__device__ __forceinline__ double poly_mutate(double y, double lo, double hi, double u, double eta) {
#pragma clang fp contract(off)
  const double span = hi - lo;
  if (!(span > 0.0)) return y;
  const double d1 = (y - lo) / span, d2 = (hi - y) / span;
  const double mp = 1.0 / (eta + 1.0);
  double dq;
  if (u < 0.5) {
    const double xy = 1.0 - d1;
    const double val = 2.0 * u + (1.0 - 2.0 * u) * pow(xy, eta + 1.0);
    dq = pow(val, mp) - 1.0;
  } else {
    const double xy = 1.0 - d2;
    const double val = 2.0 * (1.0 - u) + 2.0 * (u - 0.5) * pow(xy, eta + 1.0);
    dq = 1.0 - pow(val, mp);
  }
  return clip(y + dq * span, lo, hi);
}

// Thread t < (P / 2) d: coordinate t % d of the pair of children t / d
__device__ __forceinline__ void pareto_variation_body(const VarArgs& a, int t) {
#pragma clang fp contract(off)
  const int P = a.P, d = a.d, H = P / 2;
  if (t >= H * d) return;
  const int k = t / d, c = t - k * d;
  const int w0 = tournament(a, 2 * k), w1 = tournament(a, 2 * k + 1);
  const double lo = a.lb[c], hi = a.ub[c];
  double c0 = a.X[(size_t)w0 * d + c], c1 = a.X[(size_t)w1 * d + c];
  const double* ug = a.u + 2 * (size_t)P;
  const double* ux = ug + H + 3 * ((size_t)k * d + c);
  if (ug[k] < a.cr && ux[0] < 0.5) {
    const double y1 = c0 < c1 ? c0 : c1, y2 = c0 < c1 ? c1 : c0;
    const double dy = y2 - y1;
    if (dy > 1e-14) {
      const double bq1 = sbx_betaq(ux[1], 1.0 + 2.0 * (y1 - lo) / dy, a.eta_c);
      const double bq2 = sbx_betaq(ux[1], 1.0 + 2.0 * (hi - y2) / dy, a.eta_c);
      const double n1 = clip(0.5 * ((y1 + y2) - bq1 * dy), lo, hi);
      const double n2 = clip(0.5 * ((y1 + y2) + bq2 * dy), lo, hi);
      const bool swap = ux[2] < 0.5;
      c0 = swap ? n2 : n1;
      c1 = swap ? n1 : n2;
    }
  }
  const double* um = ug + H + 3 * (size_t)H * d;
  const double* m0 = um + 2 * ((size_t)(2 * k) * d + c);
  const double* m1 = um + 2 * ((size_t)(2 * k + 1) * d + c);
  if (m0[0] < a.pm) c0 = poly_mutate(c0, lo, hi, m0[1], a.eta_m);
  if (m1[0] < a.pm) c1 = poly_mutate(c1, lo, hi, m1[1], a.eta_m);
  a.child[(size_t)(2 * k) * d + c] = clip(c0, lo, hi);
  a.child[(size_t)(2 * k + 1) * d + c] = clip(c1, lo, hi);
}

// ---------------------------------------------------------------------------------------------------------------
// A generation of S populations; blockIdx.y the sample in the three kernels below.
struct GenArgs {
  const double *lb, *ub;
  const double* u;     // sample s's uniforms at u + s * u_stride
  size_t u_stride;
  size_t u_off;        // this generation's draws within a sample's uniforms
  double *X, *F, *crowd;     // the population: [S][P][d], [S][P][m], [S][P]
  int* rank;                 // [S][P]
  double *X2, *F2, *crowd2;  // [parents; children]: [S][2P][d], [S][2P][m], [S][2P]
  int *rank2, *order;        // [S][2P]
  double* child;             // X2 == NULL (dkg_pareto_variation: no F, nothing to copy): the children [P][d]
  int P, d, m;
  double cr, eta_c, pm, eta_m;
};

// x[s][p][k] = lb[k] + u[s][p][k] (ub[k] - lb[k]), clipped into the bounds
__global__ __launch_bounds__(256) void pareto_init_kernel(GenArgs g) {
#pragma clang fp contract(off)
  const int t = blockIdx.x * blockDim.x + threadIdx.x, s = blockIdx.y;
  const int total = g.P * g.d;
  if (t >= total) return;
  const int k = t % g.d;
  g.X[(size_t)s * total + t] = clip(g.lb[k] + g.u[s * g.u_stride + t] * (g.ub[k] - g.lb[k]), g.lb[k], g.ub[k]);
}

// The parents into the first half of [parents; children], and the children: one thread per (pair of children,
// coordinate) of pareto_variation_body
__global__ __launch_bounds__(256) void pareto_variation_kernel(GenArgs g) {
  const int s = blockIdx.y, P = g.P, d = g.d, m = g.m;
  const int t = blockIdx.x * blockDim.x + threadIdx.x, nt = gridDim.x * blockDim.x;
  const double* X = g.X + (size_t)s * P * d;
  double* child = g.child;
  if (g.X2) {
    const double* F = g.F + (size_t)s * P * m;
    double* X2 = g.X2 + (size_t)s * 2 * P * d;
    double* F2 = g.F2 + (size_t)s * 2 * P * m;
    for (int e = t; e < P * d; e += nt) X2[e] = X[e];
    for (int e = t; e < P * m; e += nt) F2[e] = F[e];
    child = X2 + (size_t)P * d;
  }
  VarArgs a{X, g.rank + (size_t)s * P, g.crowd + (size_t)s * P, g.lb, g.ub, g.u + s * g.u_stride + g.u_off, child,
            P, d, g.cr, g.eta_c, g.pm, g.eta_m};
  pareto_variation_body(a, t);
}

static hipError_t launch_variation(const GenArgs& g, int S, hipStream_t s) {
  const int total = g.P / 2 * g.d;
  hipLaunchKernelGGL(pareto_variation_kernel, dim3((total + 255) / 256, S), dim3(256), 0, s, g);
  return hipGetLastError();
}

// survivor r of sample s = point order[s][r] of its [parents; children]
__global__ __launch_bounds__(256) void pareto_gather_kernel(GenArgs g) {
  const int s = blockIdx.y, P = g.P, d = g.d, m = g.m;
  const int w = d + m + 2;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= P * w) return;
  const int r = t / w, c = t - r * w;
  const int src = g.order[(size_t)s * 2 * P + r];
  if (src < 0 || src >= 2 * P) return;  // never for r < keep; keeps a bad order in bounds
  const size_t s2 = (size_t)s * 2 * P + src, s1 = (size_t)s * P + r;
  if (c < d) g.X[s1 * d + c] = g.X2[s2 * d + c];
  else if (c < d + m) g.F[s1 * m + (c - d)] = g.F2[s2 * m + (c - d)];
  else if (c == d + m) g.rank[s1] = g.rank2[s2];
  else g.crowd[s1] = g.crowd2[s2];
}

// ---------------------------------------------------------------------------------------------------------------
// Pruning.  One workgroup per sample; LDS: F [Q][m], alive [Q] (0 alive, -1 not: front_crowding's front 0).
__host__ __device__ inline size_t prune_lds_bytes(int Q, int m) {
  return (size_t)Q * m * sizeof(double) + (size_t)Q * sizeof(int);
}

__global__ __launch_bounds__(1024) void pareto_prune_kernel(const double* __restrict__ F, const int* __restrict__ rank,
                                                            int Q, int m, int k, int* __restrict__ count,
                                                            int* __restrict__ index) {
  extern __shared__ __attribute__((aligned(16))) double pu_smem[];
  __shared__ double red_cd[16];
  __shared__ int red_ix[16];
  double* f = pu_smem;
  int* alive = reinterpret_cast<int*>(pu_smem + (size_t)Q * m);
  const size_t s = blockIdx.x;
  F += s * Q * m;
  rank += s * Q;
  index += s * k;
  const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
  for (int e = tid; e < Q * m; e += nt) f[e] = F[e];
  for (int e = tid; e < Q; e += nt) alive[e] = rank[e] == 0 ? 0 : -1;
  for (int e = tid; e < k; e += nt) index[e] = -1;
  __syncthreads();
  // of members with bit-equal objective vectors the lowest index stays
  bool dup[PR_PPT];
#pragma unroll
  for (int sl = 0; sl < PR_PPT; ++sl) {
    const int i = tid + sl * nt;
    dup[sl] = false;
    if (i >= Q || alive[i] != 0) continue;
    for (int j = 0; j < i && !dup[sl]; ++j) {
      if (alive[j] != 0) continue;
      bool same = true;
      for (int c = 0; c < m; ++c)
        same = same && __double_as_longlong(f[(size_t)i * m + c]) == __double_as_longlong(f[(size_t)j * m + c]);
      dup[sl] = same;
    }
  }
  __syncthreads();
#pragma unroll
  for (int sl = 0; sl < PR_PPT; ++sl)
    if (dup[sl]) alive[tid + sl * nt] = -1;
  __syncthreads();
  int cnt = 0;
#pragma unroll
  for (int sl = 0; sl < PR_PPT; ++sl) {
    const int i = tid + sl * nt;
    cnt += __syncthreads_count(i < Q && alive[i] == 0);
  }
  while (cnt > k) {  // uniform
    double bcd = __builtin_inf();
    int bix = 0x7fffffff;
#pragma unroll
    for (int sl = 0; sl < PR_PPT; ++sl) {
      const int i = tid + sl * nt;
      if (i >= Q || alive[i] != 0) continue;
      const double cd = front_crowding(f, alive, Q, m, i, 0);
      if (cd < bcd || (cd == bcd && i < bix)) {
        bcd = cd;
        bix = i;
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double ocd = __shfl_xor(bcd, off);
      const int oix = __shfl_xor(bix, off);
      if (ocd < bcd || (ocd == bcd && oix < bix)) {
        bcd = ocd;
        bix = oix;
      }
    }
    if (lane == 0) {
      red_cd[wave] = bcd;
      red_ix[wave] = bix;
    }
    __syncthreads();
    bcd = red_cd[0];
    bix = red_ix[0];
    for (int w2 = 1; w2 < nw; ++w2) {
      const double ocd = red_cd[w2];
      const int oix = red_ix[w2];
      if (ocd < bcd || (ocd == bcd && oix < bix)) {
        bcd = ocd;
        bix = oix;
      }
    }
    __syncthreads();  // every thread has read the wave results and this round's alive set
    if (bix >= Q) break;  // never: cnt > k >= 1 members are alive
    if (tid == 0) alive[bix] = -1;
    __syncthreads();
    --cnt;
  }
  if (tid == 0) count[s] = cnt;
#pragma unroll
  for (int sl = 0; sl < PR_PPT; ++sl) {
    const int i = tid + sl * nt;
    if (i >= Q || alive[i] != 0) continue;
    int pos = 0;
    for (int j = 0; j < i; ++j) pos += alive[j] == 0 ? 1 : 0;
    if (pos < k) index[pos] = i;
  }
}

}  // namespace dkg

using namespace dkg;

namespace {

int check_model(const dkg_output* outs, int m, int d) {
  if (!outs) return failf(DKG_ERR_ARG, "NULL pointer");
  int st = check_dims(m, d);
  for (int i = 0; i < m && !st; ++i) {
    char who[32];
    std::snprintf(who, sizeof who, "output %d", i);
    st = check_output_state(outs[i], false, who);
  }
  return st;
}

int check_population(int P) {
  if (P < 8 || P % 4) return failf(DKG_ERR_ARG, "population P=%d (a multiple of 4, at least 8)", P);
  if (P > 1024) return failf(DKG_ERR_UNSUPPORTED, "population P=%d (supported <= 1024)", P);
  return DKG_OK;
}

int check_params(const dkg_nsga2_params* p) {
  if (!p) return failf(DKG_ERR_ARG, "NULL pointer");
  if (!(p->cr >= 0.0 && p->cr <= 1.0) || !(p->m >= 0.0 && p->m <= 1.0) || !(p->eta_c >= 0.0) || !(p->eta_m >= 0.0))
    return failf(DKG_ERR_ARG, "nsga2 parameters cr=%g eta_c=%g m=%g eta_m=%g", p->cr, p->eta_c, p->m, p->eta_m);
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

// What the variation reads besides the population
GenArgs gen_args(const double* lb, const double* ub, const double* u, int P, int d, int m,
                 const dkg_nsga2_params* prm) {
  GenArgs g{};
  g.lb = lb;
  g.ub = ub;
  g.u = u;
  g.P = P;
  g.d = d;
  g.m = m;
  g.cr = prm->cr;
  g.eta_c = prm->eta_c;
  g.pm = prm->m;
  g.eta_m = prm->eta_m;
  return g;
}

// The fitness of an evolution: the values of P points of every sample, sample s's points [P][d] at x + s * x_stride,
// into F + s * f_stride [P][m]; lb / ub not NULL: the model input is unit_cube(x, lb, ub).
struct Evaluator {
  hipError_t (*launch)(const void* ctx, const double* x, size_t x_stride, double* F, size_t f_stride,
                       const double* lb, const double* ub, int P, hipStream_t s);
  const void* ctx;
  const char* what;  // the kernel, for dkg_last_error
};

// ctx: a MeanArgs holding the model.  One population: the strides are not read.
hipError_t eval_mean(const void* ctx, const double* x, size_t, double* F, size_t, const double* lb, const double* ub,
                     int P, hipStream_t s) {
  MeanArgs a = *static_cast<const MeanArgs*>(ctx);
  a.x = x;
  a.lb = lb;
  a.ub = ub;
  a.P = P;
  a.mean = F;
  return launch_mean(a, s);
}

// ctx: the dkg_rff_paths
hipError_t eval_paths(const void* ctx, const double* x, size_t x_stride, double* F, size_t f_stride, const double* lb,
                      const double* ub, int P, hipStream_t s) {
  return launch_rff_eval(*static_cast<const dkg_rff_paths*>(ctx), x, x_stride, F, f_stride, lb, ub, P, s);
}

// The evolution's workspace carve: [parents; children] of S populations and their ranking, then (wide) the wide
// rank's scratch for the 2P points of a generation
struct GenWs {
  size_t x2, f2, crowd2, rank2, order, wide, total;
};
GenWs gen_ws(int S, int P, int d, int m, bool wide) {
  GenWs w{};
  Carve c;
  const size_t q = (size_t)S * 2 * P;
  w.x2 = c.take(q * d * sizeof(double));
  w.f2 = c.take(q * m * sizeof(double));
  w.crowd2 = c.take(q * sizeof(double));
  w.rank2 = c.take(q * sizeof(int));
  w.order = c.take(q * sizeof(int));
  w.wide = c.take(wide ? wide_ws(2 * P).total : 0);
  w.total = c.total();
  return w;
}

// NSGA-II of S populations of P points in d dimensions with m objectives (the caller has checked S, d and m with its
// model): the initial sample, its values and ranks, then `gens` times the variation, the children's values, the rank
// of [parents; children] with keep = P, and the survivors.  wide: the workspace carries the wide rank's scratch, and
// one population is ranked by launch_rank_any's rule; otherwise one workgroup ranks each sample.
int evolve(const Evaluator& ev, int S, int d, int m, bool wide, const double* lb, const double* ub, int P, int gens,
           const dkg_nsga2_params* prm, const double* uniforms, double* X, double* F, int* rank, double* crowd,
           void* work, size_t work_bytes, hipStream_t s) {
  int st = check_population(P);
  if (st) return st;
  if (gens < 0 || gens > (1 << 20)) return failf(DKG_ERR_ARG, "gens=%d generations", gens);
  if ((st = check_params(prm))) return st;
  if (!lb || !ub || !uniforms || !X || !F || !rank || !crowd || !work) return failf(DKG_ERR_ARG, "NULL pointer");
  const GenWs w = gen_ws(S, P, d, m, wide);
  if (work_bytes < w.total) return failf(DKG_ERR_WORKSPACE, "workspace %zu bytes < required %zu", work_bytes, w.total);
  const size_t Pd = (size_t)P * d, Pm = (size_t)P * m, draws = dkg_pareto_draws(P, d);
  GenArgs g = gen_args(lb, ub, uniforms, P, d, m, prm);
  g.u_stride = Pd + (size_t)gens * draws;
  g.X = X;
  g.F = F;
  g.crowd = crowd;
  g.rank = rank;
  g.X2 = at<double>(work, w.x2);
  g.F2 = at<double>(work, w.f2);
  g.crowd2 = at<double>(work, w.crowd2);
  g.rank2 = at<int>(work, w.rank2);
  g.order = at<int>(work, w.order);
  void* wide_work = wide && S == 1 ? at<char>(work, w.wide) : nullptr;
  const double *elb = prm->raw_inputs ? nullptr : lb, *eub = prm->raw_inputs ? nullptr : ub;
  // the Q = P or 2P points per sample of f, keep = P
  auto rank_step = [&](const double* f, int Q, int* rk, double* cd) {
    return hip_status(wide_work ? launch_rank_any(f, Q, m, P, rk, cd, g.order, wide_work, s)
                                : launch_rank(f, S, Q, m, P, rk, cd, g.order, s),
                      "pareto_rank_kernel");
  };
  const dim3 b256(256);
  hipLaunchKernelGGL(pareto_init_kernel, dim3((P * d + 255) / 256, S), b256, 0, s, g);
  if ((st = hip_status(hipGetLastError(), "pareto_init_kernel")) ||
      (st = hip_status(ev.launch(ev.ctx, X, Pd, F, Pm, elb, eub, P, s), ev.what)) ||
      (st = rank_step(F, P, rank, crowd)))
    return st;
  const int gt = P * (d + m + 2);
  for (int gen = 0; gen < gens; ++gen) {
    g.u_off = Pd + (size_t)gen * draws;
    if ((st = hip_status(launch_variation(g, S, s), "pareto_variation_kernel")) ||
        (st = hip_status(ev.launch(ev.ctx, g.X2 + Pd, 2 * Pd, g.F2 + Pm, 2 * Pm, elb, eub, P, s), ev.what)) ||
        (st = rank_step(g.F2, 2 * P, g.rank2, g.crowd2)))
      return st;
    hipLaunchKernelGGL(pareto_gather_kernel, dim3((gt + 255) / 256, S), b256, 0, s, g);
    if ((st = hip_status(hipGetLastError(), "pareto_gather_kernel"))) return st;
  }
  return DKG_OK;
}

}  // namespace

extern "C" {

int dkg_posterior_mean(const dkg_output* outs, int m, int d, const double* x, int P, double* mean, void* stream) {
  int st = check_model(outs, m, d);
  if (st) return st;
  if (P < 0 || P > (1 << 24)) return failf(DKG_ERR_ARG, "P=%d points", P);
  if (P == 0) return DKG_OK;
  if (!x || !mean) return failf(DKG_ERR_ARG, "NULL pointer");
  return hip_status(launch_mean(mean_args(outs, m, d, x, P, mean), (hipStream_t)stream), "posterior_mean_kernel");
}

size_t dkg_pareto_rank_workspace(int Q, int m) {
  if (Q < 1 || Q > WR_MAXQ || m < 1 || m > DKG_MAX_OUTPUTS) return 0;
  return wide_ws(Q).total;
}

int dkg_pareto_rank(const double* F, int Q, int m, int keep, int* rank, double* crowd, int* order, void* work,
                    size_t work_bytes, void* stream) {
  if (Q < 1 || m < 1 || keep < 1 || keep > Q) return failf(DKG_ERR_ARG, "Q=%d m=%d keep=%d", Q, m, keep);
  if (Q > (work ? WR_MAXQ : PR_MAXQ))
    return failf(DKG_ERR_UNSUPPORTED, "Q=%d points (supported <= %d, <= %d with a workspace)", Q, PR_MAXQ, WR_MAXQ);
  if (m > DKG_MAX_OUTPUTS) return failf(DKG_ERR_UNSUPPORTED, "m=%d objectives (supported <= %d)", m, DKG_MAX_OUTPUTS);
  if (!F || !rank || !crowd || !order) return failf(DKG_ERR_ARG, "NULL pointer");
  if (work && work_bytes < wide_ws(Q).total)
    return failf(DKG_ERR_WORKSPACE, "workspace %zu bytes < required %zu", work_bytes, wide_ws(Q).total);
  return hip_status(launch_rank_any(F, Q, m, keep, rank, crowd, order, work, (hipStream_t)stream), "dkg_pareto_rank");
}

int dkg_debug_pareto_wide(int mode) {
  if (mode < -1 || mode > 1) {
    failf(DKG_ERR_ARG, "dkg_debug_pareto_wide: mode=%d (-1 the rule, 0 never below %d points, 1 always)", mode,
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
  if (d < 1) return failf(DKG_ERR_ARG, "d=%d", d);
  if (d > DKG_MAX_DIM) return failf(DKG_ERR_UNSUPPORTED, "d=%d (supported 1..%d)", d, DKG_MAX_DIM);
  if ((st = check_params(prm))) return st;
  if (!X || !rank || !crowd || !lb || !ub || !uniforms || !children) return failf(DKG_ERR_ARG, "NULL pointer");
  // one population, its uniforms as given, no [parents; children]; the kernel only reads X, rank and crowd
  GenArgs g = gen_args(lb, ub, uniforms, P, d, 0, prm);
  g.X = const_cast<double*>(X);
  g.rank = const_cast<int*>(rank);
  g.crowd = const_cast<double*>(crowd);
  g.child = children;
  return hip_status(launch_variation(g, 1, (hipStream_t)stream), "pareto_variation_kernel");
}

size_t dkg_pareto_workspace(int P, int d, int m) {
  if (P < 8 || P % 4 || P > 1024 || d < 1 || d > DKG_MAX_DIM || m < 1 || m > DKG_MAX_OUTPUTS) return 0;
  return gen_ws(1, P, d, m, true).total;
}

int dkg_pareto_nsga2(const dkg_output* outs, int m, int d, const double* lb, const double* ub, int P, int gens,
                     const dkg_nsga2_params* prm, const double* uniforms, double* X, double* F, int* rank,
                     double* crowd, void* work, size_t work_bytes, void* stream) {
  int st = check_model(outs, m, d);
  if (st) return st;
  const MeanArgs model = mean_args(outs, m, d, nullptr, 0, nullptr);
  return evolve({eval_mean, &model, "posterior_mean_kernel"}, 1, d, m, true, lb, ub, P, gens, prm, uniforms, X, F,
                rank, crowd, work, work_bytes, (hipStream_t)stream);
}

size_t dkg_pareto_paths_workspace(int S, int P, int d, int m) {
  if (S < 1 || S > DKG_JES_MAX_SAMPLES || P < 8 || P % 4 || P > 1024 || d < 1 || d > DKG_MAX_DIM || m < 1 ||
      m > DKG_MAX_OUTPUTS)
    return 0;
  return gen_ws(S, P, d, m, false).total;
}

int dkg_pareto_nsga2_paths(const dkg_rff_paths* paths, const double* lb, const double* ub, int P, int gens,
                           const dkg_nsga2_params* prm, const double* uniforms, double* X, double* F, int* rank,
                           double* crowd, void* work, size_t work_bytes, void* stream) {
  int st = check_rff_paths(paths);
  if (st) return st;
  return evolve({eval_paths, paths, "rff_eval_kernel"}, paths->S, paths->d, paths->m, false, lb, ub, P, gens, prm,
                uniforms, X, F, rank, crowd, work, work_bytes, (hipStream_t)stream);
}

int dkg_pareto_prune(const double* F, const int* rank, int S, int Q, int m, int k, int* count, int* index,
                     void* stream) {
  if (S < 1 || Q < 1 || m < 1 || k < 1) return failf(DKG_ERR_ARG, "S=%d Q=%d m=%d k=%d", S, Q, m, k);
  if (S > DKG_JES_MAX_SAMPLES) return failf(DKG_ERR_UNSUPPORTED, "S=%d samples (supported <= %d)", S, DKG_JES_MAX_SAMPLES);
  if (Q > PR_MAXQ || k > PR_MAXQ) return failf(DKG_ERR_UNSUPPORTED, "Q=%d k=%d (supported <= %d)", Q, k, PR_MAXQ);
  if (m > DKG_MAX_OUTPUTS) return failf(DKG_ERR_UNSUPPORTED, "m=%d objectives (supported <= %d)", m, DKG_MAX_OUTPUTS);
  if (!F || !rank || !count || !index) return failf(DKG_ERR_ARG, "NULL pointer");
  const size_t lds = prune_lds_bytes(Q, m);
  raise_lds_limit(reinterpret_cast<const void*>(pareto_prune_kernel), lds);
  hipLaunchKernelGGL(pareto_prune_kernel, dim3(S), dim3(rank_threads(Q)), lds, (hipStream_t)stream, F, rank, Q, m, k,
                     count, index);
  return hip_status(hipGetLastError(), "pareto_prune_kernel");
}

}  // extern "C"
