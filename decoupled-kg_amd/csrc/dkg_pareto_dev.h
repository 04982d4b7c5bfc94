// Device bodies of the NSGA-II stages that more than one translation unit launches: the one-workgroup rank
// (dkg_pareto.hip: one population; dkg_rff.hip: one workgroup per sample, and the pruning's crowding) and the
// variation (the same two).  A kernel that calls a body gives the bits every other kernel calling it gives.
#pragma once

#include <algorithm>

#include "dkg_stages.h"

namespace dkg {

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

// MB: the objectives' register bucket (2, 4 or 8 >= m).  The scans over the Q points are branch-free and unrolled
// so that their LDS reads are in flight together: one workgroup's scans are bound by LDS latency, not arithmetic.
// pr_smem: rank_lds_bytes(Q, m) bytes of LDS, 16-byte aligned.
template <int MB>
__device__ __forceinline__ void pareto_rank_body(const double* __restrict__ F, int Q, int m, int keep,
                                                 int* __restrict__ rank, double* __restrict__ crowd,
                                                 int* __restrict__ order, double* pr_smem) {
#pragma clang fp contract(off)
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

__device__ __forceinline__ double clip(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

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

}  // namespace dkg
