// Hypervolume knowledge gradient (Daulton et al., ICML 2023) on the device (gfx950), q = 1, one-shot, with
// BoTorch's X_evaluation_mask for the decoupled setting, and its value function (the hypervolume of the
// posterior mean at q points).  The reference drives BoTorch's qHypervolumeKnowledgeGradient through
// HvkgOptimisationSpec (modules/acquisition_optimisation_strategy.py:276-444).  A one-shot point is
// X_full [1 + Nf Np][d]: row 0 the candidate x, row 1 + f Np + p point p of fantasy f.  Per output i
//   Y_fp,i = y_mean_i + y_std_i (mu_i(x'_fp) + [i in E] z_f,i c_i(x'_fp, x) / sigma~_i(x)),
//   acq    = ((1 / Nf) sum_f HV_f - current_value) / cost,   HV_f the volume of the union of the boxes [ref, Y_fp]:
// the fantasy mean is the exact posterior mean after observing mu_i(x) + sigma~_i(x) z_f,i at x.  An evaluation is
// four launches (three in value-function mode) whatever B, Nf, Np and m are:
//
//   hvkg_cand_kernel     grid (restart, output in E): k = s kappa(X, x), q = L^-1 k out of R^T's fragments,
//                        sigma~ = sqrt(s - |q|^2 + noise), w = L^-T q = K^-1 k.
//   hvkg_fantasy_kernel  grid (16 fantasy points, output, restart), one wave per point, lanes over the training
//                        rows: mu(x') and k(x', X) w in one pass, then Y; with the gradient dY/dx' and
//                        s dkappa(x', x)/dx'.
//   hvkg_hv_kernel       one wave per (restart, fantasy): HV_f and dHV_f/dY (m = 2 a sort and one sweep; m = 3
//                        slabs on the last objective over 2-d sweeps, lane k the slab k).  dkg_hypervolume launches
//                        it alone.
//   hvkg_finish_kernel   one workgroup per restart: acq; with the gradient dacq/dx' and, per output in E, the
//                        vectors t = sum_fp a_fp k(X, x'_fp), u = K^-1 t and the candidate's gradient
//                        (1 / sigma~) sum_fp a_fp s dkappa(x'_fp, x)/dx + sum_j dk_j/dx (C w_j / sigma~^3 - u_j / sigma~).
//
// No atomics; every sum runs in a fixed order that depends on the restart's own data only, so two calls give the
// same bits and a restart's results do not depend on B or on its row.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "dkg_acq.h"
#include "dkg_stages.h"

namespace dkg {

constexpr int HK_WAVES = 4;      // waves per workgroup of the candidate, fantasy and finish kernels
constexpr int HK_POINTS = 16;    // fantasy points per workgroup of the fantasy stage (4 per wave, in turn)
constexpr int HK_MAXM = 3;       // objectives the hypervolume stage handles
constexpr int HK_WSTRIDE = 1024; // doubles between the w vectors of the workspace: the limit n_pad
constexpr unsigned HVKG_MAGIC = 0x48564b47u;

struct HvkgPlan {
  unsigned magic;
  int m, d, Nf, Np, R, rows, mask, max_B, np_max;  // np_max: the largest n_pad of the outputs
  double ref[HK_MAXM];
  double current, cost;
  const dkg_output* tab;  // device [m]
  const double* z;        // device [Nf][m]
  double* w;              // device [max_B][m][HK_WSTRIDE]: K^-1 k(X, x)
  double* sig;            // device [max_B][m]: sigma~(x)
  double* Y;              // device [max_B][R][m]
  double* cxx;            // device [max_B][R][m]: c(x', x)
  double* dY;             // device [max_B][R][m][d]: dY/dx'
  double* dkx;            // device [max_B][R][m][d]: s dkappa(x', x)/dx'
  double* hv;             // device [max_B][Nf]
  double* dhv;            // device [max_B][R][m]
};

struct HvkgHost {
  HvkgPlan plan;
  dkg_output tab[HK_MAXM];
  double z[DKG_HVKG_MAX_FANTASIES * HK_MAXM];
};

// The sum of one value per thread over the workgroup, returned to every thread: wave_sum, then the waves in index
// order.  red: LDS [HK_WAVES].  Two barriers; every thread of the workgroup calls it.
__device__ __forceinline__ double block_sum(double v, double* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double s = wave_sum(v);
  __syncthreads();  // the previous call's reads of red are done
  if (lane == 0) red[wave] = s;
  __syncthreads();
  double t = 0.0;
#pragma unroll
  for (int w = 0; w < HK_WAVES; ++w) t += red[w];
  return t;
}

// q = P v for the lower-triangular P = L^-1 held as R^T's fragments (P[c][r] = R[r][c]): wave `wave` owns the row
// tiles wave, wave + HK_WAVES, ...; lane l the row 16 t + (l & 15) over the columns 4 kb + (l >> 4) of the tile's
// k-blocks in order, the four lanes of a row by cross-lane adds.  v, q: LDS [np]; the caller puts barriers around it.
__device__ __forceinline__ void tri_matvec(const double* __restrict__ root, int np, const double* v, double* q) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int T = np / 16, KB = np / 4;
  for (int t = wave; t < T; t += HK_WAVES) {
    double acc = 0.0;
    const int nj = 2 * (t + 1);
    for (int j = 0; j < nj; ++j) {
      const double2 rt = frag_pair(root, t, j, lane, KB);
      const int c0 = 8 * j + (lane >> 4);
      acc = fma(rt.x, v[c0], acc);
      acc = fma(rt.y, v[c0 + 4], acc);
    }
    acc += partner_f64<4>(acc);
    acc += partner_f64<5>(acc);
    if (lane < 16) q[16 * t + lane] = acc;
  }
}

// w = P^T q: wave `wave` owns the 16-byte words j = wave, wave + HK_WAVES, ... (the columns 8 j .. 8 j + 7), lane l
// the rows 16 t + (l & 15) of the tiles t >= j / 2 in order, the 16 lanes of a column by the in-row butterfly.
// q: LDS [np]; w [np] (LDS or global).
__device__ __forceinline__ void tri_matvec_t(const double* __restrict__ root, int np, const double* q, double* w) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int T = np / 16, KB = np / 4;
  for (int j = wave; j < KB / 2; j += HK_WAVES) {
    double a0 = 0.0, a1 = 0.0;
    for (int t = j / 2; t < T; ++t) {
      const double2 rt = frag_pair(root, t, j, lane, KB);
      const double qc = q[16 * t + (lane & 15)];
      a0 = fma(rt.x, qc, a0);
      a1 = fma(rt.y, qc, a1);
    }
    DKG_BUTTERFLY_ROW({ a0 = a0 + partner_f64<S_>(a0); })
    DKG_BUTTERFLY_ROW({ a1 = a1 + partner_f64<S_>(a1); })
    if ((lane & 15) == 0) {
      w[8 * j + (lane >> 4)] = a0;
      w[8 * j + 4 + (lane >> 4)] = a1;
    }
  }
}

struct HvkgCandArgs {
  const dkg_output* tab;
  const double* x;  // [B][rows][d]; row 0 the candidate
  double *w, *sig;
  int m, d, rows, mask;
};

template <int DM>
__global__ __launch_bounds__(HK_WAVES* WAVE) void hvkg_cand_kernel(HvkgCandArgs a) {
  extern __shared__ __attribute__((aligned(16))) double hc_smem[];
  const int b = blockIdx.x, i = blockIdx.y;
  if (!((a.mask >> i) & 1)) return;  // the whole workgroup
  const dkg_output& o = a.tab[i];
  const int n = o.n, d = a.d, np = pad16(n);
  double* kv = hc_smem;     // [np]
  double* q = kv + np;      // [np]
  double* red = q + np;     // [HK_WAVES]
  const int tid = threadIdx.x;
  const double* __restrict__ tx = o.train_x;
  double xr[DM], il[DM];
#pragma unroll
  for (int k = 0; k < DM; ++k) {
    const int kk = min(k, d - 1);
    il[k] = o.inv_lengthscale[kk];
    xr[k] = a.x[(size_t)b * a.rows * d + kk] * il[k];
  }
  const double os = o.outputscale;
  with_kind(o.kernel, [&](auto kind_c) {
    constexpr int KIND = decltype(kind_c)::value;
    const const_dptr tab = psi_tab();
    for (int j = tid; j < np; j += HK_WAVES * WAVE) {
      const int jc = min(j, n - 1);
      double xs[DM];
      scaled_point<DM>(xs, tx + (size_t)jc * d, il, d);
      const double v = cross_kernel_term<DM, KIND>(xr, xs, d, os, tab);
      kv[j] = (j < n) ? v : 0.0;
    }
  });
  __syncthreads();
  tri_matvec(o.root_frag, np, kv, q);
  __syncthreads();
  double part = 0.0;
  for (int j = tid; j < np; j += HK_WAVES * WAVE) part = fma(q[j], q[j], part);
  const double q2 = block_sum(part, red);
  if (tid == 0) a.sig[(size_t)b * a.m + i] = sqrt(os - q2 + o.noise);
  tri_matvec_t(o.root_frag, np, q, a.w + ((size_t)b * a.m + i) * HK_WSTRIDE);
}

struct HvkgFanArgs {
  const dkg_output* tab;
  const double* x;  // [B][rows][d]
  const double* z;  // [Nf][m]
  const double *w, *sig;
  double *Y, *cxx, *dY, *dkx, *y_out;
  int m, d, R, Np, rows, mask, grad;
};

__host__ __device__ inline size_t hvkg_fan_lds_bytes(int n, int d) { return (size_t)n * (d + 2) * sizeof(double); }

template <int DM>
__global__ __launch_bounds__(HK_WAVES* WAVE) void hvkg_fantasy_kernel(HvkgFanArgs a) {
  extern __shared__ __attribute__((aligned(16))) double hf_smem[];
  const int i = blockIdx.y, b = blockIdx.z;
  const dkg_output& o = a.tab[i];
  const int n = o.n, d = a.d;
  const bool obs = (a.mask >> i) & 1;  // output i is observed at the candidate
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  double* xs = hf_smem;                 // [n][d] training inputs / lengthscale
  double* als = xs + (size_t)n * d;     // [n]
  double* ws = als + n;                 // [n]
  const double* __restrict__ wsrc = a.w + ((size_t)b * a.m + i) * HK_WSTRIDE;
  for (int e = tid; e < n * d; e += HK_WAVES * WAVE) xs[e] = o.train_x[e] * o.inv_lengthscale[e % d];
  for (int e = tid; e < n; e += HK_WAVES * WAVE) {
    als[e] = o.alpha[e];
    ws[e] = obs ? wsrc[e] : 0.0;
  }
  __syncthreads();
  const double os = o.outputscale;
  const double sig = obs ? a.sig[(size_t)b * a.m + i] : 1.0;
  const int iters = (n + WAVE - 1) / WAVE;  // wave-uniform trip count
  const int off = a.rows - a.R;             // 1 with a candidate row, 0 in value-function mode
  const double* __restrict__ xb = a.x + (size_t)b * a.rows * d;
  double il[DM];
  clamped_row<DM>(il, o.inv_lengthscale, d);
  for (int pq = wave; pq < HK_POINTS; pq += HK_WAVES) {
    const int r = blockIdx.x * HK_POINTS + pq;
    if (r >= a.R) break;  // wave-uniform
    const double coef = obs ? a.z[(size_t)(r / a.Np) * a.m + i] / sig : 0.0;
    double xr[DM];
    scaled_point<DM>(xr, xb + (size_t)(off + r) * d, il, d);
    double macc = 0.0, cacc = 0.0, ga[DM];
#pragma unroll
    for (int k = 0; k < DM; ++k) ga[k] = 0.0;
    double kxx = 0.0, hxx = 0.0;  // s kappa(x', x) and s kappa'(r) / r there
    with_kind(o.kernel, [&](auto kind_c) {
      constexpr int KIND = decltype(kind_c)::value;
      const const_dptr tab = psi_tab();
      for (int it = 0; it < iters; ++it) {
        const int j = lane + it * WAVE;
        const int jc = min(j, n - 1);
        const double* xj = xs + (size_t)jc * d;
        const double kvr = cross_kernel_term<DM, KIND>(xr, xj, d, os, tab);
        const double kv = (j < n) ? kvr : 0.0;
        macc = fma(kv, als[jc], macc);
        cacc = fma(kv, ws[jc], cacc);
        if (a.grad) {
          double xjr[DM];
          clamped_row<DM>(xjr, xj, d);
          const double aj = obs ? fma(-coef, ws[jc], als[jc]) : als[jc];
          const double h = (j < n) ? os * kernel_dprofile_t<KIND>(sq_dist<DM>(xr, xjr, d)) * aj : 0.0;
#pragma unroll
          for (int k = 0; k < DM; ++k) ga[k] = fma(h, (xr[k] - xjr[k]) * il[k], ga[k]);
        }
      }
      if (obs) {
        double xc[DM];
        scaled_point<DM>(xc, xb, il, d);
        kxx = cross_kernel_term<DM, KIND>(xr, xc, d, os, tab);
        hxx = os * kernel_dprofile_t<KIND>(sq_dist<DM>(xr, xc, d));
      }
    });
    const double mu = o.mean_constant + wave_sum(macc);
    const double cx = obs ? kxx - wave_sum(cacc) : 0.0;
    const double yv = fma(o.y_std, obs ? mu + coef * cx : mu, o.y_mean);
    const size_t at = ((size_t)b * a.R + r) * a.m + i;
    if (lane == 0) {
      a.Y[at] = yv;
      a.cxx[at] = cx;
      if (a.y_out) a.y_out[at] = yv;
    }
    if (a.grad) {
#pragma unroll
      for (int k = 0; k < DM; ++k) {
        if (k < d) {  // uniform
          const double gs = wave_sum(ga[k]);
          const double dk = obs ? hxx * (xr[k] - xb[k] * il[k]) * il[k] : 0.0;
          if (lane == 0) {
            a.dY[at * d + k] = o.y_std * (obs ? gs + coef * dk : gs);
            a.dkx[at * d + k] = dk;
          }
        }
      }
    }
  }
}

struct HvkgHvArgs {
  const double* Y;  // [S][Np][m]
  double *hv, *dhv; // [S], [S][Np][m] (nullable)
  double ref[HK_MAXM];
  int Np, m;
};

// One wave per set of Np <= 32 points.  A point counts when it is strictly above ref in every objective.  m = 3:
// the points in the order (y2 descending, index ascending) have ranks 0 .. K - 1; slab k holds the ranks <= k and
// has the thickness y2_(k) - y2_(k+1) (the last one y2_(K-1) - ref2); HV = sum_k thickness_k A_k with A_k the area
// the slab's points dominate over (ref0, ref1).  m = 2: the one slab of all K points, thickness 1.  Lane k sweeps
// slab k over the points in the order (y0 descending, y1 descending, rank ascending): a point adds
// (y0 - ref0) (y1 - h) when y1 exceeds h, the largest y1 so far, strictly.  Every term is positive.  Gradients:
// dA_k/dy0 = y1 - h and dA_k/dy1 = y0 - (y0 of the next point that adds, or ref0) for the points that add, 0 for
// the others; dHV/dy2 of rank k = A_k - A_(k-1), which is exactly 0 for a point that adds nothing to its slab (the
// two sweeps then run the same operations).
__global__ __launch_bounds__(WAVE) void hvkg_hv_kernel(HvkgHvArgs a) {
  constexpr int MP = DKG_HVKG_MAX_PARETO;
  __shared__ double y[HK_MAXM][MP];
  __shared__ int rk[MP];        // the rank of point p (MP: the point does not count)
  __shared__ int ord[MP];       // the sweep order: ord[t] the point swept t-th
  __shared__ double area[MP];   // A_k
  __shared__ double G[2][MP][MP + 1];  // G[c][k][p]: dA_k / dy_c of point p
  const int s = blockIdx.x, lane = threadIdx.x;
  const int Np = a.Np, m = a.m;
  const bool grad = a.dhv != nullptr;
  const bool live = lane < Np;
  double y0 = 0.0, y1 = 0.0, y2 = 0.0;
  if (live) {
    const double* yp = a.Y + ((size_t)s * Np + lane) * m;
    y0 = yp[0];
    y1 = yp[1];
    y2 = (m == 3) ? yp[2] : 0.0;
  }
  const bool valid = live && y0 > a.ref[0] && y1 > a.ref[1] && (m < 3 || y2 > a.ref[2]);
  if (lane < MP) {
    y[0][lane] = y0;
    y[1][lane] = y1;
    y[2][lane] = y2;
    rk[lane] = valid ? 0 : MP;
  }
  __syncthreads();
  const int K = __popcll(ballot(valid));
  // the rank: the valid points ahead in (y2 descending, index ascending); for m = 2 every y2 is 0: the index order
  int rank = MP;
  if (valid) {
    rank = 0;
    for (int q = 0; q < Np; ++q) {
      const bool ahead = y[2][q] > y2 || (y[2][q] == y2 && q < lane);
      rank += (rk[q] != MP && ahead) ? 1 : 0;
    }
  }
  __syncthreads();
  if (lane < MP) rk[lane] = rank;
  __syncthreads();
  // the sweep position: the valid points ahead in (y0 descending, y1 descending, rank ascending)
  if (valid) {
    int pos = 0;
    for (int q = 0; q < Np; ++q) {
      const double q0 = y[0][q], q1 = y[1][q];
      const bool ahead = q0 > y0 || (q0 == y0 && (q1 > y1 || (q1 == y1 && rk[q] < rank)));
      pos += (rk[q] != MP && ahead) ? 1 : 0;
    }
    ord[pos] = lane;
  }
  if (grad && lane < MP)
    for (int p = 0; p < MP; ++p) G[0][lane][p] = G[1][lane][p] = 0.0;
  __syncthreads();
  // lane k: slab k
  const int k = lane;
  const bool slab = (m == 3) ? k < K : (K > 0 && k == K - 1);
  double A = 0.0, thick = 0.0;
  if (slab) {
    double h = a.ref[1];
    int prev = -1;
    for (int t = 0; t < K; ++t) {
      const int p = ord[t];
      const double p0 = y[0][p], p1 = y[1][p];
      if (rk[p] <= k && p1 > h) {
        A = fma(p0 - a.ref[0], p1 - h, A);
        if (grad) {
          G[0][k][p] = p1 - h;
          if (prev >= 0) G[1][k][prev] = y[0][prev] - p0;
        }
        prev = p;
        h = p1;
      }
    }
    if (grad && prev >= 0) G[1][k][prev] = y[0][prev] - a.ref[0];
    thick = 1.0;
  }
  if (lane < MP) area[lane] = A;
  __syncthreads();
  if (m == 3 && slab) {
    // y2 of the ranks k and k + 1: the points whose rank is k / k + 1
    double zk = 0.0, zn = a.ref[2];
    for (int q = 0; q < Np; ++q) {
      zk = (rk[q] == k) ? y[2][q] : zk;
      zn = (rk[q] == k + 1) ? y[2][q] : zn;
    }
    thick = zk - zn;
  }
  const double hv = wave_sum(thick * A);
  if (lane == 0) a.hv[s] = hv;
  if (grad) {
    // the slabs' thicknesses to LDS (over y[2] of the invalid lanes' slots is not possible: a row of its own)
    __syncthreads();
    if (lane < MP) G[0][lane][MP] = thick;
    __syncthreads();
    if (live) {
      double g0 = 0.0, g1 = 0.0, g2 = 0.0;
      if (valid) {
        for (int kk = 0; kk < MP; ++kk) {
          const double th = G[0][kk][MP];
          g0 = fma(th, G[0][kk][lane], g0);
          g1 = fma(th, G[1][kk][lane], g1);
        }
        if (m == 3) g2 = area[rank] - (rank > 0 ? area[rank - 1] : 0.0);
      }
      double* gp = a.dhv + ((size_t)s * Np + lane) * m;
      gp[0] = g0;
      gp[1] = g1;
      if (m == 3) gp[2] = g2;
    }
  }
}

struct HvkgFinArgs {
  const dkg_output* tab;
  const double* x;  // [B][rows][d]
  const double* z;
  const double *w, *sig, *cxx, *dY, *dkx, *hv, *dhv;
  double *acq, *dacq;  // [B], [B][rows][d] (nullable)
  double current, cost;
  int m, d, Nf, Np, R, rows, mask, np_max;
};

__host__ __device__ inline size_t hvkg_fin_lds_bytes(int R, int np_max) {
  return ((size_t)R + 3 * (size_t)np_max + HK_WAVES) * sizeof(double);
}

template <int DM>
__global__ __launch_bounds__(HK_WAVES* WAVE) void hvkg_finish_kernel(HvkgFinArgs a) {
  extern __shared__ __attribute__((aligned(16))) double hx_smem[];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int m = a.m, d = a.d, R = a.R;
  if (tid == 0) {
    double s = 0.0;
    for (int f = 0; f < a.Nf; ++f) s += a.hv[(size_t)b * a.Nf + f];
    a.acq[b] = (s / (double)a.Nf - a.current) / a.cost;
  }
  if (a.dacq == nullptr) return;
  const double gscale = (1.0 / (double)a.Nf) / a.cost;
  const int off = a.rows - R;
  const double* __restrict__ dhv = a.dhv + (size_t)b * R * m;
  // ---- the fantasy points' rows: sum_i dHV/dY_i dY_i/dx'
  for (int e = tid; e < R * d; e += HK_WAVES * WAVE) {
    const int r = e / d, g = e - r * d;
    double s = 0.0;
    for (int i = 0; i < m; ++i) s = fma(dhv[(size_t)r * m + i], a.dY[(((size_t)b * R + r) * m + i) * d + g], s);
    a.dacq[((size_t)b * a.rows + off + r) * d + g] = gscale * s;
  }
  if (a.mask == 0) return;
  // ---- the candidate's row
  double* av = hx_smem;            // [R]: a_fp
  double* tv = av + R;             // [np_max]: t, then v
  double* qv = tv + a.np_max;      // [np_max]
  double* uv = qv + a.np_max;      // [np_max]
  double* red = uv + a.np_max;     // [HK_WAVES]
  const double* __restrict__ xb = a.x + (size_t)b * a.rows * d;
  double gx[DM];
#pragma unroll
  for (int k = 0; k < DM; ++k) gx[k] = 0.0;
  for (int i = 0; i < m; ++i) {
    if (!((a.mask >> i) & 1)) continue;  // uniform
    const dkg_output& o = a.tab[i];
    const int n = o.n, np = pad16(n);
    const double os = o.outputscale;
    const double sig = a.sig[(size_t)b * m + i];
    const double* __restrict__ tx = o.train_x;
    __syncthreads();  // the previous output's reads of the LDS vectors are done
    for (int r = tid; r < R; r += HK_WAVES * WAVE)
      av[r] = dhv[(size_t)r * m + i] * o.y_std * a.z[(size_t)(r / a.Np) * m + i] * gscale;
    __syncthreads();
    // C = sum_r a_r c(x'_r, x) and D_g = sum_r a_r s dkappa(x'_r, x)/dx'_g
    double cp = 0.0, dp[DM];
#pragma unroll
    for (int k = 0; k < DM; ++k) dp[k] = 0.0;
    for (int r = tid; r < R; r += HK_WAVES * WAVE) {
      const size_t at = ((size_t)b * R + r) * m + i;
      cp = fma(av[r], a.cxx[at], cp);
#pragma unroll
      for (int k = 0; k < DM; ++k) dp[k] = fma(av[r], a.dkx[at * d + min(k, d - 1)], dp[k]);
    }
    const double C = block_sum(cp, red);
    double il[DM], xc[DM];
    clamped_row<DM>(il, o.inv_lengthscale, d);
    scaled_point<DM>(xc, xb, il, d);
    // t_j = sum_r a_r s kappa(X_j, x'_r), the fantasy points in order (a point with a_r = 0 adds nothing)
    with_kind(o.kernel, [&](auto kind_c) {
      constexpr int KIND = decltype(kind_c)::value;
      const const_dptr tab = psi_tab();
      for (int j = tid; j < np; j += HK_WAVES * WAVE) {
        const int jc = min(j, n - 1);
        double xs[DM];
        scaled_point<DM>(xs, tx + (size_t)jc * d, il, d);
        double t = 0.0;
        for (int r = 0; r < R; ++r) {
          const double ar = av[r];
          if (ar == 0.0) continue;  // uniform
          double xr[DM];
          scaled_point<DM>(xr, xb + (size_t)(off + r) * d, il, d);
          t = fma(ar, cross_kernel_term<DM, KIND>(xr, xs, d, os, tab), t);
        }
        tv[j] = (j < n) ? t : 0.0;
      }
    });
    __syncthreads();
    tri_matvec(o.root_frag, np, tv, qv);
    __syncthreads();
    tri_matvec_t(o.root_frag, np, qv, uv);
    __syncthreads();
    // sum_j dk_j/dx_g (C w_j / sigma~^3 - u_j / sigma~)
    const double* __restrict__ wv = a.w + ((size_t)b * m + i) * HK_WSTRIDE;
    const double c3 = C / (sig * sig * sig), is = 1.0 / sig;
    double pg[DM];
#pragma unroll
    for (int k = 0; k < DM; ++k) pg[k] = 0.0;
    with_kind(o.kernel, [&](auto kind_c) {
      constexpr int KIND = decltype(kind_c)::value;
      for (int j = tid; j < n; j += HK_WAVES * WAVE) {
        double xs[DM];
        scaled_point<DM>(xs, tx + (size_t)j * d, il, d);
        const double vj = fma(c3, wv[j], -uv[j] * is);
        const double h = os * kernel_dprofile_t<KIND>(sq_dist<DM>(xc, xs, d)) * vj;
#pragma unroll
        for (int k = 0; k < DM; ++k) pg[k] = fma(h, (xc[k] - xs[k]) * il[k], pg[k]);
      }
    });
#pragma unroll
    for (int k = 0; k < DM; ++k) {
      if (k < d) {  // uniform
        const double Gk = block_sum(pg[k], red);
        const double Dk = block_sum(dp[k], red);
        gx[k] += Gk - Dk * is;
      }
    }
  }
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < DM; ++k)
      if (k < d) a.dacq[(size_t)b * a.rows * d + k] = gx[k];
  }
}

}  // namespace dkg

using namespace dkg;

namespace {

struct HvkgWs {
  size_t tab, z, w, sig, Y, cxx, dY, dkx, hv, dhv, total;
};
HvkgWs hvkg_ws(int m, int d, int Nf, int Np, int max_B) {
  const size_t B = (size_t)max_B, R = (size_t)Nf * Np, D = sizeof(double);
  HvkgWs w{};
  Carve c;
  w.tab = c.take((size_t)m * sizeof(dkg_output));
  w.z = c.take((size_t)Nf * m * D);
  w.w = c.take(B * m * HK_WSTRIDE * D);
  w.sig = c.take(B * m * D);
  w.Y = c.take(B * R * m * D);
  w.cxx = c.take(B * R * m * D);
  w.dY = c.take(B * R * m * d * D);
  w.dkx = c.take(B * R * m * d * D);
  w.hv = c.take(B * Nf * D);
  w.dhv = c.take(B * R * m * D);
  w.total = c.total();
  return w;
}

int hv_check_m(int m) {
  if (m < 1) return failf(DKG_ERR_ARG, "m=%d objectives", m);
  if (m != 2 && m != 3)
    return failf(DKG_ERR_UNSUPPORTED, "m=%d objectives: the hypervolume kernels handle m = 2 and m = 3 only", m);
  return DKG_OK;
}

// sizes only (dkg_hvkg_workspace and dkg_hvkg_init share it); 0 when they are fine
int hvkg_check_sizes(int m, int d, int Nf, int Np, int max_B) {
  if (d < 1 || Nf < 1 || Np < 1 || max_B < 1)
    return failf(DKG_ERR_ARG, "m=%d d=%d num_fantasies=%d num_pareto=%d max_B=%d", m, d, Nf, Np, max_B);
  int st = hv_check_m(m);
  if (st) return st;
  if ((st = check_dims(m, d))) return st;
  if (Nf > DKG_HVKG_MAX_FANTASIES)
    return failf(DKG_ERR_UNSUPPORTED, "num_fantasies=%d (supported <= %d)", Nf, DKG_HVKG_MAX_FANTASIES);
  if (Np > DKG_HVKG_MAX_PARETO)
    return failf(DKG_ERR_UNSUPPORTED, "num_pareto=%d (supported <= %d)", Np, DKG_HVKG_MAX_PARETO);
  if (max_B > DKG_HVKG_MAX_RESTARTS)
    return failf(DKG_ERR_UNSUPPORTED, "max_B=%d restarts (supported <= %d)", max_B, DKG_HVKG_MAX_RESTARTS);
  return DKG_OK;
}

int launch_hv(const double* Y, int S, int Np, int m, const double* ref, double* hv, double* dhv, hipStream_t s) {
  HvkgHvArgs ha{Y, hv, dhv, {0.0, 0.0, 0.0}, Np, m};
  for (int i = 0; i < m; ++i) ha.ref[i] = ref[i];
  hipLaunchKernelGGL(hvkg_hv_kernel, dim3(S), dim3(WAVE), 0, s, ha);
  return hip_status(hipGetLastError(), "hvkg_hv_kernel");
}

}  // namespace

extern "C" {

size_t dkg_hvkg_plan_bytes(void) { return sizeof(HvkgHost); }

size_t dkg_hvkg_workspace(int m, int d, int num_fantasies, int num_pareto, int max_B) {
  if (hvkg_check_sizes(m, d, num_fantasies, num_pareto, max_B) != DKG_OK) return 0;
  return hvkg_ws(m, d, num_fantasies, num_pareto, max_B).total;
}

int dkg_hvkg_init(const dkg_output* outs, int m, int d, const double* ref_point, int num_fantasies, int num_pareto,
                  const double* base_samples, unsigned mask, double current_value, double cost, int max_B,
                  void* workspace, size_t workspace_bytes, void* host_plan, void* stream) {
  if (!outs || !ref_point || !workspace || !host_plan || (mask != 0 && !base_samples))
    return failf(DKG_ERR_ARG, "NULL pointer");
  const int Nf = num_fantasies, Np = num_pareto;
  int st = hvkg_check_sizes(m, d, Nf, Np, max_B);
  if (st) return st;
  if ((mask >> m) != 0) return failf(DKG_ERR_ARG, "mask=0x%x names outputs outside [0, %d)", mask, m);
  if (mask == 0 && Nf != 1)
    return failf(DKG_ERR_ARG, "an empty mask selects the value function, which takes num_fantasies = 1; got %d", Nf);
  if (!(cost > 0.0) || !std::isfinite(cost)) return failf(DKG_ERR_ARG, "cost=%g is not positive", cost);
  if (!std::isfinite(current_value)) return failf(DKG_ERR_ARG, "current_value=%g", current_value);
  int np_max = 16;
  for (int k = 0; k < m; ++k) {
    char who[32];
    std::snprintf(who, sizeof who, "output %d", k);
    if ((st = check_output_state(outs[k], true, who))) return st;
    np_max = std::max(np_max, pad16(outs[k].n));
  }
  const HvkgWs w = hvkg_ws(m, d, Nf, Np, max_B);
  if (workspace_bytes < w.total)
    return failf(DKG_ERR_WORKSPACE, "workspace %zu bytes < required %zu", workspace_bytes, w.total);
  HvkgHost* h = static_cast<HvkgHost*>(host_plan);
  std::memset(h, 0, sizeof(HvkgHost));
  std::memcpy(h->tab, outs, (size_t)m * sizeof(dkg_output));
  if (mask != 0) std::memcpy(h->z, base_samples, (size_t)Nf * m * sizeof(double));
  HvkgPlan& p = h->plan;
  p.m = m; p.d = d; p.Nf = Nf; p.Np = Np; p.R = Nf * Np; p.rows = p.R + (mask != 0 ? 1 : 0);
  p.mask = (int)mask; p.max_B = max_B; p.np_max = np_max;
  for (int i = 0; i < m; ++i) p.ref[i] = ref_point[i];
  p.current = current_value; p.cost = cost;
  p.tab = at<const dkg_output>(workspace, w.tab);
  p.z = at<const double>(workspace, w.z);
  p.w = at<double>(workspace, w.w);
  p.sig = at<double>(workspace, w.sig);
  p.Y = at<double>(workspace, w.Y);
  p.cxx = at<double>(workspace, w.cxx);
  p.dY = at<double>(workspace, w.dY);
  p.dkx = at<double>(workspace, w.dkx);
  p.hv = at<double>(workspace, w.hv);
  p.dhv = at<double>(workspace, w.dhv);
  hipStream_t s = (hipStream_t)stream;
  st = hip_status(hipMemcpyAsync(at<char>(workspace, w.tab), h->tab, (size_t)m * sizeof(dkg_output),
                                 hipMemcpyHostToDevice, s),
                  "dkg_hvkg_init: table upload");
  if (st) return st;
  st = hip_status(hipMemcpyAsync(at<char>(workspace, w.z), h->z, (size_t)Nf * m * sizeof(double),
                                 hipMemcpyHostToDevice, s),
                  "dkg_hvkg_init: base samples upload");
  if (st) return st;
  p.magic = HVKG_MAGIC;
  return DKG_OK;
}

int dkg_hvkg_forward(const void* host_plan, const double* x_full, int B, double* acq, double* dacq_dx, double* y_out,
                     void* stream) {
  if (!host_plan || !x_full || !acq) return failf(DKG_ERR_ARG, "NULL pointer");
  const HvkgHost* h = static_cast<const HvkgHost*>(host_plan);
  const HvkgPlan& p = h->plan;
  if (p.magic != HVKG_MAGIC) return failf(DKG_ERR_ARG, "the plan is not initialised (dkg_hvkg_init)");
  if (B < 1 || B > p.max_B) return failf(DKG_ERR_ARG, "B=%d restarts outside [1, max_B=%d]", B, p.max_B);
  hipStream_t s = (hipStream_t)stream;
  const int grad = dacq_dx != nullptr;
  const int npw = p.np_max;
  const dim3 block(HK_WAVES * WAVE);
  int st;
  if (p.mask != 0) {
    HvkgCandArgs ca{p.tab, x_full, p.w, p.sig, p.m, p.d, p.rows, p.mask};
    const size_t lds = (2 * (size_t)npw + HK_WAVES) * sizeof(double);
    by_dim(p.d, [&](auto dm) { launch_lds(hvkg_cand_kernel<decltype(dm)::value>, dim3(B, p.m), block, lds, s, ca); });
    st = hip_status(hipGetLastError(), "hvkg_cand_kernel");
    if (st) return st;
  }
  HvkgFanArgs fa{p.tab, x_full, p.z, p.w, p.sig, p.Y, p.cxx, p.dY, p.dkx, y_out,
                 p.m, p.d, p.R, p.Np, p.rows, p.mask, grad};
  by_dim(p.d, [&](auto dm) {
    launch_lds(hvkg_fantasy_kernel<decltype(dm)::value>, dim3((p.R + HK_POINTS - 1) / HK_POINTS, p.m, B), block,
               hvkg_fan_lds_bytes(npw, p.d), s, fa);
  });
  st = hip_status(hipGetLastError(), "hvkg_fantasy_kernel");
  if (st) return st;
  st = launch_hv(p.Y, B * p.Nf, p.Np, p.m, p.ref, p.hv, grad ? p.dhv : nullptr, s);
  if (st) return st;
  HvkgFinArgs xa{p.tab, x_full, p.z, p.w, p.sig, p.cxx, p.dY, p.dkx, p.hv, p.dhv, acq, dacq_dx,
                 p.current, p.cost, p.m, p.d, p.Nf, p.Np, p.R, p.rows, p.mask, npw};
  by_dim(p.d, [&](auto dm) {
    launch_lds(hvkg_finish_kernel<decltype(dm)::value>, dim3(B), block, hvkg_fin_lds_bytes(p.R, npw), s, xa);
  });
  return hip_status(hipGetLastError(), "hvkg_finish_kernel");
}

int dkg_hypervolume(const double* Y, int S, int num_pareto, int m, const double* ref_point, double* hv, double* dhv,
                    void* stream) {
  if (!Y || !ref_point || !hv) return failf(DKG_ERR_ARG, "NULL pointer");
  if (S < 1 || num_pareto < 1) return failf(DKG_ERR_ARG, "S=%d sets of num_pareto=%d points", S, num_pareto);
  int st = hv_check_m(m);
  if (st) return st;
  if (num_pareto > DKG_HVKG_MAX_PARETO)
    return failf(DKG_ERR_UNSUPPORTED, "num_pareto=%d (supported <= %d)", num_pareto, DKG_HVKG_MAX_PARETO);
  return launch_hv(Y, S, num_pareto, m, ref_point, hv, dhv, (hipStream_t)stream);
}

}  // extern "C"
