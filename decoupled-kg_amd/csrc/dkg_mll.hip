// Marginal log-likelihood of the fitted state and its gradient in the hyperparameters (gfx950): the objective
// of the MAP fit (dkg_amd/fit.py; the reference's fit_gpytorch_mll on ExactMarginalLogLikelihood,
// modules/model/factory.py:24-151, pipeline/nodes/bo_loop.py:63-79, 589-619), from the caches the state
// preparation builds (dkg_linalg.hip): L = chol(K), M = L^{-1}, alpha = M^T M r with r = y - c.
//   value    = -1/2 r.alpha - sum_i log L_ii - (n / 2) log 2 pi
//   G = M^T M = K^{-1},  W = alpha alpha^T - G,  t_ik = (x_i - x_k) / l (componentwise)
//   d/dc     = sum_i alpha_i
//   d/dnoise = 1/2 tr W
//   d/ds     = 1/2 sum_ik W_ik kappa(|t_ik|^2)
//   d/dl_j   = -1/2 sum_ik W_ik s h(|t_ik|^2) t_ik,j^2 / l_j        (h = kappa'(r) / r, kernel_dprofile)
// Two kernels, all outputs side by side (blockIdx.y = output):
//   mll_grad_kernel      one workgroup per 32 x 32 tile (ti >= tj) of the pair space: its tile of G by MFMA,
//                        kept in registers, contracted there with kappa, h and t^2 into d + 2 partial sums
//   mll_finalize_kernel  one workgroup per output: the partials in tile order, sum alpha, sum log L_ii, r.alpha
// K^{-1} is never written to memory.  Every sum runs in a fixed order (no atomics): same bits on every call.
#include <algorithm>

#include "dkg_kernels.h"

namespace dkg {

// Tile (ti, tj) of G: G_ik = sum_q M[q][i] M[q][k].  M is lower triangular, so the sum starts at the tile's
// first row 32 ti (entries with q < i are masked to zero, whatever the upper triangle holds).  Wave w takes
// the 16 x 16 sub-tile (w >> 1, w & 1); both MFMA operands are row segments of M: A[i][kk] = M[q0 + kk][i0 + i],
// lane l: M[q0 + (l >> 4)][i0 + (l & 15)], and the same with k0 for B.  Rows and columns past n are masked, not
// read.  Off-diagonal tiles count twice (W, kappa, h and t^2 are symmetric); a diagonal tile counts its full
// square once.
__global__ __launch_bounds__(256) void mll_grad_kernel(MllBatch bt) {
  constexpr int DM = DKG_MAX_DIM;
  __shared__ double sXi[MLL_TB][DM + 1], sXk[MLL_TB][DM + 1];
  __shared__ double sAi[MLL_TB], sAk[MLL_TB];
  __shared__ double sPart[4][MLL_NP];
  const int o = blockIdx.y;
  const dkg_output& oo = bt.o[o];
  const int n = oo.n, d = bt.d;
  if (n <= 0 || *bt.info[o] != 0) return;
  if ((int)blockIdx.x >= mll_tiles(n)) return;
  int ti, tj;
  lower_tile(blockIdx.x, ti, tj);
  const int i0 = ti * MLL_TB, k0 = tj * MLL_TB;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int si = wave >> 1, sj = wave & 1;
  const double* __restrict__ M = bt.M[o];

  // the tile's training rows and alpha entries (zero past n)
  for (int e = tid; e < MLL_TB * d; e += blockDim.x) {
    const int r = e / d, j = e - r * d;
    sXi[r][j] = (i0 + r < n) ? oo.train_x[(size_t)(i0 + r) * d + j] : 0.0;
    sXk[r][j] = (k0 + r < n) ? oo.train_x[(size_t)(k0 + r) * d + j] : 0.0;
  }
  if (tid < MLL_TB) {
    sAi[tid] = (i0 + tid < n) ? bt.alpha[o][i0 + tid] : 0.0;
    sAk[tid] = (k0 + tid < n) ? bt.alpha[o][k0 + tid] : 0.0;
  }

  // G tile: k-loop over the rows q >= 32 ti of M, U steps of 4 rows with every load in flight at once
  const int ca = i0 + 16 * si + (lane & 15), cb = k0 + 16 * sj + (lane & 15);
  const int qq = lane >> 4;
  d4 acc = {0.0, 0.0, 0.0, 0.0};
  constexpr int U = 8;
  for (int q0 = i0; q0 < n; q0 += 4 * U) {
    double a[U], b[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int q = q0 + 4 * u + qq;
      a[u] = (q < n && ca < n && q >= ca) ? M[(size_t)q * n + ca] : 0.0;
      b[u] = (q < n && cb < n && q >= cb) ? M[(size_t)q * n + cb] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) acc = mfma_f64(a[u], b[u], acc);
  }
  __syncthreads();

  // epilogue, in registers: lane l, register r holds G[i0 + 16 si + (l >> 4) + 4 r][k0 + 16 sj + (l & 15)]
  const int kind = oo.kernel;
  const double* __restrict__ il = oo.inv_lengthscale;
  const int kc = 16 * sj + (lane & 15);
  const bool kin = k0 + kc < n;
  const double ak = sAk[kc];
  const double w2 = (ti != tj) ? 2.0 : 1.0;
  double xk[DM], sl[DM];
#pragma unroll
  for (int j = 0; j < DM; ++j) {
    xk[j] = (j < d) ? sXk[kc][j] : 0.0;
    sl[j] = 0.0;
  }
  double s_tr = 0.0, s_kap = 0.0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int ir = 16 * si + (lane >> 4) + 4 * r;
    const bool in = kin && (i0 + ir < n);
    const double w = in ? fma(sAi[ir], ak, -acc[r]) : 0.0;
    double tt[DM];
    double r2 = 0.0;
#pragma unroll
    for (int j = 0; j < DM; ++j) {
      if (j < d) {  // wave-uniform
        const double t = (sXi[ir][j] - xk[j]) * il[j];
        tt[j] = t * t;
        r2 = fma(t, t, r2);  // scaled_r2's order: the r^2 the kernel matrix was built from
      } else {
        tt[j] = 0.0;
      }
    }
    const double kap = kernel_profile(kind, r2);
    const double wh = w2 * w * kernel_dprofile(kind, r2);
    s_kap = fma(w2 * w, kap, s_kap);
    if (i0 + ir == k0 + kc) s_tr += w;
#pragma unroll
    for (int j = 0; j < DM; ++j) sl[j] = fma(wh, tt[j], sl[j]);
  }
  s_tr = wave_sum(s_tr);
  s_kap = wave_sum(s_kap);
#pragma unroll
  for (int j = 0; j < DM; ++j)
    if (j < d) sl[j] = wave_sum(sl[j]);  // wave-uniform
  if (lane == 0) {
    sPart[wave][0] = s_tr;
    sPart[wave][1] = s_kap;
#pragma unroll
    for (int j = 0; j < DM; ++j) sPart[wave][2 + j] = sl[j];
  }
  __syncthreads();
  if (tid < MLL_NP)  // the four waves in wave order
    bt.part[o][(size_t)blockIdx.x * MLL_NP + tid] =
        ((sPart[0][tid] + sPart[1][tid]) + sPart[2][tid]) + sPart[3][tid];
}

// One workgroup of four waves per output: wave 0 sum alpha, wave 1 sum log L_ii, wave 2 r.alpha (lane partials
// over i = lane, lane + 64, ... in order, then the wave butterfly), wave 3 the tile partials, lane p summing
// entry p over the tiles in tile order.  out = [value, d/dc, d/dl_1 .. d/dl_d, d/ds, d/dnoise].
__global__ __launch_bounds__(256) void mll_finalize_kernel(MllBatch bt) {
  __shared__ double sS[3];
  __shared__ double sP[MLL_NP];
  const int o = blockIdx.x;
  const dkg_output& oo = bt.o[o];
  const int n = oo.n, d = bt.d;
  if (n <= 0 || *bt.info[o] != 0) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double* __restrict__ alpha = bt.alpha[o];
  if (wave < 3) {
    const double c = oo.mean_constant;
    double s = 0.0;
    for (int i = lane; i < n; i += 64) {
      if (wave == 0) s += alpha[i];
      else if (wave == 1) s += log(bt.L[o][(size_t)i * n + i]);
      else s = fma(bt.y[o][i] - c, alpha[i], s);
    }
    s = wave_sum(s);
    if (lane == 0) sS[wave] = s;
  } else if (lane < MLL_NP) {
    const int T = mll_tiles(n);
    const double* __restrict__ part = bt.part[o];
    double s = 0.0;
    constexpr int U = 16;  // loads in flight; the sum keeps the tile order
    for (int t0 = 0; t0 < T; t0 += U) {
      double v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) v[u] = (t0 + u < T) ? part[(size_t)(t0 + u) * MLL_NP + lane] : 0.0;
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (t0 + u < T) s += v[u];
    }
    sP[lane] = s;
  }
  __syncthreads();
  double* __restrict__ out = bt.out[o];
  if (tid == 0) {
    out[0] = -0.5 * sS[2] - sS[1] - 0.5 * n * 1.8378770664093453;  // log 2 pi
    out[1] = sS[0];
    out[2 + d] = 0.5 * sP[1];
    out[3 + d] = 0.5 * sP[0];
  }
  if (tid < d) out[2 + tid] = -0.5 * oo.outputscale * oo.inv_lengthscale[tid] * sP[2 + tid];
}

hipError_t launch_mll(const MllBatch& b, int m, hipStream_t s) {
  int nmax = 0;
  for (int i = 0; i < m; ++i) nmax = std::max(nmax, (int)b.o[i].n);
  hipLaunchKernelGGL(mll_grad_kernel, dim3(mll_tiles(nmax), m), dim3(256), 0, s, b);
  hipLaunchKernelGGL(mll_finalize_kernel, dim3(m), dim3(256), 0, s, b);
  return hipGetLastError();
}

}  // namespace dkg
