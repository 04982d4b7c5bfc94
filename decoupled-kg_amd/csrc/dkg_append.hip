// One observation appended to an output's fitted state without refactorising (gfx950): the bordered
// Cholesky update of the caches dkg_prepare_output / dkg_cross_root build (dkg_linalg.hip).  The reference
// rebuilds its model, and with it every posterior cache, at each BO iteration (bo_loop.py:457-465; the
// caches sit behind model.posterior, discretekg.py:182-185); a decoupled step adds one row to one output.
// With M = L^{-1}, k = s kappa(X, x_new), r' = y' - c and j the jitter of the old factorisation:
//   l = M k,  lambda^2 = s kappa(x, x) + noise + j - l.l          (not positive definite when <= 0)
//   L' = [[L, 0], [l^T, lambda]],  M' = [[M, 0], [-(l^T M) / lambda, 1 / lambda]]
//   beta' = M' r' (its last entry by forward substitution, (r'_n - l.beta) / lambda),  alpha' = M'^T beta'
//   Q_D' = [Q_D, (s kappa(D, x_new) - Q_D l) / lambda],  mu_D' = c + Q_D' beta'
// Three kernels, all out of place (the old arrays are only read):
//   append_copy_kernel   rows 0..n-1 of L' and M' (the old rows and a zero column)
//   append_solve_kernel  one workgroup: k, l, lambda, the new rows of L' and M', beta', alpha', the info flag
//   append_disc_kernel   one workgroup per 16-row tile of D: the old disc_frag streamed in fragment order
//                        into the layout of n_pad(n + 1) with the new column, and mu_D'
// root_frag' comes from M' by pack_linv_kernel.  Every reduction runs in a fixed order.
#include <algorithm>

#include "dkg_kernels.h"

namespace dkg {

// Rows r < n of L' and M': [old row, 0].
__global__ __launch_bounds__(256) void append_copy_kernel(const double* __restrict__ L, const double* __restrict__ M,
                                                          int n, double* __restrict__ Ln, double* __restrict__ Mn) {
  const int n1 = n + 1;
  const size_t total = (size_t)n * n1;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const size_t r = e / n1;
    const int c = (int)(e - r * n1);
    const bool in = c < n;
    Ln[e] = in ? L[r * n + c] : 0.0;
    Mn[e] = in ? M[r * n + c] : 0.0;
  }
}

// The solve, one workgroup of 16 waves (as alpha_kernel): two passes over M, rows then columns.
//   pass 1 (one row per wave, lanes along the row):  l = M k  and  beta = M r'[0..n)
//   lambda, beta'_n                                  every wave forms them from the same LDS values: same bits
//   pass 2 (64 columns per step, wave w the rows w mod 16, partials met in LDS in wave order):
//          w = M^T l (the new row of M' is -w / lambda)  and  M^T beta (alpha' = M^T beta + M'_n beta'_n)
// K entries as kernel_matrix_kernel forms them (outputscale * kernel_profile; the diagonal's noise + jitter
// added as one number).  Leaves l, beta' and lambda in the workspace for append_disc_kernel.
__global__ __launch_bounds__(1024) void append_solve_kernel(AppendArgs a) {
  __shared__ double sk[1024], sr[1024], sl[1024], sb[1024];
  __shared__ double part[2][16][64];
  const int n = a.o.n, n1 = n + 1, d = a.d, tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
  const double* __restrict__ M = a.M;
  const double* xnew = a.xt + (size_t)n * d;
  const double c = a.o.mean_constant;
  for (int i = tid; i < n; i += blockDim.x) {
    sk[i] = a.o.outputscale * kernel_profile(a.o.kernel, scaled_r2(a.xt + (size_t)i * d, xnew, a.o.inv_lengthscale, d));
    sr[i] = a.y[i] - c;
  }
  __syncthreads();
  // (a wave keeps RU of its rows in flight at once: one workgroup's passes over M are bound by the latency of
  // its loads, not by arithmetic; each row's sum keeps its order, lane partials in q order, then wave_sum)
  constexpr int RU = 4;
  for (int i0 = wave; i0 < n; i0 += RU * nw) {
    double s1[RU], s2[RU];
#pragma unroll
    for (int u = 0; u < RU; ++u) s1[u] = s2[u] = 0.0;
    const int ilast = min(i0 + (RU - 1) * nw, n - 1);
    for (int q = lane; q <= ilast; q += 64) {
      const double kq = sk[q], rq = sr[q];
      double mv[RU];
#pragma unroll
      for (int u = 0; u < RU; ++u) {
        const int i = i0 + u * nw;
        mv[u] = (i < n && q <= i) ? M[(size_t)i * n + q] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < RU; ++u) {
        if (q <= i0 + u * nw) {
          s1[u] = fma(mv[u], kq, s1[u]);
          s2[u] = fma(mv[u], rq, s2[u]);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < RU; ++u) {
      const int i = i0 + u * nw;
      if (i < n) {  // wave-uniform
        const double a1 = wave_sum(s1[u]), a2 = wave_sum(s2[u]);
        if (lane == 0) {
          sl[i] = a1;
          sb[i] = a2;
        }
      }
    }
  }
  __syncthreads();
  double pl = 0.0, pb = 0.0;
  for (int i = lane; i < n; i += 64) {
    pl = fma(sl[i], sl[i], pl);
    pb = fma(sl[i], sb[i], pb);
  }
  const double ll = wave_sum(pl), lb = wave_sum(pb);
  const double kdiag = a.o.outputscale * kernel_profile(a.o.kernel, 0.0) + a.diag;
  const double lam2 = kdiag - ll;
  if (!(lam2 > 0.0) || !isfinite(lam2)) {  // the same value in every wave: the whole workgroup leaves
    if (tid == 0) *a.info = n1;            // potrf's convention: the failing column + 1
    return;
  }
  const double lam = sqrt(lam2);
  const double bn = ((a.y[n] - c) - lb) / lam;
  for (int g0 = 0; g0 < pad16(n1); g0 += 64) {
    const int q = g0 + lane;
    double s1 = 0.0, s2 = 0.0;
    if (q < n) {
      const int i1 = q + ((wave - q) % nw + nw) % nw;  // first row >= q with i = wave (mod nw)
      constexpr int CU = 8;  // loads in flight per lane; the sums keep their row order
      for (int i = i1; i < n; i += CU * nw) {
        double mv[CU];
#pragma unroll
        for (int u = 0; u < CU; ++u) {
          const int iu = i + u * nw;
          mv[u] = (iu < n) ? M[(size_t)iu * n + q] : 0.0;  // coalesced across lanes
        }
#pragma unroll
        for (int u = 0; u < CU; ++u) {
          const int iu = i + u * nw;
          if (iu < n) {
            s1 = fma(mv[u], sl[iu], s1);
            s2 = fma(mv[u], sb[iu], s2);
          }
        }
      }
    }
    part[0][wave][lane] = s1;
    part[1][wave][lane] = s2;
    __syncthreads();
    if (wave == 0 && q < pad16(n1)) {
      double w = 0.0, av = 0.0;
      for (int w2 = 0; w2 < nw; ++w2) {
        w += part[0][w2][lane];
        av += part[1][w2][lane];
      }
      if (q < n) {
        const double u = -w / lam;
        a.Ln[(size_t)n * n1 + q] = sl[q];
        a.Mn[(size_t)n * n1 + q] = u;
        a.alpha[q] = fma(u, bn, av);
      } else if (q == n) {
        a.Ln[(size_t)n * n1 + n] = lam;
        a.Mn[(size_t)n * n1 + n] = 1.0 / lam;
        a.alpha[n] = bn / lam;
      } else {
        a.alpha[q] = 0.0;
      }
    }
    __syncthreads();
  }
  for (int i = tid; i < 1024; i += blockDim.x) {
    a.lvec[i] = (i < n) ? sl[i] : 0.0;
    a.beta[i] = (i < n) ? sb[i] : (i == n) ? bn : 0.0;
  }
  if (tid == 0) *a.lam = lam;
}

// One 16-row tile of D per workgroup of four waves.  Wave w takes the old tile's 1 KiB pairs j = w (mod 4)
// (lane l of pair j holds rows 16 t + (l & 15), columns 8 j + (l >> 4) and 8 j + 4 + (l >> 4): one 16-byte
// load per lane), adds them into its dots with l and beta' and stores them at the same pair of the new
// tile, whose stride is that of n_pad(n + 1): when n + 1 crosses a multiple of 16 this is the relayout.
// The partial dots meet in LDS in a fixed order; lanes 0-15 then form the new column and the mean, and the
// pair that holds column n is stored last with it (a crossing: that pair and the next are new, zero
// elsewhere).  Rows past N stay exactly zero.
__global__ __launch_bounds__(256) void append_disc_kernel(AppendArgs a) {
  __shared__ double sl[1024], sb[1024];
  __shared__ double part[2][4][64];
  __shared__ double sq[16];
  if (*a.info != 0) return;
  const int n = a.o.n, npo = pad16(n), npn = pad16(n + 1);
  const int po = npo >> 3, pn = npn >> 3;  // pairs per tile, old and new
  const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4;
  for (int q = tid; q < npo; q += blockDim.x) {
    sl[q] = (q < n) ? a.lvec[q] : 0.0;
    sb[q] = (q < n) ? a.beta[q] : 0.0;
  }
  __syncthreads();
  const double2* __restrict__ src = reinterpret_cast<const double2*>(a.o.disc_frag) + (size_t)t * po * 64 + lane;
  double2* __restrict__ dst = reinterpret_cast<double2*>(a.qn) + (size_t)t * pn * 64 + lane;
  const int jn = n >> 3;  // the pair that holds column n
  double accl = 0.0, accb = 0.0;
#pragma unroll 4
  for (int j = wave; j < po; j += 4) {
    const double2 v = src[(size_t)j * 64];
    const int c0 = 8 * j + g;
    accl = fma(v.x, sl[c0], accl);
    accl = fma(v.y, sl[c0 + 4], accl);
    accb = fma(v.x, sb[c0], accb);
    accb = fma(v.y, sb[c0 + 4], accb);
    if (j != jn) dst[(size_t)j * 64] = v;
  }
  part[0][wave][lane] = accl;
  part[1][wave][lane] = accb;
  __syncthreads();
  if (tid < 16) {
    const int row = 16 * t + tid;
    double dl = 0.0, db = 0.0;
#pragma unroll
    for (int w = 0; w < 4; ++w)
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        dl += part[0][w][16 * h + tid];
        db += part[1][w][16 * h + tid];
      }
    double qv = 0.0, mu = 0.0;
    if (row < a.N) {
      const double kv = a.o.outputscale * kernel_profile(a.o.kernel, scaled_r2(a.disc + (size_t)row * a.d,
                                                                               a.xt + (size_t)n * a.d,
                                                                               a.o.inv_lengthscale, a.d));
      qv = (kv - dl) / *a.lam;
      mu = a.o.mean_constant + fma(qv, a.beta[n], db);
    }
    a.mean[row] = mu;
    sq[tid] = qv;
  }
  __syncthreads();
  if (wave == 0) {
    double2 v = make_double2(0.0, 0.0);
    if (jn < po) v = src[(size_t)jn * 64];
    if (g == (n & 3)) {
      if ((n >> 2) & 1) v.y = sq[lane & 15];
      else v.x = sq[lane & 15];
    }
    dst[(size_t)jn * 64] = v;
  } else if (wave == 1 && pn > po) {
    dst[(size_t)(po + 1) * 64] = make_double2(0.0, 0.0);
  }
}

hipError_t launch_append(const AppendArgs& a, double* root_frag, hipStream_t s) {
  const int n = a.o.n;
  const size_t total = (size_t)n * (n + 1);
  const int blocks = (int)std::min<size_t>((total + 255) / 256, 4096);
  hipLaunchKernelGGL(append_copy_kernel, dim3(blocks), dim3(256), 0, s, a.L, a.M, n, a.Ln, a.Mn);
  hipLaunchKernelGGL(append_solve_kernel, dim3(1), dim3(1024), 0, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if ((e = launch_pack_linv(a.Mn, n + 1, root_frag, s)) != hipSuccess) return e;
  if (a.N > 0) hipLaunchKernelGGL(append_disc_kernel, dim3(pad16(a.N) / 16), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace dkg
