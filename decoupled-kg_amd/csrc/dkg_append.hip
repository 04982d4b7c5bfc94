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

// ---------------------------------------------------------------------------------------------------------------
// A block of K <= 32 rows appended to J states at once (dkg_append_rows; include/dkg.h has the math).  Every launch
// carries all jobs, blockIdx.y (z in rows_w_kernel) the job; the work of a job is laid out by its own n, K and N
// alone, so its bits do not depend on the call it rides in.  The kernels carry K + 1 vectors through both passes
// over M: the K rows of B = s kappa(X2, X) M^T, and beta = M r' with them, then W = B M and M^T beta.
//   rows_copy_kernel    rows 0..n-1 of L' and M' (the old rows and K zeros)
//   rows_kx_kernel      kx = s kappa(X2, X) with r' as row K, and kd = s kappa(X2, D)
//   rows_b_kernel       bx[k][i] = sum_{q <= i} kx[k][q] M[i][q]: four rows of M per workgroup, one per wave, lanes
//                       along the row (q order), then wave_sum
//   rows_w_kernel       one (64-column slab, 128-row chunk) of M per workgroup: lane = column, wave w the rows
//                       w mod 4 in row order, the waves met in LDS in wave order; the chunks' partials go to wp
//   rows_chol_kernel    one workgroup per job: S, its Cholesky in LDS, C^{-1}, beta2, gamma, the K new rows of L'
//                       and the right block of M's, the job's status
//   rows_finish_kernel  per column: the chunks' partials summed in chunk order, the new rows of M', alpha'
//   rows_pack_kernel    root_frag' from M' (pack_linv_kernel's map)
//   rows_disc_kernel    one 16-row tile of D per workgroup: the old disc_frag streamed into the layout of
//                       n_pad(n + K) (the relayout when a multiple of 16 is crossed), the K new columns, mu_D'
// A job that is not positive definite writes its status and nothing the later kernels of another job read; the
// kernels after rows_chol_kernel leave such a job alone.

__global__ __launch_bounds__(256) void rows_copy_kernel(const RowsJob* __restrict__ jobs) {
  const RowsJob& a = jobs[blockIdx.y];
  const int n = a.o.n, n1 = n + a.K;
  const size_t total = (size_t)n * n1;
  const double* __restrict__ L = a.L;
  const double* __restrict__ M = a.M;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const size_t r = e / n1;
    const int c = (int)(e - r * n1);
    const bool in = c < n;
    a.Ln[e] = in ? L[r * n + c] : 0.0;
    a.Mn[e] = in ? M[r * n + c] : 0.0;
  }
}

// blockIdx.x = k: row k < K of kx (padding to np zero) and of kd (rows past N zero); k = K: r' = y - c.
__global__ __launch_bounds__(256) void rows_kx_kernel(const RowsJob* __restrict__ jobs, int d) {
  const RowsJob& a = jobs[blockIdx.y];
  const int n = a.o.n, K = a.K, np = pad16(n), k = blockIdx.x;
  if (k > K) return;
  double* __restrict__ row = a.kx + (size_t)k * np;
  if (k == K) {
    for (int q = threadIdx.x; q < np; q += blockDim.x) row[q] = (q < n) ? a.y[q] - a.o.mean_constant : 0.0;
    return;
  }
  const double* xk = a.xt + (size_t)(n + k) * d;
  for (int q = threadIdx.x; q < np; q += blockDim.x)
    row[q] = (q < n) ? a.o.outputscale * kernel_profile(a.o.kernel, scaled_r2(a.xt + (size_t)q * d, xk,
                                                                               a.o.inv_lengthscale, d))
                     : 0.0;
  const int Np = pad16(a.N);
  double* __restrict__ kd = a.kd + (size_t)k * Np;
  for (int q = threadIdx.x; q < Np; q += blockDim.x)
    kd[q] = (q < a.N) ? a.o.outputscale * kernel_profile(a.o.kernel, scaled_r2(a.disc + (size_t)q * d, xk,
                                                                                a.o.inv_lengthscale, d))
                      : 0.0;
}

// bx[k][i] for the four rows i of M this workgroup holds, one per wave (rows n..np-1: zero), k <= K.
__global__ __launch_bounds__(256) void rows_b_kernel(const RowsJob* __restrict__ jobs) {
  const RowsJob& a = jobs[blockIdx.y];
  const int n = a.o.n, K = a.K, np = pad16(n);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double* __restrict__ M = a.M;
  const double* __restrict__ kx = a.kx;
  const int i = 4 * blockIdx.x + wave;  // wave-uniform
  if (i >= np) return;
  double acc[ROWS_MAX + 1];
#pragma unroll
  for (int k = 0; k <= ROWS_MAX; ++k) acc[k] = 0.0;
  if (i < n) {
    for (int q = lane; q <= i; q += 64) {
      const double mv = M[(size_t)i * n + q];
#pragma unroll
      for (int k = 0; k <= ROWS_MAX; ++k)
        if (k <= K) acc[k] = fma(mv, kx[(size_t)k * np + q], acc[k]);
    }
  }
#pragma unroll
  for (int k = 0; k <= ROWS_MAX; ++k) {
    if (k <= K) {
      const double sum = wave_sum(acc[k]);
      if (lane == 0) a.bx[(size_t)k * np + i] = sum;
    }
  }
}

// wp[rc][k][q] = sum over the chunk's rows i >= q of bx[k][i] M[i][q], k <= K (chunks above the diagonal: zero).
__global__ __launch_bounds__(256) void rows_w_kernel(const RowsJob* __restrict__ jobs) {
  __shared__ double part[3][ROWS_MAX + 1][64];
  const RowsJob& a = jobs[blockIdx.z];
  const int n = a.o.n, K = a.K, np = pad16(n);
  const int rc = blockIdx.y, q0 = 64 * blockIdx.x;
  if (q0 >= np || rc * ROWS_CHUNK >= n) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = q0 + lane;
  const double* __restrict__ M = a.M;
  const double* __restrict__ bx = a.bx;
  const int iend = min((rc + 1) * ROWS_CHUNK, n);
  double acc[ROWS_MAX + 1];
#pragma unroll
  for (int k = 0; k <= ROWS_MAX; ++k) acc[k] = 0.0;
  constexpr int CU = 8;  // loads in flight per lane; the sums keep their row order
  if (iend > q0) {       // wave-uniform: the chunk reaches the slab's diagonal
    for (int i = rc * ROWS_CHUNK + wave; i < iend; i += 4 * CU) {
      double mv[CU];
#pragma unroll
      for (int u = 0; u < CU; ++u) {
        const int iu = i + 4 * u;
        mv[u] = (iu < iend && q < n && q <= iu) ? M[(size_t)iu * n + q] : 0.0;  // coalesced across lanes
      }
#pragma unroll
      for (int u = 0; u < CU; ++u) {
        const int iu = min(i + 4 * u, iend - 1);  // past the end: mv = 0
#pragma unroll
        for (int k = 0; k <= ROWS_MAX; ++k)
          if (k <= K) acc[k] = fma(mv[u], bx[(size_t)k * np + iu], acc[k]);
      }
    }
  }
  if (wave > 0) {
#pragma unroll
    for (int k = 0; k <= ROWS_MAX; ++k)
      if (k <= K) part[wave - 1][k][lane] = acc[k];
  }
  __syncthreads();
  if (wave == 0 && q < np) {
    double* __restrict__ wp = a.wp + (size_t)rc * (K + 1) * np;
#pragma unroll
    for (int k = 0; k <= ROWS_MAX; ++k)
      if (k <= K) wp[(size_t)k * np + q] = ((acc[k] + part[0][k][lane]) + part[1][k][lane]) + part[2][k][lane];
  }
}

// One workgroup of 16 waves per job.  S's lower triangle and r'[n..) - B beta by one wave per entry (lanes along
// i, wave_sum), the Cholesky column by column in LDS (thread r = row r), C^{-1} a column per thread.
__global__ __launch_bounds__(1024) void rows_chol_kernel(const RowsJob* __restrict__ jobs, int d,
                                                         int* __restrict__ info) {
  __shared__ double sS[ROWS_MAX][ROWS_MAX + 1], sI[ROWS_MAX][ROWS_MAX + 1];
  __shared__ double sres[ROWS_MAX], sb2[ROWS_MAX], sg[ROWS_MAX];
  const RowsJob& a = jobs[blockIdx.x];
  const int n = a.o.n, K = a.K, np = pad16(n), n1 = n + K;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double* __restrict__ bx = a.bx;
  const int T = K * (K + 1) / 2;
  for (int e = wave; e < T + K; e += 16) {  // wave-uniform
    int ra, rb;
    if (e < T) lower_tile(e, ra, rb);
    else ra = e - T, rb = K;
    double p = 0.0;
    for (int i = lane; i < n; i += 64) p = fma(bx[(size_t)ra * np + i], bx[(size_t)rb * np + i], p);
    const double dot = wave_sum(p);
    if (lane == 0) {
      if (e < T) {
        const double kab = a.o.outputscale * kernel_profile(a.o.kernel, scaled_r2(a.xt + (size_t)(n + ra) * d,
                                                                                  a.xt + (size_t)(n + rb) * d,
                                                                                  a.o.inv_lengthscale, d));
        sS[ra][rb] = ((ra == rb) ? kab + a.diag : kab) - dot;
      } else {
        sres[ra] = (a.y[n + ra] - a.o.mean_constant) - dot;
      }
    }
  }
  for (int j = 0; j < K; ++j) {
    __syncthreads();
    const double piv = sS[j][j];  // the same value in every thread
    if (!(piv > 0.0) || !isfinite(piv)) {
      if (tid == 0) info[blockIdx.x] = n + j + 1;  // potrf's convention: the failing column + 1
      return;
    }
    const double l = sqrt(piv);
    __syncthreads();
    if (tid == j) sS[j][j] = l;
    if (tid > j && tid < K) sS[tid][j] = sS[tid][j] / l;
    __syncthreads();
    if (tid > j && tid < K) {
      const double lr = sS[tid][j];
      for (int c = j + 1; c <= tid; ++c) sS[tid][c] = fma(-lr, sS[c][j], sS[tid][c]);
    }
  }
  __syncthreads();
  if (tid < K) {  // column tid of C^{-1}
    const int c = tid;
    for (int r = 0; r < c; ++r) sI[r][c] = 0.0;
    sI[c][c] = 1.0 / sS[c][c];
    for (int r = c + 1; r < K; ++r) {
      double acc = 0.0;
      for (int t = c; t < r; ++t) acc = fma(sS[r][t], sI[t][c], acc);
      sI[r][c] = -acc / sS[r][r];
    }
  }
  __syncthreads();
  if (tid < K) {
    double acc = 0.0;
    for (int j = 0; j <= tid; ++j) acc = fma(sI[tid][j], sres[j], acc);
    sb2[tid] = acc;
  }
  __syncthreads();
  if (tid < K) {
    double acc = 0.0;
    for (int j = tid; j < K; ++j) acc = fma(sI[j][tid], sb2[j], acc);
    sg[tid] = acc;
  }
  __syncthreads();
  for (int e = tid; e < ROWS_CH_DOUBLES; e += blockDim.x) {
    double v;
    if (e < ROWS_MAX * ROWS_MAX) {
      const int r = e / ROWS_MAX, c = e % ROWS_MAX;
      v = (r < K && c <= r) ? sI[r][c] : 0.0;
    } else {
      const int k = (e - ROWS_MAX * ROWS_MAX) % ROWS_MAX;
      v = (k >= K) ? 0.0 : (e < ROWS_MAX * ROWS_MAX + ROWS_MAX) ? sb2[k] : sg[k];
    }
    a.ch[e] = v;
  }
  for (int e = tid; e < K * n1; e += blockDim.x) {  // the K new rows of L', and the right block of M's
    const int k = e / n1, c = e - k * n1;
    const size_t at = (size_t)(n + k) * n1 + c;
    if (c < n) {
      a.Ln[at] = bx[(size_t)k * np + c];
    } else {
      const int j = c - n;
      a.Ln[at] = (j <= k) ? sS[k][j] : 0.0;
      a.Mn[at] = (j <= k) ? sI[k][j] : 0.0;
    }
  }
  if (tid == 0) info[blockIdx.x] = 0;
}

// Column q of the new state per lane: W[k][q] from the chunks in chunk order, M'[n + k][q] = -(C^{-1} W)[k][q],
// alpha'[q] = (M^T beta)[q] - sum_k W[k][q] gamma[k]; alpha'[n + k] = gamma[k]; zero up to n_pad(n + K).
__global__ __launch_bounds__(64) void rows_finish_kernel(const RowsJob* __restrict__ jobs,
                                                         const int* __restrict__ info) {
  const RowsJob& a = jobs[blockIdx.y];
  if (info[blockIdx.y] != 0) return;
  const int n = a.o.n, K = a.K, np = pad16(n), n1 = n + K;
  const int q = 64 * blockIdx.x + threadIdx.x;
  if (q >= pad16(n1)) return;
  const double* __restrict__ ch = a.ch;
  if (q >= n) {
    a.alpha[q] = (q < n1) ? ch[ROWS_MAX * ROWS_MAX + ROWS_MAX + (q - n)] : 0.0;
    return;
  }
  const double* __restrict__ wp = a.wp;
  const int nrc = (n + ROWS_CHUNK - 1) / ROWS_CHUNK;
  double w[ROWS_MAX + 1];
#pragma unroll
  for (int k = 0; k <= ROWS_MAX; ++k) w[k] = 0.0;
  for (int rc = 0; rc < nrc; ++rc) {
#pragma unroll
    for (int k = 0; k <= ROWS_MAX; ++k)
      if (k <= K) w[k] += wp[((size_t)rc * (K + 1) + k) * np + q];
  }
  double wg = 0.0, mtb = 0.0;
#pragma unroll
  for (int k = 0; k <= ROWS_MAX; ++k)
    if (k == K) mtb = w[k];
#pragma unroll
  for (int k = 0; k < ROWS_MAX; ++k) {
    if (k < K) {
      double acc = 0.0;
#pragma unroll
      for (int j = 0; j <= k; ++j) acc = fma(ch[k * ROWS_MAX + j], w[j], acc);
      a.Mn[(size_t)(n + k) * n1 + q] = -acc;
      wg = fma(w[k], ch[ROWS_MAX * ROWS_MAX + ROWS_MAX + k], wg);
    }
  }
  a.alpha[q] = mtb - wg;
}

// root_frag' from M' (pack_linv_kernel's map, one job per blockIdx.y).
__global__ __launch_bounds__(256) void rows_pack_kernel(const RowsJob* __restrict__ jobs,
                                                        const int* __restrict__ info) {
  const RowsJob& a = jobs[blockIdx.y];
  if (info[blockIdx.y] != 0) return;
  const int n1 = a.o.n + a.K, np = pad16(n1), KB = np / 4;
  const size_t total = (size_t)np * np;
  const double* __restrict__ X = a.Mn;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const int l = (int)(e & 63);
    const size_t blk = e >> 6;
    const int kb = (int)(blk % KB);
    const int tj = (int)(blk / KB);
    const int row = 16 * tj + (l & 15);
    const int col = 4 * kb + (l >> 4);
    a.rf[frag_index(tj, kb, l, KB)] = (row < n1 && col < n1) ? X[(size_t)row * n1 + col] : 0.0;
  }
}

// One 16-row tile of D per workgroup of four waves, as append_disc_kernel: wave w streams the old tile's pairs
// j = w (mod 4) (lane l of pair j: row l & 15, columns 8 j + (l >> 4) and 8 j + 4 + (l >> 4)) into its K + 1 dots
// with bx (the rows of B, then beta) and stores the pairs that hold old columns only at the same place of the new
// tile.  The four column groups meet by shuffles, the four waves in LDS, both in a fixed order.  Then
// T = kd - Q_D B^T, the new columns T C^{-T}, the mean, and the pairs from column n on: old columns, new columns,
// zeros.  Rows past N stay exactly zero.
__global__ __launch_bounds__(256) void rows_disc_kernel(const RowsJob* __restrict__ jobs,
                                                        const int* __restrict__ info) {
  __shared__ double part[ROWS_MAX + 1][4][16];
  __shared__ double sT[16][ROWS_MAX + 1], sNew[16][ROWS_MAX + 1];
  __shared__ double sch[ROWS_CH_DOUBLES];
  const RowsJob& a = jobs[blockIdx.y];
  const int N = a.N, t = blockIdx.x;
  if (N == 0 || 16 * t >= pad16(N) || info[blockIdx.y] != 0) return;
  const int n = a.o.n, K = a.K, n1 = n + K, npo = pad16(n), npn = pad16(n1), Np = pad16(N);
  const int po = npo >> 3, pn = npn >> 3;  // pairs per tile, old and new
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, lr = lane & 15;
  for (int e = tid; e < ROWS_CH_DOUBLES; e += blockDim.x) sch[e] = a.ch[e];
  const double* __restrict__ bx = a.bx;
  const double2* __restrict__ src = reinterpret_cast<const double2*>(a.o.disc_frag) + (size_t)t * po * 64 + lane;
  double2* __restrict__ dst = reinterpret_cast<double2*>(a.qn) + (size_t)t * pn * 64 + lane;
  const int jn = n >> 3;  // the first pair that holds a new column
  double acc[ROWS_MAX + 1];
#pragma unroll
  for (int k = 0; k <= ROWS_MAX; ++k) acc[k] = 0.0;
  for (int j = wave; j < po; j += 4) {
    const double2 v = src[(size_t)j * 64];
    const int c0 = 8 * j + g;
#pragma unroll
    for (int k = 0; k <= ROWS_MAX; ++k) {
      if (k <= K) {
        acc[k] = fma(v.x, bx[(size_t)k * npo + c0], acc[k]);
        acc[k] = fma(v.y, bx[(size_t)k * npo + c0 + 4], acc[k]);
      }
    }
    if (j < jn) dst[(size_t)j * 64] = v;
  }
#pragma unroll
  for (int k = 0; k <= ROWS_MAX; ++k) {
    if (k <= K) {
      double s = acc[k];
      s += __shfl_xor(s, 16);
      s += __shfl_xor(s, 32);
      if (lane < 16) part[k][wave][lane] = s;
    }
  }
  __syncthreads();
  for (int e = tid; e < 16 * (K + 1); e += blockDim.x) {
    const int row = e & 15, k = e >> 4;
    const double dot = ((part[k][0][row] + part[k][1][row]) + part[k][2][row]) + part[k][3][row];
    sT[row][k] = (k < K) ? a.kd[(size_t)k * Np + 16 * t + row] - dot : dot;  // kd is zero past N; k = K: Q_D beta
  }
  __syncthreads();
  for (int e = tid; e < 16 * K; e += blockDim.x) {
    const int row = e & 15, k = e >> 4;
    double s = 0.0;
    for (int j = 0; j <= k; ++j) s = fma(sT[row][j], sch[k * ROWS_MAX + j], s);
    sNew[row][k] = s;
  }
  __syncthreads();
  if (tid < 16) {
    double mu = sT[tid][K];
    for (int k = 0; k < K; ++k) mu = fma(sNew[tid][k], sch[ROWS_MAX * ROWS_MAX + k], mu);
    a.mean[16 * t + tid] = (16 * t + tid < N) ? a.o.mean_constant + mu : 0.0;
  }
  for (int j = jn + wave; j < pn; j += 4) {
    double2 v = make_double2(0.0, 0.0);
    if (j < po) v = src[(size_t)j * 64];
    const int c0 = 8 * j + g, c1 = c0 + 4;
    if (c0 >= n) v.x = (c0 < n1) ? sNew[lr][c0 - n] : 0.0;
    if (c1 >= n) v.y = (c1 < n1) ? sNew[lr][c1 - n] : 0.0;
    dst[(size_t)j * 64] = v;
  }
}

hipError_t launch_append_rows(const RowsJob* jobs, int J, int d, int nmax, int Kmax, int Nmax, int* info,
                              hipStream_t s) {
  const size_t total = (size_t)nmax * (nmax + Kmax);
  const int cblocks = (int)std::min<size_t>((total + 255) / 256, 1024);
  const int np1 = pad16(nmax + Kmax);
  const int pblocks = (int)std::min<size_t>(((size_t)np1 * np1 + 255) / 256, 1024);
  hipLaunchKernelGGL(rows_copy_kernel, dim3(cblocks, J), dim3(256), 0, s, jobs);
  hipLaunchKernelGGL(rows_kx_kernel, dim3(Kmax + 1, J), dim3(256), 0, s, jobs, d);
  hipLaunchKernelGGL(rows_b_kernel, dim3(pad16(nmax) / 4, J), dim3(256), 0, s, jobs);
  hipLaunchKernelGGL(rows_w_kernel, dim3((pad16(nmax) + 63) / 64, (nmax + ROWS_CHUNK - 1) / ROWS_CHUNK, J), dim3(256),
                     0, s, jobs);
  hipLaunchKernelGGL(rows_chol_kernel, dim3(J), dim3(1024), 0, s, jobs, d, info);
  hipLaunchKernelGGL(rows_finish_kernel, dim3((np1 + 63) / 64, J), dim3(64), 0, s, jobs, info);
  hipLaunchKernelGGL(rows_pack_kernel, dim3(pblocks, J), dim3(256), 0, s, jobs, info);
  if (Nmax > 0) hipLaunchKernelGGL(rows_disc_kernel, dim3(pad16(Nmax) / 16, J), dim3(256), 0, s, jobs, info);
  return hipGetLastError();
}

}  // namespace dkg
