// Sample paths for joint entropy search on the device (gfx950): random-Fourier-feature posterior paths and their
// evaluation.  The reference draws the paths with BoTorch's get_gp_samples (modules/pareto/jes_sample_pareto.py:81-86);
// the NSGA-II that runs on them and the pruning of its fronts are dkg_pareto.hip's, which takes launch_rff_eval as its
// fitness.  Specification: include/dkg.h; DESIGN.md 8e.
//
//   rff_feature_kernel   omega, bias and Phi [n][R] of up to 8 (sample, output) problems: lane = feature, wave = row
//   rff_gram_kernel      A = Phi^T Phi + diag I in 32 x 32 tiles of v_mfma_f64_16x16x4_f64, k in order
//   rff_gram_valu_kernel the same contraction in 16 x 16 VALU tiles (dkg_debug_rff_gram; the A/B of DESIGN.md 8e)
//   launch_cholesky_batch / launch_tri_inverse_batch (dkg_linalg.hip): L = chol(A), X = L^{-1}
//   rff_theta_kernel     theta = X^T (X Phi^T r + sqrt(noise) z), coef and offset; one workgroup per problem
//   rff_eval_kernel      F[s][p][i]: one workgroup per (sample, output, 16 points), (omega, bias, coef) in LDS, one
//                        wave per point, lane l the features l, l + 64, ... as one fma chain, then wave_sum; the
//                        points as given or mapped to the unit cube with lb / ub (launch_rff_eval, dkg_kernels.h)
// fp64 throughout; every sum runs in a fixed order; no atomics on floating-point values.
#include <algorithm>
#include <atomic>
#include <cmath>

#include "dkg_acq.h"

namespace dkg {

constexpr int RFF_NB = 8;          // problems per batch of the factorisation (PrepBatch holds DKG_MAX_OUTPUTS)
constexpr int RFF_MAXR = DKG_RFF_MAX_FEATURES;
static_assert(RFF_NB <= DKG_MAX_OUTPUTS, "a PrepBatch carries the batch");
static_assert(DKG_RFF_EVAL_LDS_BYTES(DKG_RFF_MAX_FEATURES, DKG_MAX_DIM) <= 160 * 1024,
              "the widest path's (omega, bias, coef) fit in one workgroup's LDS");

struct RffBatch {
  dkg_output o[RFF_NB];        // n, kernel, outputscale, noise, mean_constant, y_mean, y_std, inv_lengthscale, train_x
  const double* y[RFF_NB];     // targets [n], model space
  const double *wn[RFF_NB], *g[RFF_NB], *ub[RFF_NB], *z[RFF_NB];
  double *omega[RFF_NB], *bias[RFF_NB], *coef[RFF_NB], *offset[RFF_NB];
  double* Phi[RFF_NB];         // [n][R]
  double* A[RFF_NB];           // [R][R]
  const double* X[RFF_NB];     // [R][R], L^{-1}
  const int* info[RFF_NB];
  double diag[RFF_NB];         // noise + jitter
  int d, R;
};

// Grid (R / 64, n / 16, problems); lane = feature, the workgroup's 4 waves share 16 training rows.
__global__ __launch_bounds__(256) void rff_feature_kernel(RffBatch b) {
  const int q = blockIdx.z;
  const dkg_output& o = b.o[q];
  const int n = o.n, d = b.d, R = b.R;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = blockIdx.x * WAVE + lane;
  if (r >= R) return;
  const double gs = o.kernel == DKG_RBF ? 1.0 : 1.0 / sqrt(b.g[q][r]);
  double w[DKG_MAX_DIM];
#pragma unroll
  for (int j = 0; j < DKG_MAX_DIM; ++j) {
    const int jj = min(j, d - 1);
    w[j] = b.wn[q][(size_t)r * d + jj] * o.inv_lengthscale[jj] * gs;
  }
  const double bias = 6.283185307179586476925 * b.ub[q][r];
  if (blockIdx.y == 0 && wave == 0) {
#pragma unroll
    for (int j = 0; j < DKG_MAX_DIM; ++j)
      if (j < d) b.omega[q][(size_t)r * d + j] = w[j];
    b.bias[q][r] = bias;
  }
  const double amp = sqrt(2.0 * o.outputscale / R);
  for (int kk = wave; kk < 16; kk += 4) {
    const int k = blockIdx.y * 16 + kk;
    if (k >= n) break;
    double ph = 0.0;
#pragma unroll
    for (int j = 0; j < DKG_MAX_DIM; ++j)
      if (j < d) ph = fma(w[j], o.train_x[(size_t)k * d + j], ph);
    b.Phi[q][(size_t)k * R + r] = amp * cos(ph + bias);
  }
}

// A = Phi^T Phi + diag I.  Grid (T^2, problems), T = R / 32 rounded up; wave w the 16 x 16 sub-tile (w & 1, w >> 1);
// the training rows in order, four per MFMA.  A[i][j] and A[j][i] are the same products in the same order.
__global__ __launch_bounds__(256) void rff_gram_kernel(RffBatch b) {
  const int q = blockIdx.y;
  const int n = b.o[q].n, R = b.R;
  const int T = (R + 31) / 32;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i0 = (blockIdx.x / T) * 32 + 16 * (wave & 1), j0 = (blockIdx.x % T) * 32 + 16 * (wave >> 1);
  if (i0 >= R || j0 >= R) return;  // wave-uniform
  const double* __restrict__ Phi = b.Phi[q];
  const int ci = i0 + (lane & 15), cj = j0 + (lane & 15);
  d4 acc = {0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < n; k0 += 4) {
    const int k = k0 + (lane >> 4);
    const double av = (k < n && ci < R) ? Phi[(size_t)k * R + ci] : 0.0;
    const double bv = (k < n && cj < R) ? Phi[(size_t)k * R + cj] : 0.0;
    acc = mfma_f64(av, bv, acc);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = i0 + (lane >> 4) + 4 * r;
    if (row < R && cj < R) b.A[q][(size_t)row * R + cj] = acc[r] + (row == cj ? b.diag[q] : 0.0);
  }
}

// The same matrix by VALU fma chains: grid (T16^2, problems), one thread per entry of a 16 x 16 tile, the two
// column strips of Phi staged in LDS 16 rows at a time.
__global__ __launch_bounds__(256) void rff_gram_valu_kernel(RffBatch b) {
  __shared__ double sa[16][17], sb[16][17];
  const int q = blockIdx.y;
  const int n = b.o[q].n, R = b.R;
  const int T = (R + 15) / 16;
  const int i0 = (blockIdx.x / T) * 16, j0 = (blockIdx.x % T) * 16;
  const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
  const double* __restrict__ Phi = b.Phi[q];
  double acc = 0.0;
  for (int k0 = 0; k0 < n; k0 += 16) {
    const int k = k0 + ty;
    sa[ty][tx] = (k < n && i0 + tx < R) ? Phi[(size_t)k * R + i0 + tx] : 0.0;
    sb[ty][tx] = (k < n && j0 + tx < R) ? Phi[(size_t)k * R + j0 + tx] : 0.0;
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) acc = fma(sa[kk][ty], sb[kk][tx], acc);
    __syncthreads();
  }
  const int row = i0 + ty, col = j0 + tx;
  if (row < R && col < R) b.A[q][(size_t)row * R + col] = acc + (row == col ? b.diag[q] : 0.0);
}

// theta = A^{-1} Phi^T r + L^{-T} sqrt(noise) z, r = y - c, with X = L^{-1} (zero above the diagonal): the first
// term as X^T X u refined once against L L^T; then coef = y_std amp theta and offset = y_mean + y_std c.  One
// workgroup per problem; the triangular products as alpha_kernel runs them: a row per wave with lane partial sums
// in column order and a fixed-order wave reduction; columns by groups of 64 with the 16 wave partials met in wave
// order.
__global__ __launch_bounds__(1024) void rff_theta_kernel(RffBatch b) {
  __shared__ double u[RFF_MAXR];
  __shared__ double t[RFF_MAXR];
  __shared__ double th[RFF_MAXR];
  __shared__ double w[RFF_MAXR];
  __shared__ double part[16][64];
  const int q = blockIdx.x;
  if (*b.info[q] != 0) return;
  const dkg_output& o = b.o[q];
  const int n = o.n, R = b.R;
  const double* __restrict__ Phi = b.Phi[q];
  const double* __restrict__ X = b.X[q];
  const double c = o.mean_constant;
  for (int r = threadIdx.x; r < R; r += blockDim.x) {
    double s = 0.0;
    for (int k = 0; k < n; ++k) s = fma(Phi[(size_t)k * R + r], b.y[q][k] - c, s);
    u[r] = s;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  // out = M in for a lower-triangular M (only k <= i is read): a row per wave
  auto rows = [&](const double* __restrict__ M, const double* in, double* out) {
    for (int i = wave; i < R; i += nw) {
      double s = 0.0;
      for (int k = lane; k <= i; k += 64) s = fma(M[(size_t)i * R + k], in[k], s);
      s = wave_sum(s);
      if (lane == 0) out[i] = s;
    }
    __syncthreads();
  };
  // out = M^T in: columns by groups of 64, wave w the rows i = w (mod 16) of its lane's column
  auto cols = [&](const double* __restrict__ M, const double* in, double* out) {
    for (int g0 = 0; g0 < R; g0 += 64) {
      const int k = g0 + lane;
      double s = 0.0;
      if (k < R) {
        const int i1 = k + ((wave - k) % nw + nw) % nw;  // first row >= k with i = wave (mod nw)
        for (int i = i1; i < R; i += nw) s = fma(M[(size_t)i * R + k], in[i], s);
      }
      part[wave][lane] = s;
      __syncthreads();
      if (wave == 0 && k < R) {
        double a = 0.0;
        for (int w2 = 0; w2 < nw; ++w2) a += part[w2][lane];
        out[k] = a;
      }
      __syncthreads();
    }
  };
  const double* __restrict__ L = b.A[q];
  // th = A^{-1} u through the explicit inverse, then one step of iterative refinement against L L^T: a product with
  // L^{-1} is not backward stable, and at noise 1e-4 s the first solve alone is a few times the floor
  rows(X, u, t);
  cols(X, t, th);
  cols(L, th, t);   // L^T th
  rows(L, t, w);    // L (L^T th)
  for (int r = threadIdx.x; r < R; r += blockDim.x) w[r] = u[r] - w[r];
  __syncthreads();
  rows(X, w, t);
  cols(X, t, w);    // the correction
  // L^{-T} sqrt(noise) z
  const double sn = sqrt(o.noise);
  for (int r = threadIdx.x; r < R; r += blockDim.x) t[r] = sn * b.z[q][r];
  __syncthreads();
  cols(X, t, u);
  const double scale = o.y_std * sqrt(2.0 * o.outputscale / R);
  for (int r = threadIdx.x; r < R; r += blockDim.x) b.coef[q][r] = scale * ((th[r] + w[r]) + u[r]);
  if (threadIdx.x == 0) *b.offset[q] = fma(o.y_std, c, o.y_mean);
}

// ---------------------------------------------------------------------------------------------------------------
constexpr int RE_WAVES = 4;    // waves per workgroup of rff_eval_kernel
constexpr int RE_POINTS = 16;  // points per workgroup (4 per wave, one after the other)

struct EvalArgs {
  dkg_rff_paths p;
  const double* x;       // sample s's points at x + s * x_stride, [P][d]
  size_t x_stride;       // 0: every sample evaluates the same points
  double* F;             // sample s's values at F + s * f_stride, [P][m]
  size_t f_stride;
  const double *lb, *ub; // not NULL: the model input is (x - lb) / (ub - lb)
  int P;
};

// Grid (P / 16, m, S).  LDS (DKG_RFF_EVAL_LDS_BYTES): omega transposed [d][R] (a lane's reads are then a stride of
// one double), bias [R], coef [R].  A point's value is its own lane chains and wave_sum: the same bits whatever P,
// its row, and the samples beside it.
template <int DM>
__global__ __launch_bounds__(RE_WAVES* WAVE) void rff_eval_kernel(EvalArgs a) {
  extern __shared__ __attribute__((aligned(16))) double re_smem[];
  const int s = blockIdx.z, i = blockIdx.y;
  const int R = a.p.R, d = a.p.d, m = a.p.m;
  const size_t so = (size_t)s * m + i;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double* wT = re_smem;                // [d][R]
  double* bs = re_smem + (size_t)d * R;  // [R]
  double* cs = bs + R;                 // [R]
  const double* __restrict__ om = a.p.omega + so * R * d;
  for (int e = tid; e < R * d; e += RE_WAVES * WAVE) wT[(size_t)(e % d) * R + e / d] = om[e];
  for (int e = tid; e < R; e += RE_WAVES * WAVE) {
    bs[e] = a.p.bias[so * R + e];
    cs[e] = a.p.coef[so * R + e];
  }
  __syncthreads();
  const double off = a.p.offset[so];
  const int iters = (R + WAVE - 1) / WAVE;  // wave-uniform trip count
  const double* __restrict__ xb = a.x + (size_t)s * a.x_stride;
  double* __restrict__ Fb = a.F + (size_t)s * a.f_stride;
  const int p0 = blockIdx.x * RE_POINTS;
  for (int qq = wave; qq < RE_POINTS; qq += RE_WAVES) {
    const int p = p0 + qq;
    if (p >= a.P) break;  // wave-uniform
    double xr[DM];
#pragma unroll
    for (int k = 0; k < DM; ++k) {
      const int kk = min(k, d - 1);
      const double xv = xb[(size_t)p * d + kk];
      xr[k] = a.lb ? unit_cube(xv, a.lb[kk], a.ub[kk]) : xv;
    }
    double acc = 0.0;
    for (int it = 0; it < iters; ++it) {
      const int r = lane + it * WAVE;
      const int rc = min(r, R - 1);
      double ph = 0.0;
#pragma unroll
      for (int k = 0; k < DM; ++k)
        if (k < d) ph = fma(wT[(size_t)k * R + rc], xr[k], ph);
      acc = fma((r < R) ? cos(ph + bs[rc]) : 0.0, cs[rc], acc);
    }
    const double sum = wave_sum(acc);
    if (lane == 0) Fb[(size_t)p * m + i] = off + sum;
  }
}

hipError_t launch_rff_eval(const dkg_rff_paths& p, const double* x, size_t x_stride, double* F, size_t f_stride,
                           const double* lb, const double* ub, int P, hipStream_t s) {
  const EvalArgs a{p, x, x_stride, F, f_stride, lb, ub, P};
  const size_t lds = DKG_RFF_EVAL_LDS_BYTES(a.p.R, a.p.d);
  const dim3 grid((a.P + RE_POINTS - 1) / RE_POINTS, a.p.m, a.p.S), block(RE_WAVES * WAVE);
  by_dim(a.p.d, [&](auto dm) { launch_lds(rff_eval_kernel<decltype(dm)::value>, grid, block, lds, s, a); });
  return hipGetLastError();
}

int check_rff_paths(const dkg_rff_paths* p) {
  if (!p) return failf(DKG_ERR_ARG, "NULL pointer");
  if (p->S < 1 || p->m < 1 || p->d < 1 || p->R < 1)
    return failf(DKG_ERR_ARG, "paths S=%d m=%d d=%d R=%d", p->S, p->m, p->d, p->R);
  if (p->S > DKG_JES_MAX_SAMPLES)
    return failf(DKG_ERR_UNSUPPORTED, "S=%d samples (supported <= %d)", p->S, DKG_JES_MAX_SAMPLES);
  const int st = check_dims(p->m, p->d);
  if (st) return st;
  if (p->R > RFF_MAXR) return failf(DKG_ERR_UNSUPPORTED, "R=%d features (supported <= %d)", p->R, RFF_MAXR);
  if (!p->omega || !p->bias || !p->coef || !p->offset) return failf(DKG_ERR_ARG, "paths: NULL pointer");
  return DKG_OK;
}

}  // namespace dkg

using namespace dkg;

namespace {

std::atomic<int> g_rff_gram_valu{0};

// dkg_rff_weights' workspace: the batch's factorisation flags, then per slot A, X and Phi
struct RffWs {
  size_t info, a, x, phi, slot, total;
};
RffWs rff_ws(int R, int n_max) {
  RffWs w{};
  Carve slot;  // a, x and phi are offsets within a slot
  w.a = slot.take((size_t)R * R * sizeof(double));
  w.x = slot.take((size_t)R * R * sizeof(double));
  w.phi = slot.take((size_t)n_max * R * sizeof(double));
  w.slot = slot.total();
  w.info = 0;
  w.total = 256 + RFF_NB * w.slot;
  return w;
}

hipError_t launch_gram(const RffBatch& b, int nb, hipStream_t s) {
  if (g_rff_gram_valu.load(std::memory_order_relaxed)) {
    const int T = (b.R + 15) / 16;
    hipLaunchKernelGGL(rff_gram_valu_kernel, dim3(T * T, nb), dim3(256), 0, s, b);
  } else {
    const int T = (b.R + 31) / 32;
    hipLaunchKernelGGL(rff_gram_kernel, dim3(T * T, nb), dim3(256), 0, s, b);
  }
  return hipGetLastError();
}

}  // namespace

extern "C" {

int dkg_debug_rff_gram(int mode) {
  if (mode < -1 || mode > 1) {
    failf(DKG_ERR_ARG, "dkg_debug_rff_gram: mode=%d (0 the MFMA tiles, 1 the VALU tiles, -1 reads)", mode);
    return -2;
  }
  if (mode < 0) return g_rff_gram_valu.load(std::memory_order_relaxed);
  return g_rff_gram_valu.exchange(mode, std::memory_order_relaxed);
}

size_t dkg_rff_workspace(int R, int n_max) {
  if (R < 1 || R > RFF_MAXR || n_max < 1 || n_max > 1024) return 0;
  return rff_ws(R, n_max).total;
}

int dkg_rff_weights(const dkg_output* outs, int m, int d, const double* const* train_y, const double* wn,
                    const double* g, const double* ub, const double* z, int max_tries, const dkg_rff_paths* paths,
                    void* work, size_t work_bytes, double* jitter_used, void* stream) {
  int st = check_rff_paths(paths);
  if (st) return st;
  if (!outs || !train_y || !wn || !ub || !z || !work) return failf(DKG_ERR_ARG, "NULL pointer");
  if (m != paths->m || d != paths->d) return failf(DKG_ERR_ARG, "m=%d d=%d against paths of m=%d d=%d", m, d, paths->m, paths->d);
  if (max_tries < 0) return failf(DKG_ERR_ARG, "max_tries=%d", max_tries);
  int n_max = 1;
  bool need_g = false;
  for (int i = 0; i < m; ++i) {
    const dkg_output& o = outs[i];
    if (o.n < 1) return failf(DKG_ERR_ARG, "output %d: n=%d training points", i, o.n);
    if (o.n > 1024) return failf(DKG_ERR_UNSUPPORTED, "output %d: n=%d > 1024 training points", i, o.n);
    if (o.kernel < DKG_MATERN12 || o.kernel > DKG_RBF) return failf(DKG_ERR_ARG, "output %d: kernel id %d", i, o.kernel);
    if (!o.inv_lengthscale || !o.train_x || !train_y[i]) return failf(DKG_ERR_ARG, "output %d: NULL pointer", i);
    if (!(o.noise > 0.0) || !(o.outputscale > 0.0))
      return failf(DKG_ERR_ARG, "output %d: noise=%g outputscale=%g", i, o.noise, o.outputscale);
    n_max = std::max(n_max, (int)o.n);
    need_g = need_g || o.kernel != DKG_RBF;
  }
  if (need_g && !g) return failf(DKG_ERR_ARG, "NULL pointer (the Gamma draws of a Matern output)");
  const int S = paths->S, R = paths->R;
  const RffWs w = rff_ws(R, n_max);
  if (work_bytes < w.total) return failf(DKG_ERR_WORKSPACE, "workspace %zu bytes < required %zu", work_bytes, w.total);
  hipStream_t s = (hipStream_t)stream;
  int* d_info = at<int>(work, w.info);
  const int total = S * m;
  for (int q0 = 0; q0 < total; q0 += RFF_NB) {
    const int nb = std::min(RFF_NB, total - q0);
    RffBatch b{};
    PrepBatch pb{};
    b.d = d;
    b.R = R;
    int nbmax = 1;
    for (int j = 0; j < nb; ++j) {
      const int q = q0 + j, i = q % m;
      char* slot = at<char>(work, 256 + (size_t)j * w.slot);
      b.o[j] = outs[i];
      b.y[j] = train_y[i];
      b.wn[j] = wn + (size_t)q * R * d;
      b.g[j] = g ? g + (size_t)q * R : nullptr;
      b.ub[j] = ub + (size_t)q * R;
      b.z[j] = z + (size_t)q * R;
      b.omega[j] = paths->omega + (size_t)q * R * d;
      b.bias[j] = paths->bias + (size_t)q * R;
      b.coef[j] = paths->coef + (size_t)q * R;
      b.offset[j] = paths->offset + q;
      b.A[j] = at<double>(slot, w.a);
      b.X[j] = at<double>(slot, w.x);
      b.Phi[j] = at<double>(slot, w.phi);
      b.info[j] = d_info + j;
      b.diag[j] = outs[i].noise;
      pb.A[j] = b.A[j];
      pb.X[j] = const_cast<double*>(b.X[j]);
      pb.n[j] = R;
      pb.info[j] = d_info + j;
      nbmax = std::max(nbmax, (int)outs[i].n);
      if (jitter_used) jitter_used[q] = 0.0;
    }
    int h_info[RFF_NB];
    hipLaunchKernelGGL(rff_feature_kernel, dim3((R + WAVE - 1) / WAVE, (nbmax + 15) / 16, nb), dim3(256), 0, s, b);
    if ((st = hip_status(hipGetLastError(), "rff_feature_kernel")) ||
        (st = hip_status(hipMemsetAsync(d_info, 0, RFF_NB * sizeof(int), s), "hipMemsetAsync")) ||
        (st = hip_status(launch_gram(b, nb, s), "rff_gram_kernel")) ||
        (st = hip_status(launch_cholesky_batch(pb, nb, s), "cholesky_batch")) ||
        (st = hip_status(hipMemcpyAsync(h_info, d_info, nb * sizeof(int), hipMemcpyDeviceToHost, s), "hipMemcpyAsync")) ||
        (st = hip_status(hipStreamSynchronize(s), "hipStreamSynchronize")))
      return st;
    // dkg_prepare_outputs' policy: the problems that failed are retried one by one with absolute jitter 1e-8 * 10^i
    for (int j = 0; j < nb; ++j) {
      if (h_info[j] == 0) continue;
      RffBatch one{};
      one.d = d;
      one.R = R;
      one.o[0] = b.o[j];
      one.Phi[0] = b.Phi[j];
      one.A[0] = b.A[j];
      int hi = h_info[j];
      for (int attempt = 1; attempt <= max_tries && hi != 0; ++attempt) {
        const double jit = 1e-8 * std::pow(10.0, attempt - 1);
        one.diag[0] = b.o[j].noise + jit;
        if ((st = hip_status(launch_gram(one, 1, s), "rff_gram_kernel")) ||
            (st = hip_status(hipMemsetAsync(d_info + j, 0, sizeof(int), s), "hipMemsetAsync")) ||
            (st = hip_status(launch_cholesky(b.A[j], pb.X[j], R, d_info + j, s), "cholesky")) ||
            (st = hip_status(hipMemcpyAsync(&hi, d_info + j, sizeof(int), hipMemcpyDeviceToHost, s), "hipMemcpyAsync")) ||
            (st = hip_status(hipStreamSynchronize(s), "hipStreamSynchronize")))
          return st;
        if (hi == 0 && jitter_used) jitter_used[q0 + j] = jit;
      }
      if (hi != 0)
        return failf(DKG_ERR_NOT_PD, "sample %d output %d: Phi^T Phi + noise I not positive definite after %d jitter "
                     "retries (pivot %d)", (q0 + j) / m, (q0 + j) % m, max_tries, hi);
    }
    if ((st = hip_status(launch_tri_inverse_batch(pb, nb, s), "tri_inverse_batch"))) return st;
    hipLaunchKernelGGL(rff_theta_kernel, dim3(nb), dim3(1024), 0, s, b);
    if ((st = hip_status(hipGetLastError(), "rff_theta_kernel"))) return st;
  }
  return DKG_OK;
}

int dkg_rff_eval(const dkg_rff_paths* paths, const double* x, int P, int shared_x, double* F, void* stream) {
  int st = check_rff_paths(paths);
  if (st) return st;
  if (P < 0 || P > (1 << 24)) return failf(DKG_ERR_ARG, "P=%d points", P);
  if (P == 0) return DKG_OK;
  if (!x || !F) return failf(DKG_ERR_ARG, "NULL pointer");
  return hip_status(launch_rff_eval(*paths, x, shared_x ? 0 : (size_t)P * paths->d, F, (size_t)P * paths->m, nullptr,
                                    nullptr, P, (hipStream_t)stream),
                    "rff_eval_kernel");
}

}  // extern "C"
