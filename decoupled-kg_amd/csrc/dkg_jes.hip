// Lower-bound joint entropy search (JES-LB / LB2, Tu et al. 2022) on the device (gfx950), q = 1, with the
// reference's target_output_ix for the decoupled setting.  The reference is
// qLowerBoundMultiObjectiveJointEntropySearch (modules/acquisition/joint_entropy_search.py):
// _compute_posterior_statistics (:378-470) asks the model and every model conditioned on a sampled Pareto set
// (:365-376) for a posterior at the candidates, _compute_entropy_upper_bound (:596-732) bounds the entropy of
// the truncated predictive over the box decomposition, and autograd differentiates the lot for optimize_acqf
// (acquisition_optimisation_strategy.py:493-508, 536-549).  Here an evaluation is two launches whatever the
// number of samples P and outputs m:
//
//   jes_moments_kernel   grid (16-candidate tiles) x ((P + 1) m state-outputs).  Per workgroup the 16 x n slab
//                        of s k(x, X) is evaluated once into LDS in the B-operand order of
//                        v_mfma_f64_16x16x4_f64 and contracted against the state-output's R^T fragments
//                        (Q = K(x, X) R stays in registers: wave w owns the column tiles w, 15 - w, 16 + w, ...
//                        over their whole k range, R^T lower triangular); it leaves mu = c + K alpha and
//                        |q|^2.  With the gradient, one more slab and contraction per input coordinate g
//                        (J_g = dK/dx_g R): dmu/dx_g = dK/dx_g alpha and dvar/dx_g = -2 q . J_g.
//                        Sums: one fma chain per lane, the four lanes of a candidate by cross-lane adds, the
//                        waves through LDS in wave order.
//   jes_entropy_kernel   one workgroup per candidate, one wave per state (state 0: the initial entropy; state
//                        p + 1: the bound under sample p), lanes over the boxes in rounds of 64.  A first pass
//                        sums W_j and the W_j-weighted box moments, the wave's registers hold the m x m
//                        covariance, its Cholesky and (for the gradient) its inverse, and a second pass over the
//                        boxes carries the adjoint back to (mu_i, v_i) (reverse mode, written out by hand); the
//                        chain rule to dx ends here with the moments stage's dmu/dx and dvar/dx.  The states
//                        meet in LDS and are summed in index order.  No atomics anywhere: two calls give the
//                        same bits, and a candidate's result does not depend on B or on its row.
#include <cstdio>
#include <cstring>

#include "dkg_acq.h"
#include "dkg_stages.h"

namespace dkg {

constexpr int JM_WAVES = 8;   // waves per workgroup of the moments stage
constexpr int JM_MAXT = 8;    // column tiles of Q per wave (n_pad <= 1024: 64 tiles over 8 waves)
constexpr int JE_WAVES = 4;   // waves per workgroup of the entropy stage (one per SIMD: the M = 8 register Cholesky)
constexpr double JES_EPS = 2.220446049250313e-16;  // 2^-52, torch.finfo(double).eps: the reference's CLAMP_LB
constexpr double JES_HALF_LOG_2PIE = 1.4189385332046727;  // (1 + log 2 pi) / 2
constexpr unsigned JES_MAGIC = 0x4a455331u;

struct JesPlan {
  unsigned magic;
  int m, P, d, J, target, only_diag, max_B, bpad, SO, max_np;
  const dkg_output* tab;  // device [SO]: state s, output i at s m + i
  const double* bounds;   // device [P][2][J][m]
  double* mu;             // device [SO][bpad]: c + K(x, X) alpha (model space)
  double* q2;             // device [SO][bpad]: |K(x, X) R|^2
  double* dmu;            // device [SO][d][bpad]
  double* dvar;           // device [SO][d][bpad]: d(s - |q|^2)/dx_g
};

struct JesHost {
  JesPlan plan;
  dkg_output tab[(DKG_JES_MAX_SAMPLES + 1) * DKG_MAX_OUTPUTS];
};

struct JesMomArgs {
  const dkg_output* tab;
  const double* x;
  double *mu, *q2, *dmu, *dvar;
  int B, d, bpad, grad;
};

__host__ __device__ inline size_t jes_mom_lds_bytes(int max_np) {
  return ((size_t)(max_np / 4) * 64 + 2 * JM_WAVES * 16) * sizeof(double);
}

template <int DM>
__global__ __launch_bounds__(JM_WAVES* WAVE) void jes_moments_kernel(JesMomArgs a) {
  extern __shared__ __attribute__((aligned(16))) double jm_smem[];
  const dkg_output& o = a.tab[blockIdx.y];
  const int n = o.n, d = a.d;
  const int np = pad16(n), T = np / 16, KB = np / 4;
  double* slab = jm_smem;                  // [KB][64]: K (or dK/dx_g) of the 16 candidates, B-operand order
  double* red = jm_smem + (size_t)KB * 64; // [2][JM_WAVES][16] partial sums of the waves
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int row = blockIdx.x * 16 + (lane & 15);
  const int rowc = min(row, a.B - 1);  // rows past B repeat the last candidate and are never stored
  double xr[DM], il[DM];
  clamped_row<DM>(il, o.inv_lengthscale, d);
  scaled_point<DM>(xr, a.x + (size_t)rowc * d, il, d);
  const double os = o.outputscale;
  const double* __restrict__ tx = o.train_x;
  const double* __restrict__ alpha = o.alpha;
  const double* __restrict__ root = o.root_frag;
  const int nch = a.grad ? d + 1 : 1;  // channel 0: K; channel 1 + g: dK/dx_g
  const int iters = (KB + JM_WAVES - 1) / JM_WAVES;
  double qreg[JM_MAXT][4];  // the wave's tiles of Q (channel 0), kept for q . J_g
#pragma unroll
  for (int s = 0; s < JM_MAXT; ++s)
#pragma unroll
    for (int r = 0; r < 4; ++r) qreg[s][r] = 0.0;

  for (int ch = 0; ch < nch; ++ch) {
    const int g = max(ch - 1, 0);
    double xg = 0.0, ilg = 0.0;
#pragma unroll
    for (int k = 0; k < DM; ++k) {
      xg = (k == g) ? xr[k] : xg;
      ilg = (k == g) ? il[k] : ilg;
    }
    // ---- the slab, and the lane's share of the alpha product
    double mpart = 0.0;
    with_kind(o.kernel, [&](auto kind_c) {
      constexpr int KIND = decltype(kind_c)::value;
      const const_dptr tab = psi_tab();
      for (int it = 0; it < iters; ++it) {
        const int kb = wave + JM_WAVES * it;
        const int col = 4 * kb + (lane >> 4);
        const int cc = min(col, n - 1);
        double xs[DM];
        scaled_point<DM>(xs, tx + (size_t)cc * d, il, d);
        double kv;
        if (ch == 0) {
          kv = cross_kernel_term<DM, KIND>(xr, xs, d, os, tab);
        } else {
          double xsg = 0.0;
#pragma unroll
          for (int k = 0; k < DM; ++k) xsg = (k == g) ? xs[k] : xsg;
          kv = os * kernel_dprofile_t<KIND>(sq_dist<DM>(xr, xs, d)) * (xg - xsg) * ilg;
        }
        const double v = (col < n) ? kv : 0.0;
        mpart = fma(v, alpha[cc], mpart);
        if (kb < KB) slab[kb * 64 + lane] = v;
      }
    });
    __syncthreads();

    // ---- D = R^T K^T per column tile: lane l, register r holds Q[l & 15][16 tj + (l >> 4) + 4 r]
    double qpart = 0.0;
#pragma unroll
    for (int s = 0; s < JM_MAXT; ++s) {
      const int tj = JM_WAVES * s + ((s & 1) ? JM_WAVES - 1 - wave : wave);
      if (tj < T) {  // wave-uniform
        d4 acc0 = {0, 0, 0, 0}, acc1 = {0, 0, 0, 0};
        const int nj = 2 * (tj + 1);  // 16-byte words of k-blocks 2 j, 2 j + 1 < 4 (tj + 1)
#pragma unroll 4
        for (int j = 0; j < nj; ++j) {
          const double2 rt = frag_pair(root, tj, j, lane, KB);
          acc0 = mfma_f64(rt.x, slab[(2 * j) * 64 + lane], acc0);
          acc1 = mfma_f64(rt.y, slab[(2 * j + 1) * 64 + lane], acc1);
        }
        const d4 acc = acc0 + acc1;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (ch == 0) qreg[s][r] = acc[r];
          qpart = fma(acc[r], qreg[s][r], qpart);
        }
      }
    }
    // lanes l, l ^ 16, l ^ 32, l ^ 48 share a candidate
    mpart += partner_f64<4>(mpart);
    mpart += partner_f64<5>(mpart);
    qpart += partner_f64<4>(qpart);
    qpart += partner_f64<5>(qpart);
    if (lane < 16) {
      red[wave * 16 + lane] = mpart;
      red[(JM_WAVES + wave) * 16 + lane] = qpart;
    }
    __syncthreads();  // also: every wave is done with the slab before the next channel's fill
    if (tid < 16) {
      double sm = 0.0, sq = 0.0;
#pragma unroll
      for (int w = 0; w < JM_WAVES; ++w) {
        sm += red[w * 16 + tid];
        sq += red[(JM_WAVES + w) * 16 + tid];
      }
      const int rr = blockIdx.x * 16 + tid;
      if (rr < a.B) {
        const size_t so = blockIdx.y;
        if (ch == 0) {
          a.mu[so * a.bpad + rr] = o.mean_constant + sm;
          a.q2[so * a.bpad + rr] = sq;
        } else {
          a.dmu[(so * d + g) * a.bpad + rr] = sm;
          a.dvar[(so * d + g) * a.bpad + rr] = -2.0 * sq;
        }
      }
    }
  }
}

struct JesEntArgs {
  const dkg_output* tab;
  const double* bounds;
  const double *mu, *q2, *dmu, *dvar;
  double *acq, *dacq, *mom;
  int m, P, d, J, target, only_diag, B, bpad, grad;
};

__device__ __forceinline__ double jes_pdf(double g) { return 0.3989422804014327 * exp(-0.5 * g * g); }
// torch's Normal.cdf, in that form: the clamp of a box probability at eps is part of the reference's function
__device__ __forceinline__ double jes_cdf(double g) { return 0.5 * (1.0 + erf(g * 0.7071067811865476)); }
// index of the pair i < k among the M (M - 1) / 2 strictly upper entries
__host__ __device__ constexpr int jes_pair(int M, int i, int k) { return i * M - i * (i + 1) / 2 + (k - i - 1); }

template <int M>
__global__ __launch_bounds__(JE_WAVES* WAVE) void jes_entropy_kernel(JesEntArgs a) {
  extern __shared__ __attribute__((aligned(16))) double je_res[];  // [P + 1][1 + d]: H and dH/dx of every state
  constexpr int NT = M > 1 ? M * (M - 1) / 2 : 1;
  const int b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m = a.m, d = a.d, J = a.J, tg = a.target;
  const int SO = (a.P + 1) * m, stride = 1 + d;
  const bool full = !a.only_diag && tg < 0;  // LB over all outputs: the m x m covariance

  for (int s = wave; s <= a.P; s += JE_WAVES) {
    // ---- the moments of the state's outputs at the candidate (untransformed space), wave-uniform
    double mu[M], v[M], tau[M], sd[M], isd[M], ys[M], dv_du[M], dtau_du[M];
#pragma unroll
    for (int i = 0; i < M; ++i) {
      mu[i] = 0.0; v[i] = 1.0; tau[i] = 0.0; sd[i] = 1.0; isd[i] = 1.0; ys[i] = 1.0; dv_du[i] = 0.0; dtau_du[i] = 0.0;
      if (i < m) {
        const dkg_output& o = a.tab[s * m + i];
        const size_t at = (size_t)(s * m + i) * a.bpad + b;
        const double y = o.y_std, y2 = y * y;
        const double var = o.outputscale - a.q2[at];
        const double u = y2 * var, un = y2 * (var + o.noise);
        ys[i] = y;
        mu[i] = fma(y, a.mu[at], o.y_mean);
        if (s == 0) {
          v[i] = un;  // var0 + noise: the argument of the initial entropy
        } else {
          // clamp_min's derivative: 1 where the argument is >= the bound
          const double vc = fmax(u, JES_EPS), an = fmax(un, JES_EPS), t0 = an - vc;
          v[i] = vc;
          tau[i] = fmax(t0, JES_EPS);
          dv_du[i] = (u >= JES_EPS) ? 1.0 : 0.0;
          dtau_du[i] = (t0 >= JES_EPS) ? ((un >= JES_EPS) ? 1.0 : 0.0) - dv_du[i] : 0.0;
          sd[i] = sqrt(vc);
          isd[i] = 1.0 / sd[i];
        }
        if (a.mom != nullptr && lane == 0) {
          a.mom[((size_t)0 * SO + s * m + i) * a.B + b] = mu[i];
          a.mom[((size_t)1 * SO + s * m + i) * a.B + b] = v[i];
          a.mom[((size_t)2 * SO + s * m + i) * a.B + b] = tau[i];
        }
      }
    }
    double H = 0.0;
    double bmm[M], bvr[M];  // dH/d(model-space mean), dH/d(model-space variance s - |q|^2)
#pragma unroll
    for (int i = 0; i < M; ++i) bmm[i] = bvr[i] = 0.0;

    if (s == 0) {
#pragma unroll
      for (int i = 0; i < M; ++i)
        if (i < m && (tg < 0 || i == tg)) {
          H += JES_HALF_LOG_2PIE + 0.5 * log(v[i]);
          bvr[i] = 0.5 * ys[i] * ys[i] / v[i];
        }
    } else {
      const int p = s - 1;
      const double* __restrict__ lo_p = a.bounds + ((size_t)p * 2 + 0) * J * m;
      const double* __restrict__ hi_p = a.bounds + ((size_t)p * 2 + 1) * J * m;
      // the box quantities of one lane: W_ji (clamped), C_ji = G_ji / W_ji, V_ji / W_ji, W_j, the clamp flags
      auto box = [&](int j0, double (&Wji)[M], double (&C)[M], double (&VW)[M], unsigned& flags) {
        const int j = j0 + lane;
        const int jc = min(j, J - 1);
        double L = 0.0;
        flags = 0;
#pragma unroll
        for (int i = 0; i < M; ++i) {
          Wji[i] = 1.0; C[i] = 0.0; VW[i] = 0.0;
          if (i < m) {
            const double gl = (lo_p[(size_t)jc * m + i] - mu[i]) * isd[i];
            const double gu = (hi_p[(size_t)jc * m + i] - mu[i]) * isd[i];
            const double pl = jes_pdf(gl), pu = jes_pdf(gu);
            const double raw = jes_cdf(gu) - jes_cdf(gl);
            flags |= (raw >= JES_EPS) ? (1u << i) : 0u;
            const double w = fmax(raw, JES_EPS);
            Wji[i] = w;
            C[i] = (pu - pl) / w;
            VW[i] = (gu * pu - gl * pl) / w;
            L += log(w);
          }
        }
        return (j < J) ? exp(L) : 0.0;
      };

      // ---- pass 1: W = sum_j W_j and the W_j-weighted sums of C_ji, V_ji / W_ji and (LB) C_ji C_jk
      double aW = 0.0, aA[M], aN[M], aT[NT];
#pragma unroll
      for (int i = 0; i < M; ++i) aA[i] = aN[i] = 0.0;
#pragma unroll
      for (int q = 0; q < NT; ++q) aT[q] = 0.0;
      for (int j0 = 0; j0 < J; j0 += WAVE) {
        double Wji[M], C[M], VW[M];
        unsigned flags;
        const double Wj = box(j0, Wji, C, VW, flags);
        aW += Wj;
#pragma unroll
        for (int i = 0; i < M; ++i) {
          aA[i] = fma(Wj, C[i], aA[i]);
          aN[i] = fma(Wj, VW[i], aN[i]);
        }
        if (full) {
#pragma unroll
          for (int i = 0; i < M; ++i)
#pragma unroll
            for (int k = i + 1; k < M; ++k) aT[jes_pair(M, i, k)] = fma(Wj * C[i], C[k], aT[jes_pair(M, i, k)]);
        }
      }
      const double Wsum = wave_sum(aW);
      const double W = fmin(Wsum, 1.0), iW = 1.0 / W;
      double A[M], N[M], am[M], D[M], Tm[NT], S[NT];
#pragma unroll
      for (int i = 0; i < M; ++i) {
        A[i] = wave_sum(aA[i]);
        N[i] = wave_sum(aN[i]);
        am[i] = sd[i] * A[i] * iW;   // sum_j omega_j s_ji
        D[i] = v[i] * N[i] * iW;
      }
#pragma unroll
      for (int q = 0; q < NT; ++q) Tm[q] = S[q] = 0.0;
      if (full) {
#pragma unroll
        for (int i = 0; i < M; ++i)
#pragma unroll
          for (int k = i + 1; k < M; ++k) {
            const int q = jes_pair(M, i, k);
            Tm[q] = wave_sum(aT[q]);
            S[q] = sd[i] * sd[k] * Tm[q] * iW;
          }
      }
      // the diagonal of the covariance in the reference's form (joint_entropy_search.py:665-671, 707-714)
      double dvar[M];
#pragma unroll
      for (int i = 0; i < M; ++i) {
        const double mom1 = mu[i] - am[i];
        dvar[i] = v[i] + tau[i] - D[i] - 2.0 * mu[i] * am[i] + mu[i] * mu[i] - mom1 * mom1;
      }
      // ---- H and its adjoints in (a_i, D_i, S_ik, v_i + tau_i)
      double ba[M], bD[M], bvpn[M], bS[NT];
#pragma unroll
      for (int i = 0; i < M; ++i) ba[i] = bD[i] = bvpn[i] = 0.0;
#pragma unroll
      for (int q = 0; q < NT; ++q) bS[q] = 0.0;
      if (!full) {
#pragma unroll
        for (int i = 0; i < M; ++i)
          if (i < m && (tg < 0 || i == tg)) {
            // LB2 clamps the variance at eps (:671); LB with a target takes log Cov_tt as it is (:716-718)
            const double var = a.only_diag ? fmax(dvar[i], JES_EPS) : dvar[i];
            const double bv = (!a.only_diag || dvar[i] >= JES_EPS) ? 0.5 / var : 0.0;
            H += JES_HALF_LOG_2PIE + 0.5 * log(var);
            bvpn[i] = bv;
            bD[i] = -bv;
            ba[i] = -2.0 * am[i] * bv;
          }
      } else {
        // Cov + 1e-6 I (:720-723), lower triangle; outputs past m: the identity
        double Lm[M][M], Li[M][M];
#pragma unroll
        for (int i = 0; i < M; ++i)
#pragma unroll
          for (int k = 0; k <= i; ++k) {
            double c;
            if (i == k) {
              c = (i < m) ? dvar[i] + 1e-6 : 1.0;
            } else {
              const double mi = mu[i] - am[i], mk = mu[k] - am[k];
              c = mu[i] * mu[k] - (mu[i] * am[k] + mu[k] * am[i]) + S[jes_pair(M, k, i)] - mi * mk;
            }
            Lm[i][k] = c;
          }
        // register Cholesky, in place
        double logdet_half = 0.0;
#pragma unroll
        for (int j = 0; j < M; ++j) {
          double sjj = Lm[j][j];
#pragma unroll
          for (int k = 0; k < j; ++k) sjj = fma(-Lm[j][k], Lm[j][k], sjj);
          const double ljj = sqrt(sjj), inv = 1.0 / ljj;
          Lm[j][j] = ljj;
          Li[j][j] = inv;
          logdet_half += log(ljj);
#pragma unroll
          for (int i = j + 1; i < M; ++i) {
            double sij = Lm[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) sij = fma(-Lm[i][k], Lm[j][k], sij);
            Lm[i][j] = sij * inv;
          }
        }
        H = m * JES_HALF_LOG_2PIE + logdet_half;
        // L^{-1} (lower), then 1/2 (Cov + 1e-6 I)^{-1} = 1/2 L^{-T} L^{-1}: the adjoint of the covariance
#pragma unroll
        for (int j = 0; j < M; ++j)
#pragma unroll
          for (int i = j + 1; i < M; ++i) {
            double sij = 0.0;
#pragma unroll
            for (int k = j; k < i; ++k) sij = fma(Lm[i][k], Li[k][j], sij);
            Li[i][j] = -sij * Li[i][i];
          }
        double bC[M][M];
#pragma unroll
        for (int i = 0; i < M; ++i)
#pragma unroll
          for (int k = 0; k <= i; ++k) {
            double sik = 0.0;
#pragma unroll
            for (int r = i; r < M; ++r) sik = fma(Li[r][i], Li[r][k], sik);
            bC[i][k] = 0.5 * sik;
          }
#pragma unroll
        for (int i = 0; i < M; ++i) {
          if (i < m) {
            bvpn[i] = bC[i][i];
            bD[i] = -bC[i][i];
            double sa = 0.0;
#pragma unroll
            for (int k = 0; k < M; ++k) sa = fma((k <= i) ? bC[i][k] : bC[k][i], am[k], sa);
            ba[i] = -2.0 * sa;
          }
#pragma unroll
          for (int k = i + 1; k < M; ++k) bS[jes_pair(M, i, k)] = (k < m) ? bC[k][i] : 0.0;
        }
      }
      if (a.grad) {
        // ---- adjoints of the raw sums, of W and the direct terms in sd_i and v_i
        double bA[M], bN[M], bT[NT], bsd[M], bvd[M];
        double bWacc = 0.0;
#pragma unroll
        for (int i = 0; i < M; ++i) {
          bA[i] = ba[i] * sd[i] * iW;
          bN[i] = bD[i] * v[i] * iW;
          bsd[i] = ba[i] * A[i] * iW;
          bvd[i] = bD[i] * N[i] * iW + bvpn[i];
          bWacc += ba[i] * am[i] + bD[i] * D[i];
        }
#pragma unroll
        for (int q = 0; q < NT; ++q) bT[q] = 0.0;
        if (full) {
#pragma unroll
          for (int i = 0; i < M; ++i)
#pragma unroll
            for (int k = i + 1; k < M; ++k) {
              const int q = jes_pair(M, i, k);
              bT[q] = bS[q] * sd[i] * sd[k] * iW;
              bsd[i] += 2.0 * bS[q] * sd[k] * Tm[q] * iW;
              bsd[k] += 2.0 * bS[q] * sd[i] * Tm[q] * iW;
              bWacc += 2.0 * bS[q] * S[q];
            }
        }
        const double bWsum = (Wsum <= 1.0) ? -bWacc * iW : 0.0;  // clamp_max's derivative

        // ---- pass 2: the adjoint of every box back to (mu_i, sd_i)
        double pm[M], ps[M];
#pragma unroll
        for (int i = 0; i < M; ++i) pm[i] = ps[i] = 0.0;
        for (int j0 = 0; j0 < J; j0 += WAVE) {
          double Wji[M], C[M], VW[M];
          unsigned flags;
          const double Wj = box(j0, Wji, C, VW, flags);
          const int jc = min(j0 + lane, J - 1);
          double bWj = bWsum;
#pragma unroll
          for (int i = 0; i < M; ++i) bWj += bA[i] * C[i] + bN[i] * VW[i];
          if (full) {
#pragma unroll
            for (int i = 0; i < M; ++i)
#pragma unroll
              for (int k = i + 1; k < M; ++k) bWj += 2.0 * bT[jes_pair(M, i, k)] * C[i] * C[k];
          }
#pragma unroll
          for (int i = 0; i < M; ++i) {
            if (i < m) {
              double tc = 0.0;
              if (full) {
#pragma unroll
                for (int k = 0; k < M; ++k)
                  if (k != i) tc += bT[k < i ? jes_pair(M, k, i) : jes_pair(M, i, k)] * C[k];
              }
              const double bCi = Wj * (bA[i] + 2.0 * tc), bVW = Wj * bN[i];
              const double iWji = 1.0 / Wji[i];
              const double bWji = ((flags >> i) & 1u) ? (bWj * Wj - bCi * C[i] - bVW * VW[i]) * iWji : 0.0;
              const double bG = bCi * iWji, bV = bVW * iWji;
              const double gl = (lo_p[(size_t)jc * m + i] - mu[i]) * isd[i];
              const double gu = (hi_p[(size_t)jc * m + i] - mu[i]) * isd[i];
              const double pl = jes_pdf(gl), pu = jes_pdf(gu);
              const double bgu = pu * (bWji - bG * gu + bV * (1.0 - gu * gu));
              const double bgl = pl * (-bWji + bG * gl - bV * (1.0 - gl * gl));
              pm[i] -= (bgu + bgl) * isd[i];
              ps[i] -= (bgu * gu + bgl * gl) * isd[i];
            }
          }
        }
#pragma unroll
        for (int i = 0; i < M; ++i)
          if (i < m) {
            const double bmu = wave_sum(pm[i]);
            const double bsdt = bsd[i] + wave_sum(ps[i]);
            const double bv = bvd[i] + bsdt * 0.5 * isd[i];
            const double bu = bv * dv_du[i] + bvpn[i] * dtau_du[i];
            bmm[i] = ys[i] * bmu;
            bvr[i] = ys[i] * ys[i] * bu;
          }
      }
    }
    // ---- this state's H and dH/dx: the chain rule through (mu, var) of its outputs, lane g the coordinate g
    if (lane == 0) je_res[s * stride] = H;
    if (a.grad) {
      double gx = 0.0;
      const int g = min(lane, d - 1);
#pragma unroll
      for (int i = 0; i < M; ++i)
        if (i < m) {
          const size_t at = ((size_t)(s * m + i) * d + g) * a.bpad + b;
          gx = fma(bmm[i], a.dmu[at], gx);
          gx = fma(bvr[i], a.dvar[at], gx);
        }
      if (lane < d) je_res[s * stride + 1 + lane] = gx;
    }
  }
  __syncthreads();
  // acq = H_0 - (1 / P) sum_p H_p, the samples in index order; thread c > 0 the gradient's coordinate c - 1
  if (tid < (a.grad ? stride : 1)) {
    double sum = 0.0;
    for (int p = 1; p <= a.P; ++p) sum += je_res[p * stride + tid];
    const double out = je_res[tid] - sum / (double)a.P;
    if (tid == 0) a.acq[b] = out;
    else a.dacq[(size_t)b * d + (tid - 1)] = out;
  }
}

}  // namespace dkg

using namespace dkg;

namespace {

// the workspace carve: the state table, then the moments and their x-gradients
struct JesWs {
  size_t tab, mu, q2, dmu, dvar, total;
};
JesWs jes_ws(int m, int P, int d, int max_B) {
  const size_t SO = (size_t)(P + 1) * m, bpad = pad16(max_B);
  JesWs w{};
  Carve c;
  w.tab = c.take(SO * sizeof(dkg_output));
  w.mu = c.take(SO * bpad * sizeof(double));
  w.q2 = c.take(SO * bpad * sizeof(double));
  w.dmu = c.take(SO * d * bpad * sizeof(double));
  w.dvar = c.take(SO * d * bpad * sizeof(double));
  w.total = c.total();
  return w;
}

// sizes only (dkg_jes_workspace and dkg_jes_init share it); 0 when they are fine
int check_sizes(int m, int P, int d, int J, int max_B) {
  if (m < 1 || P < 1 || d < 1 || J < 1 || max_B < 1)
    return failf(DKG_ERR_ARG, "m=%d P=%d d=%d J=%d max_B=%d", m, P, d, J, max_B);
  const int st = check_dims(m, d);
  if (st) return st;
  if (P > DKG_JES_MAX_SAMPLES)
    return failf(DKG_ERR_UNSUPPORTED, "P=%d Pareto samples (supported <= %d)", P, DKG_JES_MAX_SAMPLES);
  if (J > DKG_JES_MAX_BOXES) return failf(DKG_ERR_UNSUPPORTED, "J=%d boxes (supported <= %d)", J, DKG_JES_MAX_BOXES);
  if (max_B > DKG_JES_MAX_CANDIDATES)
    return failf(DKG_ERR_UNSUPPORTED, "max_B=%d candidates (supported <= %d)", max_B, DKG_JES_MAX_CANDIDATES);
  return DKG_OK;
}

}  // namespace

extern "C" {

size_t dkg_jes_plan_bytes(void) { return sizeof(JesHost); }

size_t dkg_jes_workspace(int m, int P, int d, int J, int max_B) {
  if (check_sizes(m, P, d, J, max_B) != DKG_OK) return 0;
  return jes_ws(m, P, d, max_B).total;
}

int dkg_jes_init(const dkg_output* states, int m, int P, int d, const double* bounds, int J, int target,
                 int only_diagonal, int max_B, void* workspace, size_t workspace_bytes, void* host_plan, void* stream) {
  if (!states || !bounds || !workspace || !host_plan) return failf(DKG_ERR_ARG, "NULL pointer");
  int st = check_sizes(m, P, d, J, max_B);
  if (st) return st;
  if (target < -1 || target >= m) return failf(DKG_ERR_ARG, "target=%d outside [-1, %d)", target, m);
  const int SO = (P + 1) * m;
  int max_np = 16;
  for (int k = 0; k < SO; ++k) {
    char who[48];
    std::snprintf(who, sizeof who, "state %d output %d", k / m, k % m);
    if ((st = check_output_state(states[k], true, who))) return st;
    max_np = std::max(max_np, pad16(states[k].n));
  }
  const JesWs w = jes_ws(m, P, d, max_B);
  if (workspace_bytes < w.total)
    return failf(DKG_ERR_WORKSPACE, "workspace %zu bytes < required %zu", workspace_bytes, w.total);
  JesHost* h = static_cast<JesHost*>(host_plan);
  std::memset(h, 0, sizeof(JesHost));
  std::memcpy(h->tab, states, (size_t)SO * sizeof(dkg_output));
  JesPlan& p = h->plan;
  p.m = m; p.P = P; p.d = d; p.J = J; p.target = target; p.only_diag = only_diagonal ? 1 : 0;
  p.max_B = max_B; p.bpad = pad16(max_B); p.SO = SO; p.max_np = max_np;
  p.tab = at<const dkg_output>(workspace, w.tab);
  p.bounds = bounds;
  p.mu = at<double>(workspace, w.mu);
  p.q2 = at<double>(workspace, w.q2);
  p.dmu = at<double>(workspace, w.dmu);
  p.dvar = at<double>(workspace, w.dvar);
  st = hip_status(hipMemcpyAsync(at<char>(workspace, w.tab), h->tab, (size_t)SO * sizeof(dkg_output),
                                 hipMemcpyHostToDevice, (hipStream_t)stream),
                  "dkg_jes_init: table upload");
  if (st) return st;
  p.magic = JES_MAGIC;
  return DKG_OK;
}

int dkg_jes_forward(const void* host_plan, const double* x, int B, double* acq, double* dacq_dx, double* moments_out,
                    void* stream) {
  if (!host_plan || !x || !acq) return failf(DKG_ERR_ARG, "NULL pointer");
  const JesPlan& p = static_cast<const JesHost*>(host_plan)->plan;
  if (p.magic != JES_MAGIC) return failf(DKG_ERR_ARG, "the plan is not initialised (dkg_jes_init)");
  if (B < 1 || B > p.max_B) return failf(DKG_ERR_ARG, "B=%d candidates outside [1, max_B=%d]", B, p.max_B);
  hipStream_t s = (hipStream_t)stream;
  const int grad = dacq_dx != nullptr;
  JesMomArgs ma{p.tab, x, p.mu, p.q2, p.dmu, p.dvar, B, p.d, p.bpad, grad};
  const dim3 mgrid((B + 15) / 16, p.SO), mblock(JM_WAVES * WAVE);
  const size_t mlds = jes_mom_lds_bytes(p.max_np);
  by_dim(p.d, [&](auto dm) { launch_lds(jes_moments_kernel<decltype(dm)::value>, mgrid, mblock, mlds, s, ma); });
  int st = hip_status(hipGetLastError(), "jes_moments_kernel");
  if (st) return st;
  JesEntArgs ea{p.tab, p.bounds, p.mu, p.q2, p.dmu, p.dvar, acq, dacq_dx, moments_out,
                p.m, p.P, p.d, p.J, p.target, p.only_diag, B, p.bpad, grad};
  const dim3 egrid(B), eblock(JE_WAVES * WAVE);
  const size_t elds = (size_t)(p.P + 1) * (1 + p.d) * sizeof(double);
  if (p.m == 1) hipLaunchKernelGGL(jes_entropy_kernel<1>, egrid, eblock, elds, s, ea);
  else if (p.m == 2) hipLaunchKernelGGL(jes_entropy_kernel<2>, egrid, eblock, elds, s, ea);
  else if (p.m <= 4) hipLaunchKernelGGL(jes_entropy_kernel<4>, egrid, eblock, elds, s, ea);
  else hipLaunchKernelGGL(jes_entropy_kernel<8>, egrid, eblock, elds, s, ea);
  return hip_status(hipGetLastError(), "jes_entropy_kernel");
}

}  // extern "C"
