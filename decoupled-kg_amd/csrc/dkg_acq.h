// What the acquisition and metric translation units share (dkg_pareto, dkg_jes, dkg_rff, dkg_hvkg, dkg_boxes): the
// dispatch from a run-time covariance family, input dimension or objective count to a kernel instantiation, a point
// scaled into registers and its padded distance, and the argument checks of a fitted output (the workspace carve is
// dkg_kernels.h's).
// Every device helper runs the operations its call sites ran, in their order.
#pragma once

#include <type_traits>

#include "dkg_kernels.h"

namespace dkg {

// f(integral_constant<int, KIND>) for the covariance family `kind` (wave-uniform)
template <class F>
__device__ __forceinline__ void with_kind(int kind, F&& f) {
  switch (kind) {
    case DKG_MATERN12: f(std::integral_constant<int, DKG_MATERN12>{}); break;
    case DKG_MATERN32: f(std::integral_constant<int, DKG_MATERN32>{}); break;
    case DKG_RBF: f(std::integral_constant<int, DKG_RBF>{}); break;
    default: f(std::integral_constant<int, DKG_MATERN52>{}); break;
  }
}

// dst[k] = src[min(k, d - 1)]: a row of d <= DM values in DM registers, the last one repeated (clamped loads, no
// branches)
template <int DM>
__device__ __forceinline__ void clamped_row(double (&dst)[DM], const double* __restrict__ src, int d) {
#pragma unroll
  for (int k = 0; k < DM; ++k) dst[k] = src[min(k, d - 1)];
}

// dst[k] = src[min(k, d - 1)] * il[k]: a point over the lengthscales (il: a clamped_row of 1 / lengthscale)
template <int DM>
__device__ __forceinline__ void scaled_point(double (&dst)[DM], const double* __restrict__ src, const double (&il)[DM],
                                             int d) {
#pragma unroll
  for (int k = 0; k < DM; ++k) dst[k] = src[min(k, d - 1)] * il[k];
}

// |a - b|^2 over the first d of DM coordinates as one fma chain; a coordinate past d adds t * 0
template <int DM>
__device__ __forceinline__ double sq_dist(const double (&a)[DM], const double (&b)[DM], int d) {
  double r2 = 0.0;
#pragma unroll
  for (int k = 0; k < DM; ++k) {
    const double t = a[k] - b[k];
    r2 = fma(t, (k < d) ? t : 0.0, r2);
  }
  return r2;
}

// Raises the kernel's dynamic-LDS limit where lds needs it, and launches
template <class K, class... A>
void launch_lds(K kern, dim3 grid, dim3 block, size_t lds, hipStream_t s, const A&... args) {
  raise_lds_limit(reinterpret_cast<const void*>(kern), lds);
  hipLaunchKernelGGL(kern, grid, block, lds, s, args...);
}

// f(integral_constant<int, DM>) for the dimension bucket DM = 2, 4, 8 or 16 >= d
template <class F>
void by_dim(int d, F&& f) {
  switch (dim_bucket(d)) {
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 8: f(std::integral_constant<int, 8>{}); break;
    default: f(std::integral_constant<int, 16>{}); break;
  }
}

// f(integral_constant<int, MB>) for the objectives' register bucket MB = 2, 4 or 8 >= m
template <class F>
void by_objectives(int m, F&& f) {
  if (m <= 2) f(std::integral_constant<int, 2>{});
  else if (m <= 4) f(std::integral_constant<int, 4>{});
  else f(std::integral_constant<int, 8>{});
}

// The limits on the output count and the input dimension
inline int check_dims(int m, int d) {
  if (m < 1) return failf(DKG_ERR_ARG, "m=%d outputs", m);
  if (m > DKG_MAX_OUTPUTS) return failf(DKG_ERR_UNSUPPORTED, "m=%d outputs (supported <= %d)", m, DKG_MAX_OUTPUTS);
  if (d < 1) return failf(DKG_ERR_ARG, "d=%d", d);
  if (d > DKG_MAX_DIM) return failf(DKG_ERR_UNSUPPORTED, "d=%d (supported 1..%d)", d, DKG_MAX_DIM);
  return DKG_OK;
}

// A fitted output as the kernels read it; who: the caller's name for it ("output 3"); need_root: R^T's fragments too
inline int check_output_state(const dkg_output& o, bool need_root, const char* who) {
  if (o.n < 1) return failf(DKG_ERR_ARG, "%s: n=%d training points", who, o.n);
  if (o.n > 1024) return failf(DKG_ERR_UNSUPPORTED, "%s: n=%d > 1024 training points", who, o.n);
  if (o.kernel < DKG_MATERN12 || o.kernel > DKG_RBF) return failf(DKG_ERR_ARG, "%s: kernel id %d", who, o.kernel);
  if (!o.inv_lengthscale || !o.train_x || !o.alpha || (need_root && !o.root_frag))
    return failf(DKG_ERR_ARG, "%s: NULL pointer", who);
  return DKG_OK;
}

}  // namespace dkg
