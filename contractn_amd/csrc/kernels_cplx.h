// kernels_cplx.h - complex results: the reference's normalisation by the mean MODULUS and its backward.
// A complex network runs as a real plan on (re, im) components, whose per-step stabilisation normalises by the mean of
// |re| + |im|; these kernels bring its finished result (T_e, c_e) to the reference's split (T, c) on the device.
// Data are interleaved (re, im) pairs of float or double components, n complex elements; loads and stores are 16 bytes
// wide (float4 = two complex64, double2 = one complex128) with a scalar tail when a pointer is not 16-byte aligned.
// Part of the gfx950 contraction engine (see engine.hip for the overview).
#pragma once
#include "kernel_args.h"

namespace ctn {

// Partial sums of the reductions: one double per workgroup of the reducing launch, summed in one fixed order by every
// thread of the launch that consumes them, so results are bit-reproducible (no atomics).
constexpr int kCplxBlocks = 1024;

// |z| in double: float components cannot overflow their squares there; double components go through hypot.
__device__ __forceinline__ double cplx_modulus(float re, float im) {
  return sqrt((double)re * (double)re + (double)im * (double)im);
}
__device__ __forceinline__ double cplx_modulus(double re, double im) { return hypot(re, im); }

// ---------------------------------------------------------------------------
// k_cplx_abs_sum: scratch[block] = sum of |t_i| over the elements of this workgroup (fixed grid, fixed order).
// ---------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void k_cplx_abs_sum(const T* __restrict__ t, int64_t n, int vec,
                                                      double* __restrict__ scratch) {
  __shared__ double red[4];
  constexpr int V = 16 / (int)sizeof(T);            // components per vector: whole (re, im) pairs
  typedef T vecT __attribute__((ext_vector_type(V)));
  const int64_t stride = (int64_t)gridDim.x * 256;
  const int64_t nv = vec ? 2 * n / V : 0;
  double v = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nv; i += stride) {
    const vecT x = reinterpret_cast<const vecT*>(t)[i];
#pragma unroll
    for (int j = 0; j < V; j += 2) v += cplx_modulus(x[j], x[j + 1]);
  }
  for (int64_t i = nv * V / 2 + (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride)
    v += cplx_modulus(t[2 * i], t[2 * i + 1]);
  const double tot = block_sum(v, red);
  if (threadIdx.x == 0) scratch[blockIdx.x] = tot;
}

// ---------------------------------------------------------------------------
// k_cplx_normalize: t = t_e / rho with rho = (T)(sum|t_e| / n) from the partials, c = c_e + log(rho) in T,
// *rho_out = rho.  rescaled == 0: t = t_e (a copy unless in place), c = c_e, *rho_out = 1.  t may alias t_e.
// ---------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void k_cplx_normalize(const T* src, T* dst, int64_t n, int vec,
                                                        const double* __restrict__ scratch, int parts, int rescaled,
                                                        const T* __restrict__ c_e, T* __restrict__ c_out,
                                                        double* __restrict__ rho_out) {
  double norm = 0.0;
  for (int j = 0; j < parts; ++j) norm += scratch[j];              // same order in every thread of every workgroup
  const T rho = rescaled ? (T)(norm / (double)n) : (T)1;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    c_out[0] = rescaled ? (T)(c_e[0] + (T)log((double)rho)) : c_e[0];
    rho_out[0] = (double)rho;
  }
  if (!rescaled && src == dst) return;
  constexpr int V = 16 / (int)sizeof(T);
  typedef T vecT __attribute__((ext_vector_type(V)));
  const int64_t stride = (int64_t)gridDim.x * 256;
  const int64_t nv = vec ? 2 * n / V : 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nv; i += stride) {
    vecT x = reinterpret_cast<const vecT*>(src)[i];
    if (rescaled) {
#pragma unroll
      for (int j = 0; j < V; ++j) x[j] = x[j] / rho;
    }
    reinterpret_cast<vecT*>(dst)[i] = x;
  }
  for (int64_t i = nv * V + (int64_t)blockIdx.x * 256 + threadIdx.x; i < 2 * n; i += stride)
    dst[i] = rescaled ? src[i] / rho : src[i];
}

// ---------------------------------------------------------------------------
// Backward of a rescaled k_cplx_normalize.  k_cplx_grad_dot: scratch[block] = partial of <g, t> = sum (gr tr + gi ti).
// k_cplx_grad_apply: g_te = [g - (<g, t> - g_c) u / n] / rho with u = t / |t| (0 where t = 0); g == nullptr: g = 0,
// g_c == nullptr: g_c = 0.  Everything in double, rounded once.
// ---------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void k_cplx_grad_dot(const T* __restrict__ g, const T* __restrict__ t, int64_t n,
                                                       int vec, double* __restrict__ scratch) {
  __shared__ double red[4];
  constexpr int V = 16 / (int)sizeof(T);
  typedef T vecT __attribute__((ext_vector_type(V)));
  const int64_t stride = (int64_t)gridDim.x * 256;
  const int64_t nv = vec ? 2 * n / V : 0;
  double v = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nv; i += stride) {
    const vecT x = reinterpret_cast<const vecT*>(g)[i];
    const vecT y = reinterpret_cast<const vecT*>(t)[i];
#pragma unroll
    for (int j = 0; j < V; ++j) v += (double)x[j] * (double)y[j];
  }
  for (int64_t i = nv * V + (int64_t)blockIdx.x * 256 + threadIdx.x; i < 2 * n; i += stride)
    v += (double)g[i] * (double)t[i];
  const double tot = block_sum(v, red);
  if (threadIdx.x == 0) scratch[blockIdx.x] = tot;
}

template <typename T>
__global__ __launch_bounds__(256) void k_cplx_grad_apply(const T* __restrict__ g, const T* __restrict__ t, int64_t n,
                                                         int vec, const double* __restrict__ scratch, int parts,
                                                         const T* __restrict__ g_c, const double* __restrict__ rho,
                                                         T* __restrict__ out) {
  double dot = 0.0;
  for (int j = 0; j < parts; ++j) dot += scratch[j];                // same order in every thread of every workgroup
  const double alpha = (dot - (g_c ? (double)g_c[0] : 0.0)) / (double)n;
  const double r = rho[0];
  constexpr int V = 16 / (int)sizeof(T);
  typedef T vecT __attribute__((ext_vector_type(V)));
  const int64_t stride = (int64_t)gridDim.x * 256;
  const int64_t nv = vec ? 2 * n / V : 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nv; i += stride) {
    const vecT y = reinterpret_cast<const vecT*>(t)[i];
    const vecT x = g ? reinterpret_cast<const vecT*>(g)[i] : y;
    vecT o;
#pragma unroll
    for (int j = 0; j < V; j += 2) {
      const double tr = (double)y[j], ti = (double)y[j + 1];
      const double m = cplx_modulus(y[j], y[j + 1]);
      const double ur = m > 0.0 ? tr / m : 0.0, ui = m > 0.0 ? ti / m : 0.0;
      const double gr = g ? (double)x[j] : 0.0, gi = g ? (double)x[j + 1] : 0.0;
      o[j] = (T)((gr - alpha * ur) / r);
      o[j + 1] = (T)((gi - alpha * ui) / r);
    }
    reinterpret_cast<vecT*>(out)[i] = o;
  }
  for (int64_t i = nv * V / 2 + (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    const double tr = (double)t[2 * i], ti = (double)t[2 * i + 1];
    const double m = cplx_modulus(t[2 * i], t[2 * i + 1]);
    const double ur = m > 0.0 ? tr / m : 0.0, ui = m > 0.0 ? ti / m : 0.0;
    const double gr = g ? (double)g[2 * i] : 0.0, gi = g ? (double)g[2 * i + 1] : 0.0;
    out[2 * i] = (T)((gr - alpha * ur) / r);
    out[2 * i + 1] = (T)((gi - alpha * ui) / r);
  }
}

}  // namespace ctn
