// kernels_grad.h - reverse mode of the stabilised contraction ("Autograd"): the split-format seed and the
// leaf write.  The cotangent contractions themselves are ordinary one-step plans run on the forward kernels.
// Part of the gfx950 contraction engine (see engine.hip for the overview).
#pragma once
#include "kernel_args.h"

namespace ctn {

// ---------------------------------------------------------------------------
// k_grad_seed_*: the cotangent of the plain value Z of a rescaled step from those of its split outputs
// (Z_hat = Z / mean|Z|, z = log mean|Z|), everything in split form G = G_hat e^g:
//     G_Z = e^{g - z} [G_hat - (<G_hat, Z_hat> - G_c e^{-g}) sign(Z_hat) / N]
// then re-stabilised: out = bracket / mean|bracket|, g_out = g - z + log mean|bracket| (when sum|bracket| > min_norm).
// Three launches of kGradSeedBlocks workgroups at most: the partial dot products, the bracket with its partial
// abs-sums, the division.  Every workgroup owns a fixed set of elements and every sum of partials runs in one fixed
// order, so the result is bit-reproducible.  g_hat == nullptr: G_hat = 0; g_c == nullptr: G_c = 0; g_in == nullptr:
// g = 0.  scratch: 2 * kGradSeedBlocks doubles.
// ---------------------------------------------------------------------------
constexpr int kGradSeedBlocks = 256;

// The bodies are shared with the *_tab entry kernels of the backward tape below: one text, the same bits.
template <typename T>
__device__ __forceinline__ void grad_seed_dot_body(const T* __restrict__ g_hat, const T* __restrict__ t_hat, int64_t n,
                                                   double* __restrict__ scratch) {
  __shared__ double red[4];
  double v = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    v += (double)g_hat[i] * (double)t_hat[i];
  const double tot = block_sum(v, red);
  if (threadIdx.x == 0) scratch[blockIdx.x] = tot;
}

template <typename T>
__device__ __forceinline__ void grad_seed_apply_body(const T* __restrict__ g_hat, const T* __restrict__ t_hat, int64_t n,
                                                     const T* __restrict__ g_c, const double* __restrict__ g_in,
                                                     int dot_parts, double* __restrict__ scratch, T* __restrict__ out) {
  __shared__ double red[4];
  double dot = 0.0;
  for (int j = 0; j < dot_parts; ++j) dot += scratch[j];          // same order in every thread of every workgroup
  const double gc = g_c ? (double)g_c[0] : 0.0;
  const double g = g_in ? g_in[0] : 0.0;
  const double alpha = (dot - (gc == 0.0 ? 0.0 : gc * exp(-g))) / (double)n;
  double absv = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const double t = (double)t_hat[i];
    const double sg = t > 0.0 ? 1.0 : (t < 0.0 ? -1.0 : 0.0);     // sign(0) = 0, as torch.sign
    const T b = (T)((g_hat ? (double)g_hat[i] : 0.0) - alpha * sg);
    out[i] = b;
    absv += fabs((double)b);
  }
  const double tot = block_sum(absv, red);
  if (threadIdx.x == 0) scratch[kGradSeedBlocks + blockIdx.x] = tot;
}

template <typename T>
__device__ __forceinline__ void grad_seed_norm_body(T* __restrict__ out, int64_t n, const double* __restrict__ z,
                                                    const double* __restrict__ g_in, int parts,
                                                    const double* __restrict__ scratch, double min_norm,
                                                    double* __restrict__ g_out) {
  double norm = 0.0;
  for (int j = 0; j < parts; ++j) norm += scratch[kGradSeedBlocks + j];
  const bool resc = norm > min_norm;
  const double mean = norm / (double)n;
  if (resc)
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
      out[i] = (T)((double)out[i] / mean);
  if (blockIdx.x == 0 && threadIdx.x == 0)
    g_out[0] = (g_in ? g_in[0] : 0.0) - z[0] + (resc ? log(mean) : 0.0);
}

template <typename T>
__global__ __launch_bounds__(256) void k_grad_seed_dot(const T* __restrict__ g_hat, const T* __restrict__ t_hat,
                                                       int64_t n, double* __restrict__ scratch) {
  grad_seed_dot_body<T>(g_hat, t_hat, n, scratch);
}

template <typename T>
__global__ __launch_bounds__(256) void k_grad_seed_apply(const T* __restrict__ g_hat, const T* __restrict__ t_hat,
                                                         int64_t n, const T* __restrict__ g_c,
                                                         const double* __restrict__ g_in, int dot_parts,
                                                         double* __restrict__ scratch, T* __restrict__ out) {
  grad_seed_apply_body<T>(g_hat, t_hat, n, g_c, g_in, dot_parts, scratch, out);
}

template <typename T>
__global__ __launch_bounds__(256) void k_grad_seed_norm(T* __restrict__ out, int64_t n, const double* __restrict__ z,
                                                        const double* __restrict__ g_in, int parts,
                                                        const double* __restrict__ scratch, double min_norm,
                                                        double* __restrict__ g_out) {
  grad_seed_norm_body<T>(out, n, z, g_in, parts, scratch, min_norm, g_out);
}

// ---------------------------------------------------------------------------
// k_grad_leaf: one operand's gradient, written destination-driven in the operand's own shape (C-contiguous) and
// dtype, dst[i] = src[sum_d c_d src_stride[d]] * e^{g}.  The cotangent contraction left its result in whatever axis
// order its plan chose: src_stride[d] is the stride of axis d's label in that result, 0 for a label the result does
// not carry (summed inside the operand alone: the gradient is constant along it).  A label repeated in the operand
// (a trace, `aa->`) is read at its first axis (first[d] == d) and the element is 0 where the repeats disagree.  An
// exact zero stays 0 whatever e^{g}; anything else overflows to inf as the reference's own graph does.
// ---------------------------------------------------------------------------
constexpr int kGradMaxDims = 64;
struct GradLeafArgs {
  int64_t numel;
  int32_t ndim, pad;
  int64_t dims[kGradMaxDims];
  int64_t dst_stride[kGradMaxDims];
  int64_t src_stride[kGradMaxDims];
  int32_t first[kGradMaxDims];
};

template <typename TS, typename TD>
__device__ __forceinline__ void grad_leaf_body(const GradLeafArgs& a, const TS* __restrict__ src,
                                               const double* __restrict__ g, TD* __restrict__ dst) {
  const double m = g ? exp(g[0]) : 1.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.numel; i += (int64_t)gridDim.x * 256) {
    int64_t off = 0;
    bool on = true;
    for (int d = 0; d < a.ndim; ++d) {
      const int64_t c = (i / a.dst_stride[d]) % a.dims[d];
      const int f = a.first[d];
      if (f != d) {
        if (c != (i / a.dst_stride[f]) % a.dims[f]) { on = false; break; }
      } else {
        off += c * a.src_stride[d];
      }
    }
    const double v = on ? (double)src[off] : 0.0;
    dst[i] = (TD)(v == 0.0 ? 0.0 : v * m);
  }
}

template <typename TS, typename TD>
__global__ __launch_bounds__(256) void k_grad_leaf(GradLeafArgs a, const TS* __restrict__ src,
                                                   const double* __restrict__ g, TD* __restrict__ dst) {
  grad_leaf_body<TS, TD>(a, src, g, dst);
}

// ---------------------------------------------------------------------------
// The backward tape (include/ctn_abi.h, ctn_grad_tape_*): the same kernels with every tensor pointer read from the
// tape's device table of slot addresses, tab[slot] (slot < 0: nullptr), so that a captured launch follows the caller's
// tensors from run to run.  They call the bodies of the kernels above with the same launch geometry: same bits.
// ---------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ T* tape_ptr(void* const* __restrict__ tab, int slot) {
  return slot < 0 ? nullptr : (T*)tab[slot];
}

template <typename T>
__global__ __launch_bounds__(256) void k_grad_seed_dot_tab(void* const* __restrict__ tab, int s_g, int s_t, int64_t n,
                                                           double* __restrict__ scratch) {
  grad_seed_dot_body<T>(tape_ptr<const T>(tab, s_g), tape_ptr<const T>(tab, s_t), n, scratch);
}

template <typename T>
__global__ __launch_bounds__(256) void k_grad_seed_apply_tab(void* const* __restrict__ tab, int s_g, int s_t, int64_t n,
                                                             int s_gc, const double* __restrict__ g_in, int dot_parts,
                                                             double* __restrict__ scratch, int s_out) {
  grad_seed_apply_body<T>(tape_ptr<const T>(tab, s_g), tape_ptr<const T>(tab, s_t), n, tape_ptr<const T>(tab, s_gc), g_in,
                          dot_parts, scratch, tape_ptr<T>(tab, s_out));
}

template <typename T>
__global__ __launch_bounds__(256) void k_grad_seed_norm_tab(void* const* __restrict__ tab, int s_out, int64_t n,
                                                            const double* __restrict__ z, const double* __restrict__ g_in,
                                                            int parts, const double* __restrict__ scratch, double min_norm,
                                                            double* __restrict__ g_out) {
  grad_seed_norm_body<T>(tape_ptr<T>(tab, s_out), n, z, g_in, parts, scratch, min_norm, g_out);
}

template <typename TS, typename TD>
__global__ __launch_bounds__(256) void k_grad_leaf_tab(GradLeafArgs a, void* const* __restrict__ tab, int s_src,
                                                       const double* __restrict__ g, int s_dst) {
  grad_leaf_body<TS, TD>(a, tape_ptr<const TS>(tab, s_src), g, tape_ptr<TD>(tab, s_dst));
}

// k_tape_regs: the register work behind a RUN record in one launch - regs[r_log] = the run's log register (what
// ctn_exec_snapshot_scales copies) and regs[r_dst] = regs[r_log] + regs[k0] + regs[k1], added left to right as
// k_scales_add adds them (k < 0: no such term).  One lane, plain vector stores.
__global__ __launch_bounds__(64) void k_tape_regs(const double* __restrict__ run_log, double* __restrict__ regs, int r_log,
                                                  int r_dst, int k0, int k1) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double v = run_log[0];
  regs[r_log] = v;
  if (k0 >= 0) v += regs[k0];
  if (k1 >= 0) v += regs[k1];
  regs[r_dst] = v;
}

// k_run_close: everything behind the step of a ONE-step, one-replica run in one launch (CTN_GRAD_CLOSE=1) - what k_scales,
// k_finalize and k_tape_regs do in three.  Grid (fb, 1) as k_finalize's.  Every wave of every workgroup derives the step's
// factor itself from the partials, with k_scales' own producer_scale call (a fixed order: the same bits everywhere), so
// no workgroup reads what another one writes in this launch; then the workgroup divides its share of the result with
// k_finalize's two loops.  Workgroup 0 also writes, from one lane, the run's factor and log (f.rescales[0], logs[0]),
// its register f.log_scale[0] - block_sum of ONE term is 0.0 + term -, and the tape's registers as k_tape_regs does.
// Never launched with f.defer set.
template <typename T>
__global__ __launch_bounds__(256) void k_run_close(FinalArgs f, double* __restrict__ logs, double* __restrict__ regs,
                                                   int r_log, int r_dst, int k0, int k1) {
  bool cond = false;
  T sc = (T)1;
  if (f.stabilize)
    sc = producer_scale<T>(f.partials + (size_t)f.stepOff[0] * f.R, f.stepP[0], f.stepSlots[0], f.stepNumel[0],
                           f.min_norm, 0, &cond);
  const double rl = cond ? (double)sc : 0.0;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const double lg = cond ? (double)log(sc) : 0.0;
    f.rescales[0] = rl;
    logs[0] = lg;
    double v = 0.0 + lg;
    f.log_scale[0] = v;
    regs[r_log] = v;
    if (k0 >= 0) v += regs[k0];
    if (k1 >= 0) v += regs[k1];
    regs[r_dst] = v;
  }
  if (!f.stabilize) return;
  if (rl == 0.0) return;  // the step was not rescaled (norm <= min_norm): tensor unchanged
  const T s_last = (T)rl;
  T* out = (T*)f.ptrs[f.id_out];
  constexpr int V = 16 / (int)sizeof(T);
  typedef T vecT __attribute__((ext_vector_type(V)));
  const int64_t nv = f.vec ? f.out_numel / V : 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nv; i += (int64_t)gridDim.x * 256) {
    vecT v = reinterpret_cast<vecT*>(out)[i];
#pragma unroll
    for (int j = 0; j < V; ++j) v[j] = v[j] / s_last;
    reinterpret_cast<vecT*>(out)[i] = v;
  }
  for (int64_t i = nv * V + (int64_t)blockIdx.x * 256 + threadIdx.x; i < f.out_numel; i += (int64_t)gridDim.x * 256)
    out[i] = out[i] / s_last;
}

}  // namespace ctn
