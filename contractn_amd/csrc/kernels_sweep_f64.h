// kernels_sweep_f64.h - the batched-MPS sweep of kernels_sweep.h in float64: every site of the chain inside ONE launch, a
// block of 16 inputs per workgroup, v_mfma_f64_16x16x4_f64.  Part of the gfx950 contraction engine (see engine.hip).
#pragma once
#include "kernels_sweep.h"
#include "kernels_zip_f64.h"

namespace ctn {

// ---------------------------------------------------------------------------
// K-sweep-f64.  Per site, as in kernels_sweep.h,
//
//     C[b, (p, r)] = sum_l E[b, l] W_s[l, p, r]        E'[b, r] = sum_p x_s[b, p] C[b, (p, r)]
//
// but the float64 plan keeps these as TWO steps (a GEMM that writes the B x P x D intermediate and a streaming step that
// reads it back: plan.cpp fuses the pair for fp32 only), and reports a rescale factor for both.  Here a workgroup owns 16
// inputs, keeps their state E (16 x D doubles) in LDS from the first site to the last, and the cores stream from L2
// straight into MFMA operand registers by 16-byte loads; C only ever exists in accumulators.
//
// v_mfma_f64_16x16x4_f64, D[i][j = b] (the register <-> row correspondence is that of kernels_zip_f64.h):
//   A operand: lane (i = lane & 15, kg = lane >> 4) holds W_s[l][p][rb + 2 i + c], c = 0, 1 - ONE 16-byte load feeds the
//              two accumulators (p, c); rb = 32 x (the wave's range of r);
//   B operand: lane (j = b, kg) holds E[b][l];
//   k-step t = 0..3 of a group G of 16 values of l pairs lane group kg with l = 16 G + 4 kg + t: a lane's four B operands of
//   a group are 32 consecutive bytes of its LDS row;
//   D: lane (b, h = lane >> 4) holds row i = h + 4 e in register e: r = rb + 2 h + 8 e + c - 16-byte stores of the pair c.
// EVERY wave owns the whole range of l for its columns (no split of l, NL = 1): the abs-sum of the un-rescaled C, which the
// plan's first step of a site reports, needs the complete sum over l before the absolute value - and the hand-over
// barrier of k_sweep_f32 goes away.  A wave owns 32 values of r at a time (2 P accumulators of 8 registers): 2 / 4 / 8 waves
// at D = 64 / 128 / 256; at D = 512 8 waves own 64 values of r each and walk l TWICE per site, 32 values of r per pass
// (16 waves would leave each 128 registers, 4 P accumulators at once leave no room for the queue: both spill).
// The cores are requested QD k-steps ahead into a register queue that runs on across site boundaries; ONE barrier per site
// (E' and both abs-sums complete), for which only LDS traffic is waited for.
//
// Stabilisation.  A workgroup rescales its 16 rows by a POWER OF TWO, 2^e with e = ilogb of their mean |.| (the scale goes
// into the weights x_s, exactly), and records the integer e.  With g[j][s] = sum_{i <= s} e[i][j] (an exact integer), the
// whole tensor's abs-sum at any step is sum_j a[j] 2^g[j] - a fixed-order sum of exactly scaled terms - and the factor that
// brings a block's last rows to the common scale is an exact ldexp times ONE factor common to the tensor.  (Free scales, as
// in fp32, would put exp(sum of logs) with a relative error of |sum log s| 2^-53 on every BLOCK.)  Per (replica, site,
// block) the kernel records the abs-sum of C and of E', both at the block scale g[j][s - 1], and e.
//
// Conditions (engine.hip, sweep64_match): fp64, |l| = |r| = 64, 128, 256 or 512, |p| = 2 or 4, W_s and x_s network inputs
// with r and p unit-stride, E row-major, every stride even (16-byte accesses).  No atomics, every sum in a fixed order.
// ---------------------------------------------------------------------------
struct Sweep64Args {
  void* const* ptrs;         // [R][n_tensors]
  int32_t n_tensors;
  const int32_t* site_ids;   // [S][2]: tensor ids of (W_s, x_s)
  int32_t idIn, idOut;       // the chain's input E [b][l] and its output E' [b][r]
  int32_t S, J, M;           // sites, row blocks (ceil(rows / 16)), rows
  int64_t ldIn, ldOut;       // row strides of input and output (elements)
  int64_t ldWl, ldWp;        // W_s[l][p][r]: strides of l and p (r unit-stride)
  int64_t ldX;               // x_s[b][p]: row stride (p unit-stride)
  const double* partIn;      // the input's producer partials (nullptr: a network input)
  int32_t PIn, strideIn;
  double numelIn, min_norm;
  double* rec_a;             // [R][2 S][J] abs-sums of a block's C (entry 2 s) and E' (2 s + 1) at the scale g[j][s - 1]
  int32_t* rec_e;            // [R][S][J] the exponent the block then applied (0 after the last site)
};

typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(1))) double* sw_gout64;

constexpr int kSweep64MaxExp = 1000;   // |e| of one site at most: 2^-e stays a normal number

template <int D>
struct Sweep64Shape {
  static constexpr int RW = D == 512 ? 2 : 1;          // ranges of 32 values of r per wave: passes over l per site
  static constexpr int NWV = D / (32 * RW);            // waves: 2, 4, 8, 8
  static constexpr int NT = 64 * NWV;
};

template <int D, int P>
__global__ __launch_bounds__(Sweep64Shape<D>::NT, 1) void k_sweep_f64(Sweep64Args a) {
  constexpr int RW = Sweep64Shape<D>::RW, NWV = Sweep64Shape<D>::NWV, NT = Sweep64Shape<D>::NT;
  constexpr int NG = D / 16;                  // groups of 16 values of l per site
  constexpr int QD = 4;                       // k-steps of W in flight per wave
  constexpr int LD = D + 2;                   // image rows 16 bytes more than D doubles apart
  static_assert((D == 64 || D == 128 || D == 256 || D == 512) && (P == 2 || P == 4), "shape");
  __shared__ __attribute__((aligned(16))) double img[2][SWR * LD];
  __shared__ double red[2][NWV][2];           // per site parity: a wave's abs-sums of C and E'
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i16 = lane & 15, kg = lane >> 4;
  const int j = blockIdx.x, r = blockIdx.y;
  void* const* tp = a.ptrs + (size_t)r * a.n_tensors;
  const int rows = min(SWR, a.M - SWR * j);   // the last block of a batch that is not a multiple of 16: its other rows stay zero

  // the chain's input, normalised by its producer's mean (the lazy rescale: reference einsum.py:387 on the step before)
  {
    double pv = 0.0;
    if (a.partIn) {
      const double* __restrict__ pr = a.partIn + (size_t)r * a.strideIn;
      pv = pr[min(lane, a.PIn - 1)];
      if (a.PIn > 64)
        for (int i = lane + 64; i < a.PIn; i += 64) pv += pr[i];
      pv = lane < a.PIn ? pv : 0.0;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) pv += __shfl_xor(pv, o, 64);
    }
    const double inv = (a.partIn && pv > a.min_norm) ? 1.0 / (pv / a.numelIn) : 1.0;
    const double* __restrict__ Ein = (const double*)tp[a.idIn] + (int64_t)(SWR * j) * a.ldIn;
    for (int i = tid; i < SWR * D / 2; i += NT) {
      const int row = i / (D / 2), c2 = i - row * (D / 2);
      double2 v = make_double2(0.0, 0.0);
      if (row < rows) v = *reinterpret_cast<const double2*>(Ein + (int64_t)row * a.ldIn + 2 * c2);
      *reinterpret_cast<double2*>(&img[0][row * LD + 2 * c2]) = make_double2(v.x * inv, v.y * inv);
    }
  }

  // a lane's own offsets into a core (bytes): row 4 kg of a group of l, its two columns r of every p in the wave's first range
  uint32_t voff[P];
#pragma unroll
  for (int p = 0; p < P; ++p) voff[p] = (uint32_t)(((int64_t)(4 * kg) * a.ldWl + (int64_t)p * a.ldWp + 32 * RW * w + 2 * i16) * 8);
  const int64_t stepW = a.ldWl * 8;           // next k-step of a group (bytes)

  sw_gptr Wcur = (sw_gptr)tp[a.site_ids[0]];
  sw_gptr Xcur = (sw_gptr)tp[a.site_ids[1]];
  f64x2 wq[QD][P];
  auto wrequest = [&](f64x2 (&dst)[P], sw_gptr from) {
#pragma unroll
    for (int p = 0; p < P; ++p) dst[p] = *reinterpret_cast<const __attribute__((address_space(1))) f64x2*>(from + voff[p]);
  };
#pragma unroll
  for (int u = 0; u < QD; ++u) wrequest(wq[u], Wcur + (int64_t)u * stepW);

  f64x4 acc[P][2];
#pragma unroll
  for (int p = 0; p < P; ++p)
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[p][c][e] = 0.0;

  __syncthreads();                            // the input image is in place
  double inv_s = 1.0;                         // 2^-e of the site before: the state in LDS is the un-rescaled one
  int cur = 0;
  sw_gptr Wnext = Wcur, Xnext = Xcur;
  for (int s = 0; s < a.S; ++s) {
    const bool last = s + 1 == a.S;
    // next site's tensors (the last site re-requests its own first k-steps: in bounds, never used)
    const int sn = last ? s : s + 1;
    Wnext = (sw_gptr)tp[a.site_ids[2 * sn]];
    Xnext = (sw_gptr)tp[a.site_ids[2 * sn + 1]];
    double xr[P];                              // the inputs' weights of this site (rows beyond the batch: 0)
    {
      const int row = min(SWR * j + i16, a.M - 1);
      sw_gptr xp = Xcur + (int64_t)row * a.ldX * 8;
#pragma unroll
      for (int p2 = 0; p2 < P / 2; ++p2) {
        const f64x2 v = *reinterpret_cast<const __attribute__((address_space(1))) f64x2*>(xp + 16 * p2);
        xr[2 * p2] = v.x; xr[2 * p2 + 1] = v.y;
      }
    }
    const double* erow = &img[cur][i16 * LD + 4 * kg];
    // the site's epilogue works on the un-rescaled state in LDS: its scale 2^-e goes into the weights (exact)
    double xs[P];
    const int nxt = cur ^ 1;
    double asumC = 0.0, asumE = 0.0;
#pragma unroll 1
    for (int q = 0; q < RW; ++q) {             // a pass over l: the wave's range q of 32 values of r
      sw_gptr wpass = Wcur + 256 * q;          // (32 doubles further along r)
      sw_gptr wafter = q == RW - 1 ? Wnext : wpass + 256;   // what follows the pass: the next range, or the next site's first
      double2 ef0 = *reinterpret_cast<const double2*>(erow), ef1 = *reinterpret_cast<const double2*>(erow + 2);
#pragma unroll 1
      for (int G = 0; G < NG; ++G) {
        const int gn = G == NG - 1 ? 0 : G + 1;   // the next group's B operands (after the last group: read, never used)
        sw_gptr wg = wpass + (int64_t)(16 * G) * stepW;
        sw_gptr wn = G == NG - 1 ? wafter : wg + 16 * stepW;
        const double2 en0 = *reinterpret_cast<const double2*>(erow + 16 * gn), en1 = *reinterpret_cast<const double2*>(erow + 16 * gn + 2);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const double ev = t == 0 ? ef0.x : t == 1 ? ef0.y : t == 2 ? ef1.x : ef1.y;
#pragma unroll
          for (int p = 0; p < P; ++p)
#pragma unroll
            for (int c = 0; c < 2; ++c)
              acc[p][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(wq[t % QD][p][c], ev, acc[p][c], 0, 0, 0);
          wrequest(wq[t % QD], t + QD < 4 ? wg + (int64_t)(t + QD) * stepW : wn + (int64_t)(t + QD - 4) * stepW);
        }
        ef0 = en0; ef1 = en1;
      }
      // ---- the pass's epilogue.  A lane has C[b = i16][p][r] for r = 32 (RW w + q) + 2 kg + 8 e + c: the complete sum over l.
#pragma unroll
      for (int p = 0; p < P; ++p) xs[p] = (SWR * j + i16 < a.M ? xr[p] : 0.0) * inv_s;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        double o[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          double v = xs[0] * acc[0][c][e];
          double ac = fabs(acc[0][c][e]);
#pragma unroll
          for (int p = 1; p < P; ++p) {
            v = fma(xs[p], acc[p][c][e], v);
            ac += fabs(acc[p][c][e]);
          }
          o[c] = v;
          asumC += ac;
        }
        const int col = 32 * (RW * w + q) + 2 * kg + 8 * e;
        if (last) {   // the last site's rows leave with this block's own scale (k_sweep64_finish brings them to the common one)
          if (i16 < rows) {
            sw_gout64 og = (sw_gout64)tp[a.idOut] + (int64_t)(SWR * j + i16) * a.ldOut + col;
            *reinterpret_cast<__attribute__((address_space(1))) f64x2*>(og) = f64x2{o[0], o[1]};
          }
        } else {
          *reinterpret_cast<double2*>(&img[nxt][i16 * LD + col]) = make_double2(o[0], o[1]);
        }
        asumE += fabs(o[0]) + fabs(o[1]);
      }
#pragma unroll
      for (int p = 0; p < P; ++p)
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[p][c][e] = 0.0;
    }
#pragma unroll
    for (int of = 32; of > 0; of >>= 1) {
      asumC += __shfl_xor(asumC, of, 64);
      asumE += __shfl_xor(asumE, of, 64);
    }
    if (lane == 0) { red[s & 1][w][0] = asumC; red[s & 1][w][1] = asumE; }
    // one barrier per site; only the LDS traffic is waited for - the cores requested ahead stay in flight
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_waitcnt(0xC07F);       // lgkmcnt(0)
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    double totC = 0.0, totE = 0.0;
#pragma unroll
    for (int i = 0; i < NWV; ++i) { totC += red[s & 1][i][0]; totE += red[s & 1][i][1]; }
    int ex = 0;                               // an all-zero (or non-finite) block keeps its scale: the exponent stays finite
    if (!last && totE > 0.0 && totE < INFINITY) ex = max(-kSweep64MaxExp, min(kSweep64MaxExp, ilogb(totE / (double)(SWR * D))));
    if (tid == 0) {
      const size_t ra = ((size_t)r * 2 * a.S + 2 * s) * a.J + j;
      a.rec_a[ra] = totC * inv_s;             // C = (state) . W_s at the scale of the site before: the state's own 2^-e
      a.rec_a[ra + a.J] = totE;
      a.rec_e[((size_t)r * a.S + s) * a.J + j] = ex;
    }
    inv_s = ldexp(1.0, -ex);
    cur = nxt;
    Wcur = Wnext;
    Xcur = Xnext;
  }
}

// The bookkeeping behind a float64 sweep: two short launches over the 2 S entries t (2 s: C_s, numel B P D; 2 s + 1: E'_s,
// numel B D).
//
// k_sweep64_z: Z_t = log((1 / numel_t) sum_j a_t[j] 2^g[j][s - 1]), the log of the whole tensor's mean |.| at entry t.  The
// terms are scaled by ldexp to the largest exponent among them (exact), summed in a fixed order, and the mean m 2^x
// (1 <= m < 2) gives Z = log(m) + x ln 2: one log, one product, one sum - and exactly 0 for a mean of exactly 1.
// -inf: an all-zero tensor; NaN: a non-finite record.  grid (2 S, R), 256 threads.
// <TWO>: true - the float64 sweep and the two-step sites of k_sweep_small, as described; false (the epilogue-summed sites
// of k_sweep_small<float>, kernels_sweep_small.h) - ONE entry per site, E'_s: grid (S, R), rec_a [R][S][J], Z [R][S].
template <bool TWO>
__global__ __launch_bounds__(256) void k_sweep64_z(const double* __restrict__ rec_a, const int32_t* __restrict__ rec_e, int S, int J,
                                                   double numelC, double numelE, double* __restrict__ Z) {
  __shared__ double red[4];
  __shared__ int redi[4];
  constexpr int NE = TWO ? 2 : 1;              // entries per site
  const int t = blockIdx.x, s = TWO ? t >> 1 : t, r = blockIdx.y;
  const double* pa = rec_a + ((size_t)r * NE * S + t) * J;
  const int32_t* pe = rec_e + (size_t)r * S * J;
  constexpr int kNone = INT32_MIN, kBad = INT32_MAX;
  int mx = kNone;
  for (int j = threadIdx.x; j < J; j += 256) {
    const double av = pa[j];
    if (!(av < INFINITY)) { mx = kBad; continue; }
    if (av > 0.0) {
      int g = 0;
      for (int i = 0; i < s; ++i) g += pe[(size_t)i * J + j];
      mx = max(mx, ilogb(av) + g);
    }
  }
#pragma unroll
  for (int of = 32; of > 0; of >>= 1) mx = max(mx, __shfl_xor(mx, of, 64));
  if ((threadIdx.x & 63) == 0) redi[threadIdx.x >> 6] = mx;
  __syncthreads();
  mx = max(max(redi[0], redi[1]), max(redi[2], redi[3]));
  if (mx == kNone || mx == kBad) {            // (uniform over the workgroup)
    if (threadIdx.x == 0) Z[(size_t)r * NE * S + t] = mx == kNone ? -INFINITY : NAN;
    return;
  }
  double sum = 0.0;
  for (int j = threadIdx.x; j < J; j += 256) {
    const double av = pa[j];
    if (av > 0.0) {
      int g = 0;
      for (int i = 0; i < s; ++i) g += pe[(size_t)i * J + j];
      sum += ldexp(av, g - mx);
    }
  }
  const double tot = block_sum(sum, red);
  if (threadIdx.x == 0) {
    const double ratio = tot / ((!TWO || (t & 1)) ? numelE : numelC);
    const int x0 = ilogb(ratio);
    Z[(size_t)r * NE * S + t] = log(ldexp(ratio, -x0)) + (double)(x0 + mx) * 0.6931471805599453094;
  }
}

// k_sweep64_finish: the reference's rescale factors of the 2 S member steps from the Z_t, and the last site's rows at the
// common scale.  grid (J, R), 256 threads.  <T, TWO>: the element type of the rows (double; float: k_sweep_small<float>, whose
// rows are D % 4 == 0 floats - the same 16-byte pieces) and, as in k_sweep64_z, whether a site has two entries or one.
struct Sweep64Finish {
  void* const* ptrs;
  int32_t n_tensors, idOut, S, J, R, D, M;   // D: bond dimension; M: rows (the last block may hold fewer than 16)
  int64_t ldOut;
  const double* Z;           // [R][2 S] ([R][S]: one entry per site)
  const int32_t* rec_e;      // [R][S][J]
  const int64_t* part_off;   // [2 S] ([S]): the step's region in the partials buffer starts at part_off[t] * R doubles
  const int32_t* part_slots; // [2 S] ([S]): slots per replica of that region
  double* partials;
  double numelC, numelE, min_norm;
};

template <typename T_, bool TWO>
__global__ __launch_bounds__(256) void k_sweep64_finish(Sweep64Finish f) {
  static_assert(sizeof(T_) == 8 || sizeof(T_) == 4, "double or float");
  __shared__ double norm[(TWO ? 2 : 1) * kSweepMaxSites];
  __shared__ double common;
  __shared__ int shift;
  const int j = blockIdx.x, r = blockIdx.y, T = TWO ? 2 * f.S : f.S;
  const double* Z = f.Z + (size_t)r * T;
  if (threadIdx.x == 0) {
    // the reference's recurrence (einsum.py:97-106 over the chain's steps): norm_t = numel_t exp(Z_t) / R_{t-1}; rescaled
    // iff norm_t > min_norm - the comparison k_scales makes on the slot written below -, then R_t = exp(Z_t)
    double logR = 0.0, logR_before_last = 0.0;
    for (int t = 0; t < T; ++t) {
      const double z = Z[t];
      const double nv = z == -INFINITY ? 0.0 : z != z ? INFINITY : ((!TWO || (t & 1)) ? f.numelE : f.numelC) * exp(z - logR);
      if (t + 1 == T) logR_before_last = logR;
      norm[t] = nv;
      if (nv > f.min_norm && z == z) logR = z;
    }
    // this block's rows of the last site: V = W 2^g[j][S - 2]; the reference's stored tensor = V / R_{2S-2}: an exact
    // ldexp by g - G0 times exp(G0 ln 2 - log R), G0 the nearest integer to log2 R - the same number in every block
    int g = 0;
    const int32_t* pe = f.rec_e + (size_t)r * f.S * f.J + j;
    for (int i = 0; i + 1 < f.S; ++i) g += pe[(size_t)i * f.J];
    const double G0 = rint(logR_before_last / 0.6931471805599453094);
    common = exp(G0 * 0.6931471805599453094 - logR_before_last);
    shift = g - (int)G0;
  }
  __syncthreads();
  if (j == 0) {                               // what each step's own launch would have left: its abs-sum, in slot 0
    for (int t = threadIdx.x; t < T; t += 256) {
      double* dst = f.partials + (size_t)f.part_off[t] * f.R + (size_t)r * f.part_slots[t];
      dst[0] = norm[t];
      for (int i = 1; i < f.part_slots[t]; ++i) dst[i] = 0.0;
    }
  }
  const double fac = common;
  const int sh = shift;
  const int rows = min(SWR, f.M - SWR * j);
  if constexpr (sizeof(T_) == 8) {
    double* out = (double*)f.ptrs[(size_t)r * f.n_tensors + f.idOut] + (int64_t)(SWR * j) * f.ldOut;
    const int q2 = f.D / 2;
    for (int i = threadIdx.x; i < rows * q2; i += 256) {
      const int row = i / q2, c2 = i - row * q2;
      double2* p = reinterpret_cast<double2*>(out + (int64_t)row * f.ldOut) + c2;
      double2 v = *p;
      v.x = ldexp(v.x * fac, sh); v.y = ldexp(v.y * fac, sh);
      *p = v;
    }
  } else {
    // float rows: the common factor rounded to float ONCE (the same number in every block), then as above
    const float ff = (float)fac;
    float* out = (float*)f.ptrs[(size_t)r * f.n_tensors + f.idOut] + (int64_t)(SWR * j) * f.ldOut;
    const int q4 = f.D / 4;
    for (int i = threadIdx.x; i < rows * q4; i += 256) {
      const int row = i / q4, c4 = i - row * q4;
      float4* p = reinterpret_cast<float4*>(out + (int64_t)row * f.ldOut) + c4;
      float4 v = *p;
      v.x = ldexpf(v.x * ff, sh); v.y = ldexpf(v.y * ff, sh); v.z = ldexpf(v.z * ff, sh); v.w = ldexpf(v.w * ff, sh);
      *p = v;
    }
  }
}

}  // namespace ctn
