// kernels_sweep_small.h - the batched-MPS sweep of kernels_sweep.h at small bonds (8 ... 64): every site of the chain
// inside ONE launch, ONE WAVE per block of 16 inputs, the state in registers from the first site to the last.
// Part of the gfx950 contraction engine (see engine.hip).
#pragma once
#include "kernels_sweep_f64.h"

namespace ctn {

// ---------------------------------------------------------------------------
// K-sweep-small-f32.  Per site, as in kernels_sweep.h,
//
//     C[b, (p, r)] = sum_l E[b, l] W_s[l, p, r]        E'[b, r] = sum_p x_s[b, p] C[b, (p, r)]
//
// for bonds D = 8 ... 64 (a multiple of 4), where the planner either keeps a site as TWO launched steps (a GEMM and the
// streaming sum over p, both reporting a rescale factor: the shape of the float64 plan) or, from B D P >= 65536 on, as one
// epilogue-summed step behind an absorbed marker.  <DB, P, TWO>: DB = ceil(D / 16) blocks of 16 values of l and of r,
// the physical dimension, and which of the two plan shapes the records are for.  C exists in accumulators only.
//
// v_mfma_f32_16x16x4_f32, D[i = r][j = b]:
//   B operand: lane (j = b, kg = lane >> 4) holds E[b][l]; k-step t = 0..3 of a group G of 16 values of l pairs lane
//              group kg with l = 16 G + 4 kg + t (the pairing of kernels_sweep.h);
//   A operand: lane (i = lane & 15, kg) holds W_s[16 G + 4 kg + t][p][16 q + i] for the r-block q: 16 lanes read 64
//              consecutive bytes;
//   D: lane (b, g = lane >> 4) holds rows i = 4 g + e of r-block q in register e: r = 16 q + 4 g + e.
// After the sum over p, register e of r-block q in lane (b, g) is E'[b][16 q + 4 g + e] - which is, under that pairing,
// exactly the B operand of k-step t = e of group G = q of the NEXT site in lane (b, kg = g).  The state goes from
// accumulator to operand with no LDS, no barrier and no lane movement, for the whole chain; a wave shares nothing with any
// other wave, so a workgroup is ONE wave (a batch of 256 inputs spreads over 16 CUs, not 4) and the kernel has no LDS and
// no barrier at all.
//
// The A operand: direct 4-byte loads (a core is 1 ... 64 KiB and the same for every wave: L1 / L2 hits), requested 4 to 8
// k-steps ahead into a register queue that runs on across site boundaries, as in k_sweep_f32.  This is the variant that
// was measured (ahead of the per-site launches at all six shapes of tools/sweep_small_timing.py).  The
// other candidate, a workgroup of several waves staging W_s in LDS behind one barrier per site, was NOT built and not
// measured: it ties the waves of a workgroup together, where the point of this form is that a block of rows waits for nobody.
// (A workgroup is one wave, not several, and W is zero-filled per element, not per float4: D % 4 == 0 would allow either.)
// Ragged D: what a lane would read of W at or beyond D (l >= D or r >= D) is read from an in-bounds element instead and
// cleared by an AND mask - per element and without a branch -, so the padded entries of C and of the state are exact zeros
// on their own; the state's padded columns are never loaded from E and never stored.  Rows of a block past M: their state
// and weights are zero, never stored.  Means use numel = 16 D.
//
// Stabilisation: k_sweep_f64's protocol (kernels_sweep_f64.h) in float.  A block rescales its rows by 2^e,
// e = ilogb(mean |E'|), folded into the next site's weights x_s exactly; per (replica, site, block) the kernel records e,
// the abs-sum of E' and - TWO - of C, both at the block's scale g[j][s - 1]; the abs-sums are sums over a lane's
// registers in a fixed order, then over the lanes by six shuffle levels - spread over the NEXT site's k-steps, behind its
// MFMAs: only that site's epilogue needs e -: no barrier, no atomics, the same bits every run.  k_sweep64_z<TWO> and
// k_sweep64_finish<float, TWO> rebuild the reference's per-step rescale factors from the records.  !TWO: one entry per
// site (the member step); the absorbed marker has no entry and reports 0.
//
// Conditions (fused_forms.h, sweep_small_match): fp32, 8 <= |l| = |r| <= 64 a multiple of 4, |p| = 2 or 4, W_s and x_s network
// inputs with r and p unit-stride, E row-major, ldIn, ldOut, ldWl, ldWp multiples of 4 (16-byte accesses of the state's rows).
// ---------------------------------------------------------------------------
struct SweepSmallArgs {
  void* const* ptrs;         // [R][n_tensors]
  int32_t n_tensors;
  const int32_t* site_ids;   // [S][2]: tensor ids of (W_s, x_s)
  int32_t idIn, idOut;       // the chain's input E [b][l] and its output E' [b][r]
  int32_t S, J, M, D;        // sites, row blocks (ceil(rows / 16)), rows, bond dimension
  int64_t ldIn, ldOut;       // row strides of input and output (elements)
  int64_t ldWl, ldWp;        // W_s[l][p][r]: strides of l and p (r unit-stride)
  int64_t ldX;               // x_s[b][p]: row stride (p unit-stride)
  const double* partIn;      // the input's producer partials (nullptr: a network input)
  int32_t PIn, strideIn;
  double numelIn, min_norm;
  double* rec_a;             // TWO: [R][2 S][J] abs-sums of a block's C (entry 2 s) and E' (2 s + 1); else [R][S][J], E' alone -
                             // at the scale g[j][s - 1]
  int32_t* rec_e;            // [R][S][J] the exponent the block then applied (0 after the last site)
};

// k-steps of W in flight per wave: a divisor of the 4 DB k-steps of a site (the queue's slots then fall on the same k-steps
// in every site), 4 - or as many as 32 registers hold: a k-step's MFMAs are P DB x 32 cycles, an L2 hit is ~1000
template <int DB, int P>
constexpr int sweep_small_queue() { return DB == 2 && P == 2 ? 8 : DB == 3 && P == 2 ? 6 : 4; }
constexpr int kSweepSmallMaxExp = 100;   // |e| of one site at most: 2^-e stays a normal float

template <int DB, int P, bool TWO>
__global__ __launch_bounds__(64) void k_sweep_small_f32(SweepSmallArgs a) {
  static_assert(DB >= 1 && DB <= 4 && (P == 2 || P == 4), "shape");
  constexpr int NK = 4 * DB;                  // k-steps per site
  constexpr int SSQ = sweep_small_queue<DB, P>();
  static_assert(NK % SSQ == 0 && SSQ <= NK, "queue");
  const int lane = threadIdx.x;
  const int i16 = lane & 15, kg = lane >> 4;
  const int j = blockIdx.x, r = blockIdx.y;
  const int D = a.D;
  void* const* tp = a.ptrs + (size_t)r * a.n_tensors;
  const int row = SWR * j + i16;              // this lane's input
  const bool row_ok = row < a.M;              // the last block of a batch that is not a multiple of 16: its other rows stay zero

  // the chain's input, normalised by its producer's mean (the lazy rescale: reference einsum.py:387 on the step before)
  float st[DB][4];
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
    const float nI = (float)pv;
    const float inv = (a.partIn && nI > (float)a.min_norm) ? 1.0f / (nI / (float)a.numelIn) : 1.0f;
    const float* __restrict__ Ein = (const float*)tp[a.idIn] + (int64_t)row * a.ldIn;
#pragma unroll
    for (int G = 0; G < DB; ++G) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (row_ok && 16 * G + 4 * kg < D) v = *reinterpret_cast<const float4*>(Ein + 16 * G + 4 * kg);
      st[G][0] = v.x * inv; st[G][1] = v.y * inv; st[G][2] = v.z * inv; st[G][3] = v.w * inv;
    }
  }

  // a lane's own offsets into a core (bytes): its column of every (p, r-block) in row 0 of a group of l, and its own row
  // 4 kg of the group.  k-step u = 4 G + t reads row 16 G + 4 kg + t.  Nothing of W at or beyond D is used, and every
  // request is in bounds WITHOUT a branch (a conditional load makes the compiler wait for each request where it is made):
  // only the last r-block can hold columns past D - such a lane reads column 0 - and only the last group rows past D -
  // such a lane reads row 16 G + t, which is < D because D > 16 (DB - 1) is a multiple of 4 -, and what they read is
  // cleared by an AND with an all-zero mask
  const bool c_ok = 16 * (DB - 1) + i16 < D;
  uint32_t cmask = c_ok ? ~0u : 0u;
  uint32_t voff[P][DB];
#pragma unroll
  for (int p = 0; p < P; ++p)
#pragma unroll
    for (int q = 0; q < DB; ++q) voff[p][q] = (uint32_t)(((int64_t)p * a.ldWp + (q < DB - 1 || c_ok ? 16 * q + i16 : 0)) * 4);
  const uint32_t kgoff = (uint32_t)((int64_t)(4 * kg) * a.ldWl * 4);
  uint32_t lmask[4], lko[4];                  // the last group's four k-steps
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const bool l_ok = 16 * (DB - 1) + 4 * kg + t < D;
    lmask[t] = l_ok ? ~0u : 0u;
    lko[t] = l_ok ? kgoff : 0u;
    asm volatile("" : "+v"(lmask[t]));        // (opaque: the masks stay masks, the loads unconditional)
  }
  asm volatile("" : "+v"(cmask));
  const int64_t stepW = a.ldWl * 4;           // next row of l (bytes)

  sw_gptr Wcur = (sw_gptr)tp[a.site_ids[0]];
  sw_gptr Xcur = (sw_gptr)tp[a.site_ids[1]];
  float wq[SSQ][P][DB];
  auto wrequest = [&](float (&dst)[P][DB], sw_gptr core, int u) {     // k-step u of `core` (u a compile-time value)
    const bool last_g = (u >> 2) == DB - 1;
    const uint32_t ko = last_g ? lko[u & 3] : kgoff;
    sw_gptr from = core + (int64_t)(16 * (u >> 2) + (u & 3)) * stepW;      // (wave-uniform)
#pragma unroll
    for (int p = 0; p < P; ++p)
#pragma unroll
      for (int q = 0; q < DB; ++q) {
        uint32_t v = *reinterpret_cast<const __attribute__((address_space(1))) uint32_t*>(from + (voff[p][q] + ko));
        if (last_g) v &= lmask[u & 3];
        if (q == DB - 1) v &= cmask;
        dst[p][q] = __uint_as_float(v);
      }
  };
#pragma unroll
  for (int u = 0; u < SSQ; ++u) wrequest(wq[u], Wcur, u);

  // a block's record of site s: the abs-sums of C and E' (each lane's own share, then over the lanes by shuffles in a
  // fixed order) and the exponent it applies.  Only the NEXT site's epilogue needs the exponent, so the six shuffle levels of
  // site s are spread over the k-steps of site s + 1, behind its MFMAs; after the last site they are done at once.
  auto record = [&](int s, double totC, double totE, float inv_before, bool last) {
    int ex = 0;                               // an all-zero (or non-finite) block keeps its scale: the exponent stays finite
    if (!last && totE > 0.0 && totE < INFINITY) ex = max(-kSweepSmallMaxExp, min(kSweepSmallMaxExp, ilogb(totE / (double)(SWR * D))));
    if (lane == 0) {
      if (TWO) {
        const size_t ra = ((size_t)r * 2 * a.S + 2 * s) * a.J + j;
        a.rec_a[ra] = totC * (double)inv_before;   // C = (state) . W_s at the scale of the site before: the state's own 2^-e
        a.rec_a[ra + a.J] = totE;
      } else {
        a.rec_a[((size_t)r * a.S + s) * a.J + j] = totE;
      }
      a.rec_e[((size_t)r * a.S + s) * a.J + j] = ex;
    }
    return ex;
  };
  float inv_s = 1.0f;                         // 2^-e of the site before: the state in registers is the un-rescaled one
  double pendC = 0.0, pendE = 0.0;            // the site before: this lane's share of its abs-sums, being summed over the lanes
  sw_gptr Wnext = Wcur, Xnext = Xcur;
  for (int s = 0; s < a.S; ++s) {
    const bool last = s + 1 == a.S;
    // next site's tensors (the last site re-requests its own first k-steps: in bounds, never used)
    const int sn = last ? s : s + 1;
    Wnext = (sw_gptr)tp[a.site_ids[2 * sn]];
    Xnext = (sw_gptr)tp[a.site_ids[2 * sn + 1]];
    float xr[P];                               // the input's weights of this site
    {
      sw_gptr xp = Xcur + (int64_t)min(row, a.M - 1) * a.ldX * 4;
#pragma unroll
      for (int p = 0; p < P; ++p) xr[p] = *reinterpret_cast<const __attribute__((address_space(1))) float*>(xp + 4 * p);
    }
    f32x4 acc[P][DB];
#pragma unroll
    for (int p = 0; p < P; ++p)
#pragma unroll
      for (int q = 0; q < DB; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[p][q][e] = 0.f;
#pragma unroll
    for (int u = 0; u < NK; ++u) {
#pragma unroll
      for (int p = 0; p < P; ++p)
#pragma unroll
        for (int q = 0; q < DB; ++q)
          acc[p][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(wq[u % SSQ][p][q], st[u >> 2][u & 3], acc[p][q], 0, 0, 0);
      if (u + SSQ < NK) wrequest(wq[u % SSQ], Wcur, u + SSQ);
      else wrequest(wq[u % SSQ], Wnext, u + SSQ - NK);
#pragma unroll
      for (int lv = 0; lv < 6; ++lv)           // (site 0: sums of zeros)
        if (lv * NK / 6 == u) {
          if (TWO) pendC += __shfl_xor(pendC, 32 >> lv, 64);
          pendE += __shfl_xor(pendE, 32 >> lv, 64);
        }
    }
    if (s > 0) {
      const int ex = record(s - 1, pendC, pendE, inv_s, false);   // (inv_s: still the one site s - 1 worked with)
      inv_s = ldexpf(1.0f, -ex);
    }
    // ---- the site's epilogue.  A lane has C[b = i16][p][16 q + 4 kg + e]: the complete sum over l.  The state is the
    // un-rescaled one: its scale 2^-e goes into the weights (exact)
    float xs[P];
#pragma unroll
    for (int p = 0; p < P; ++p) xs[p] = (row_ok ? xr[p] : 0.f) * inv_s;
    float asumC = 0.f, asumE = 0.f;
#pragma unroll
    for (int q = 0; q < DB; ++q) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float v = xs[0] * acc[0][q][e];
        float ac = fabsf(acc[0][q][e]);
#pragma unroll
        for (int p = 1; p < P; ++p) {
          v = fmaf(xs[p], acc[p][q][e], v);
          ac += fabsf(acc[p][q][e]);
        }
        st[q][e] = v;
        if (TWO) asumC += ac;
        asumE += fabsf(v);
      }
      if (last) {   // the last site's rows leave with this block's own scale (k_sweep64_finish brings them to the common one)
        if (row_ok && 16 * q + 4 * kg < D) {
          sw_gout og = (sw_gout)tp[a.idOut] + (int64_t)row * a.ldOut + 16 * q + 4 * kg;
          *reinterpret_cast<__attribute__((address_space(1))) f32x4*>(og) = f32x4{st[q][0], st[q][1], st[q][2], st[q][3]};
        }
      }
    }
    pendC = (double)asumC; pendE = (double)asumE;
    Wcur = Wnext;
    Xcur = Xnext;
  }
#pragma unroll
  for (int of = 32; of > 0; of >>= 1) {
    if (TWO) pendC += __shfl_xor(pendC, of, 64);
    pendE += __shfl_xor(pendE, of, 64);
  }
  record(a.S - 1, pendC, pendE, inv_s, true);
}

}  // namespace ctn
