// kernels_sweep_small_f64.h - the small-bond batched-MPS sweep of kernels_sweep_small.h in float64 (bonds 8 ... 64): every
// site of the chain inside ONE launch, ONE WAVE per block of 16 inputs, the state in registers from the first site to the
// last, v_mfma_f64_16x16x4_f64.  Part of the gfx950 contraction engine (see engine.hip).
#pragma once
#include "kernels_sweep_small.h"

namespace ctn {

// ---------------------------------------------------------------------------
// K-sweep-small-f64.  Per site, as in kernels_sweep_small.h,
//
//     C[b, (p, r)] = sum_l E[b, l] W_s[l, p, r]        E'[b, r] = sum_p x_s[b, p] C[b, (p, r)]
//
// for bonds D = 8 ... 64 (a multiple of 4) of a float64 plan, which keeps a site as TWO launched steps (a GEMM and the
// streaming sum over p, both reporting a rescale factor: plan.cpp fuses the pair for fp32 only) - the one record shape here.
// <DB, P>: DB = ceil(D / 16) blocks of 16 values of l and of r, and the physical dimension.  C exists in accumulators only.
//
// How the state gets from accumulator to operand on v_mfma_f64_16x16x4_f64, D[i = r][j = b].  The instruction's operand
// layout, as kernels_zip_f64.h and kernels_sweep_f64.h use it:
//   A (16 x 4):  lane (i = lane & 15, kg = lane >> 4) holds A[i][k = kg] - ONE double per lane and k-step;
//   B (4 x 16):  lane (j = lane & 15, kg = lane >> 4) holds B[k = kg][j];
//   D (16 x 16): lane (j = lane & 15, h = lane >> 4) holds row i = h + 4 e in register e = 0 .. 3
//                (kernels_sweep_f64.h: "lane (b, h = lane >> 4) holds row i = h + 4 e in register e", which is why its columns
//                are r = rb + 2 h + 8 e + c; kernels_zip_f64.h stores its E' rows by the same rule).
// With j = b and the r-block q, register e of acc[.][q] in lane (b, h) is row r = 16 q + h + 4 e: after the sum over p it
// is E'[b][16 q + h + 4 e].  A k-step contracts 4 values of l, one per lane group kg, so that register is the B operand
// B[k = kg][j = b] of a k-step of the NEXT site exactly if that k-step gives lane group kg = h the value
// l = 16 q + 4 e + kg: k-step e of group G = q pairs lane group kg with l = 16 G + 4 e + kg.  (float32,
// kernels_sweep_small.h: its D layout is row i = 4 h + e, so its pairing is 16 G + 4 kg + t.  Used here, the float32
// pairing would contract E'[b][16 G + kg + 4 t] against W_s[16 G + 4 kg + t]: a transposition of each group's 4 x 4
// values of l.)  The A operand of that k-step is W_s[16 G + 4 e + kg][p][16 q' + i] in lane (i, kg): the 16 lanes of a group read
// 128 consecutive bytes of row 16 G + 4 e + kg, and the four groups four consecutive rows.  So the state goes from accumulator
// to operand with no LDS, no barrier and no lane movement for the whole chain; a wave shares nothing with any other wave,
// a workgroup is ONE wave, and the kernel has no LDS, no barrier and no atomics.
// The first site's state is E[b][16 G + 4 e + kg]: four 8-byte loads per group with a stride of 4 doubles, not one wide
// load; the last site's stores are 8-byte for the same reason.  Both happen once per chain.
//
// Everything else follows k_sweep_small_f32.  The A operand: direct 8-byte loads (a core is 1 ... 128 KiB and the same
// for every wave: L1 / L2 hits), requested SSQ k-steps ahead into a register queue that runs on across site boundaries.
// Every request is unconditional and in bounds.  Ragged D: D is a multiple of 4, so a k-step of the last group is valid or
// not for ALL four lane groups at once (16 (DB - 1) + 4 e < D); an invalid one reads the group's rows 16 (DB - 1) + kg
// instead (< D) and is cleared by an AND mask on the 64-bit value; a lane whose column 16 (DB - 1) + i is at or beyond D
// reads column 0 and is cleared the same way - without a branch, so the padded entries of C and of the state are exact
// zeros on their own; the state's padded columns are never loaded from E and never stored.  Rows of a block past M: their
// state and weights are zero, never stored.  Means use numel = 16 D.
// The LDS-staged variant (several waves per workgroup behind one barrier per site) was NOT built and not measured, as
// for float32.
//
// Registers (a lone wave has 512: 256 VGPR + 256 AGPR, and MFMA accumulators may sit in AGPRs): state 8 DB, accumulators
// 8 P DB, queue 2 SSQ P DB, plus 16-odd of offsets and masks: <4, 4> 32 + 128 + 128.  The compiler's remarks for all eight
// instantiations are in DESIGN section 4: no scratch, no spills, with the queue of k_sweep_small_f32 (sweep_small_queue)
// unchanged and one pass over l.
//
// Stabilisation: k_sweep_f64's protocol unchanged.  A block rescales its rows by 2^e, e = ilogb(mean |E'|), folded into
// the next site's weights x_s exactly, |e| <= kSweep64MaxExp; per (replica, site, block) rec_a holds the abs-sums of C and
// of E', both at the block's scale g[j][s - 1], and rec_e the exponent; the abs-sums are sums over a lane's registers in a
// fixed order (4 P DB values of C, 4 DB of E'), then over the lanes by six shuffle levels - spread over the NEXT site's
// k-steps, behind its MFMAs -: the same bits every run.  k_sweep64_z<true> and k_sweep64_finish<double, true> rebuild the
// reference's per-step rescale factors from the records, unchanged.
//
// Conditions (fused_forms.h, sweep_small_f64_match): fp64, 8 <= |l| = |r| <= 64 a multiple of 4, |p| = 2 or 4, W_s and x_s
// network inputs with r and p unit-stride, E row-major, ldIn, ldOut, ldWl, ldWp even.
// ---------------------------------------------------------------------------
template <int DB, int P>
__global__ __launch_bounds__(64) void k_sweep_small_f64(SweepSmallArgs a) {
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

  // the chain's input, normalised by its producer's mean (the lazy rescale: reference einsum.py:387 on the step before):
  // register e of group G is E[b][16 G + 4 e + kg]
  double st[DB][4];
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
    const double* __restrict__ Ein = (const double*)tp[a.idIn] + (int64_t)row * a.ldIn;
#pragma unroll
    for (int G = 0; G < DB; ++G)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        double v = 0.0;
        if (row_ok && 16 * G + 4 * e < D) v = Ein[16 * G + 4 * e + kg];   // (D % 4 == 0: the four lane groups together)
        st[G][e] = v * inv;
      }
  }

  // a lane's own offsets into a core (bytes): its column of every (p, r-block) in row 0 of a group of l, and its own row kg
  // of a k-step's four.  k-step u = 4 G + e reads rows 16 G + 4 e + kg.  Nothing of W at or beyond D is used, and every
  // request is in bounds WITHOUT a branch (a conditional load makes the compiler wait for each request where it is made):
  // only the last r-block can hold columns past D - such a lane reads column 0 - and only the last group rows past D - such
  // a k-step reads rows 16 (DB - 1) + kg, which are < D because D > 16 (DB - 1) is a multiple of 4 -, and what they read is
  // cleared by an AND with an all-zero mask
  const bool c_ok = 16 * (DB - 1) + i16 < D;
  uint64_t cmask = c_ok ? ~0ull : 0ull;
  uint32_t voff[P][DB];
#pragma unroll
  for (int p = 0; p < P; ++p)
#pragma unroll
    for (int q = 0; q < DB; ++q)
      voff[p][q] = (uint32_t)(((int64_t)p * a.ldWp + (q < DB - 1 || c_ok ? 16 * q + i16 : 0) + (int64_t)kg * a.ldWl) * 8);
  uint64_t lmask[4];                          // the last group's four k-steps (the same in every lane)
  int lrow[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const bool l_ok = 16 * (DB - 1) + 4 * e < D;
    lmask[e] = l_ok ? ~0ull : 0ull;
    lrow[e] = l_ok ? 4 * e : 0;
    asm volatile("" : "+v"(lmask[e]));        // (opaque: the masks stay masks, the loads unconditional)
  }
  asm volatile("" : "+v"(cmask));
  const int64_t stepW = a.ldWl * 8;           // next row of l (bytes)

  sw_gptr Wcur = (sw_gptr)tp[a.site_ids[0]];
  sw_gptr Xcur = (sw_gptr)tp[a.site_ids[1]];
  double wq[SSQ][P][DB];
  auto wrequest = [&](double (&dst)[P][DB], sw_gptr core, int u) {     // k-step u of `core` (u a compile-time value)
    const bool last_g = (u >> 2) == DB - 1;
    sw_gptr from = core + (int64_t)(16 * (u >> 2) + (last_g ? lrow[u & 3] : 4 * (u & 3))) * stepW;      // (wave-uniform)
#pragma unroll
    for (int p = 0; p < P; ++p)
#pragma unroll
      for (int q = 0; q < DB; ++q) {
        uint64_t v = *reinterpret_cast<const __attribute__((address_space(1))) uint64_t*>(from + voff[p][q]);
        if (last_g) v &= lmask[u & 3];
        if (q == DB - 1) v &= cmask;
        dst[p][q] = __longlong_as_double((long long)v);
      }
  };
#pragma unroll
  for (int u = 0; u < SSQ; ++u) wrequest(wq[u], Wcur, u);

  // a block's record of site s: the abs-sums of C and E' (each lane's own share, then over the lanes by shuffles in a
  // fixed order) and the exponent it applies.  Only the NEXT site's epilogue needs the exponent, so the six shuffle levels of
  // site s are spread over the k-steps of site s + 1, behind its MFMAs; after the last site they are done at once.
  auto record = [&](int s, double totC, double totE, double inv_before, bool last) {
    int ex = 0;                               // an all-zero (or non-finite) block keeps its scale: the exponent stays finite
    if (!last && totE > 0.0 && totE < INFINITY) ex = max(-kSweep64MaxExp, min(kSweep64MaxExp, ilogb(totE / (double)(SWR * D))));
    if (lane == 0) {
      const size_t ra = ((size_t)r * 2 * a.S + 2 * s) * a.J + j;
      a.rec_a[ra] = totC * inv_before;        // C = (state) . W_s at the scale of the site before: the state's own 2^-e
      a.rec_a[ra + a.J] = totE;
      a.rec_e[((size_t)r * a.S + s) * a.J + j] = ex;
    }
    return ex;
  };
  double inv_s = 1.0;                         // 2^-e of the site before: the state in registers is the un-rescaled one
  double pendC = 0.0, pendE = 0.0;            // the site before: this lane's share of its abs-sums, being summed over the lanes
  sw_gptr Wnext = Wcur, Xnext = Xcur;
  for (int s = 0; s < a.S; ++s) {
    const bool last = s + 1 == a.S;
    // next site's tensors (the last site re-requests its own first k-steps: in bounds, never used)
    const int sn = last ? s : s + 1;
    Wnext = (sw_gptr)tp[a.site_ids[2 * sn]];
    Xnext = (sw_gptr)tp[a.site_ids[2 * sn + 1]];
    double xr[P];                              // the input's weights of this site
    {
      sw_gptr xp = Xcur + (int64_t)min(row, a.M - 1) * a.ldX * 8;
#pragma unroll
      for (int p = 0; p < P; ++p) xr[p] = *reinterpret_cast<const __attribute__((address_space(1))) double*>(xp + 8 * p);
    }
    f64x4 acc[P][DB];
#pragma unroll
    for (int p = 0; p < P; ++p)
#pragma unroll
      for (int q = 0; q < DB; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[p][q][e] = 0.0;
#pragma unroll
    for (int u = 0; u < NK; ++u) {
#pragma unroll
      for (int p = 0; p < P; ++p)
#pragma unroll
        for (int q = 0; q < DB; ++q)
          acc[p][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(wq[u % SSQ][p][q], st[u >> 2][u & 3], acc[p][q], 0, 0, 0);
      if (u + SSQ < NK) wrequest(wq[u % SSQ], Wcur, u + SSQ);
      else wrequest(wq[u % SSQ], Wnext, u + SSQ - NK);
#pragma unroll
      for (int lv = 0; lv < 6; ++lv)           // (site 0: sums of zeros)
        if (lv * NK / 6 == u) {
          pendC += __shfl_xor(pendC, 32 >> lv, 64);
          pendE += __shfl_xor(pendE, 32 >> lv, 64);
        }
    }
    if (s > 0) {
      const int ex = record(s - 1, pendC, pendE, inv_s, false);   // (inv_s: still the one site s - 1 worked with)
      inv_s = ldexp(1.0, -ex);
    }
    // ---- the site's epilogue.  A lane has C[b = i16][p][16 q + kg + 4 e]: the complete sum over l.  The state is the
    // un-rescaled one: its scale 2^-e goes into the weights (exact)
    double xs[P];
#pragma unroll
    for (int p = 0; p < P; ++p) xs[p] = (row_ok ? xr[p] : 0.0) * inv_s;
    double asumC = 0.0, asumE = 0.0;
#pragma unroll
    for (int q = 0; q < DB; ++q) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        double v = xs[0] * acc[0][q][e];
        double ac = fabs(acc[0][q][e]);
#pragma unroll
        for (int p = 1; p < P; ++p) {
          v = fma(xs[p], acc[p][q][e], v);
          ac += fabs(acc[p][q][e]);
        }
        st[q][e] = v;
        asumC += ac;
        asumE += fabs(v);
        if (last) {   // the last site's rows leave with this block's own scale (k_sweep64_finish brings them to the common one)
          if (row_ok && 16 * q + 4 * e < D) {
            sw_gout64 og = (sw_gout64)tp[a.idOut] + (int64_t)row * a.ldOut + 16 * q + 4 * e + kg;
            *og = v;
          }
        }
      }
    }
    pendC = asumC; pendE = asumE;
    Wcur = Wnext;
    Xcur = Xnext;
  }
#pragma unroll
  for (int of = 32; of > 0; of >>= 1) {
    pendC += __shfl_xor(pendC, of, 64);
    pendE += __shfl_xor(pendE, of, 64);
  }
  record(a.S - 1, pendC, pendE, inv_s, true);
}

}  // namespace ctn
