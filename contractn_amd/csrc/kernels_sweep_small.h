// kernels_sweep_small.h - the batched-MPS sweep of kernels_sweep.h at small bonds (8 ... 64), float32 and float64: every
// site of the chain inside ONE launch, ONE WAVE per block of 16 inputs, the state in registers from the first site to the
// last.  Part of the gfx950 contraction engine (see engine.hip).
#pragma once
#include "kernels_sweep_f64.h"

namespace ctn {

// ---------------------------------------------------------------------------
// K-sweep-small.  Per site, as in kernels_sweep.h,
//
//     C[b, (p, r)] = sum_l E[b, l] W_s[l, p, r]        E'[b, r] = sum_p x_s[b, p] C[b, (p, r)]
//
// for bonds D = 8 ... 64 (a multiple of 4), where the planner either keeps a site as TWO launched steps (a GEMM and the
// streaming sum over p, both reporting a rescale factor: the one shape of a float64 plan - plan.cpp fuses the pair for
// fp32 only) or, in float32 from B D P >= 65536 on, as one epilogue-summed step behind an absorbed marker.
// <T, DB, P, TWO>: float (v_mfma_f32_16x16x4_f32) or double (v_mfma_f64_16x16x4_f64), DB = ceil(D / 16) blocks of 16
// values of l and of r, the physical dimension, and which of the two plan shapes the records are for (double: TWO only).
// C exists in accumulators only.
//
// How the state gets from accumulator to operand.  Both instructions compute D[i = r][j = b] from
//   A (16 x 4):  lane (i = lane & 15, kg = lane >> 4) holds A[i][k = kg] - ONE value per lane and k-step;
//   B (4 x 16):  lane (j = lane & 15, kg = lane >> 4) holds B[k = kg][j];
//   D (16 x 16): lane (j = lane & 15, h = lane >> 4) holds four rows i in registers e = 0 .. 3,
// with j = b, the A operand W_s[l][p][16 q + i] of the r-block q and the B operand E[b][l].  A k-step contracts 4 values
// of l, one per lane group kg; a group G of 16 values of l is four k-steps t.  After the sum over p, register e of
// acc[.][q] in lane (b, h) is E' of that lane's row - and it is the B operand of k-step t = e of group G = q of the NEXT
// site in lane (b, kg = h) exactly if that k-step gives lane group kg the value of l which is that row.  The two
// instructions lay D out differently, so the pairing of (kg, t) with l differs:
//                 D: register e of lane (b, h) is row    k-step t of group G pairs lane group kg with    16 lanes of a group read of W_s
//   float32       i = 4 h + e                            l = 16 G + 4 kg + t  (as kernels_sweep.h)       64 consecutive bytes of row l
//   float64       i = h + 4 e                            l = 16 G + 4 t + kg                             128 consecutive bytes of row l,
//                 (kernels_sweep_f64.h: "lane (b, h = lane >> 4) holds row i = h + 4 e in register e", which is why its     the four groups four
//                 columns are r = rb + 2 h + 8 e + c; kernels_zip_f64.h stores its E' rows by the same rule)                consecutive rows
// (The float32 pairing used in float64 would contract E'[b][16 G + kg + 4 t] against W_s[16 G + 4 kg + t]: a transposition
// of each group's 4 x 4 values of l.)  So the state goes from accumulator to operand with no LDS, no barrier and no lane
// movement, for the whole chain; a wave shares nothing with any other wave, so a workgroup is ONE wave (a batch of 256
// inputs spreads over 16 CUs, not 4) and the kernel has no LDS, no barrier and no atomics at all.
// The first site's state: float32 E[b][16 G + 4 kg + 0 .. 3], one 16-byte load per group; float64 E[b][16 G + 4 e + kg],
// four 8-byte loads per group with a stride of 4 doubles, not one wide load; the last site's stores are 16-byte and 8-byte
// for the same reason.  Both happen once per chain.
//
// The A operand: direct 4-byte / 8-byte loads (a core is 1 ... 64 KiB, float64 ... 128 KiB, and the same for every wave:
// L1 / L2 hits), requested SSQ = 4 to 8 k-steps ahead into a register queue that runs on across site boundaries, as in
// k_sweep_f32.  This is the variant that was measured (ahead of the per-site launches at all six shapes
// of tools/sweep_small_timing.py).  The other candidate, a workgroup of several waves staging W_s in LDS behind one barrier
// per site, was NOT built and not measured, in either type: it ties the waves of a workgroup together, where the point of
// this form is that a block of rows waits for nobody.  (A workgroup is one wave, not several, and W is zero-filled per
// element, not per float4: D % 4 == 0 would allow either.)
// Ragged D: every request is unconditional and in bounds.  What a lane would read of W at or beyond D (l >= D or r >= D) is
// read from an in-bounds element instead and cleared by an AND mask on the 32-bit / 64-bit value - per element and without
// a branch -, so the padded entries of C and of the state are exact zeros on their own; the state's padded columns are
// never loaded from E and never stored.  A lane whose column 16 (DB - 1) + i is at or beyond D reads column 0.  Rows of l:
// in float32 a k-step of the last group is valid per lane (16 (DB - 1) + 4 kg + t < D), and a lane for which it is not
// reads row 16 (DB - 1) + t; in float64 D is a multiple of 4, so it is valid or not for ALL four lane groups at once
// (16 (DB - 1) + 4 t < D), and an invalid one reads the group's rows 16 (DB - 1) + kg instead.  Rows of a block past M:
// their state and weights are zero, never stored.  Means use numel = 16 D.
//
// Transposed cores, <.., TR = true>.  The same MPS walked from its other end (the boundary vector on the right, cores stored
// (r, p, l) or (p, r, l)): the bond a core contracts with the state is its unit-stride axis, W_s[r][p][l] with r at the stride
// ldWl.  TR = false is the text described above, instruction for instruction; TR = true changes only how the A operand is
// fetched - lane (i, kg) needs W_s[16 q + i][p][l] with l from the pairing:
//   float32   l = 16 G + 4 kg + t, t = 0 .. 3 consecutive in memory: ONE 16-byte request per (G, p, q) delivers all four k-steps
//             of a group, so the queue holds whole groups (sweep_small_queue_tr) and the site's loop runs a group at a time,
//             (p, q) by (p, q) - the four MFMAs of an entry free it, and it is requested again at once for SG groups on;
//   float64   l = 16 G + 4 t + kg: 8-byte requests, one per k-step, the four lane groups reading 32 consecutive bytes of a
//             row; queue and loop are the forward ones, only the lane's offsets and the step between k-steps differ.
// Ragged D as above: a row 16 (DB - 1) + i >= D of r reads row 0; in float32 a lane's four l of the last group are valid or
// not as a whole (D % 4 == 0) and an invalid lane reads the group's first four; in float64 a k-step is valid or not for all
// lanes and an invalid one reads l = 16 (DB - 1) + kg; all cleared by the AND masks.  Every accumulator meets the same
// operand values in the same order u = 0 .. 4 DB - 1 as the forward kernel on the cores stored the other way round, and from
// the MFMAs on nothing differs: the same bits (rec_a, rec_e, every factor).  The 16-byte requests rest on what the 16-byte
// loads of a network-input E rest on: the engine refuses operand pointers that are not 16-byte aligned, and ldWl, ldWp are
// multiples of 4.  Remarks and measurement: DESIGN sections 4, 10 and 11 (3d).
//
// Registers, float64 (a lone wave has 512: 256 VGPR + 256 AGPR, and MFMA accumulators may sit in AGPRs): state 8 DB,
// accumulators 8 P DB, queue 2 SSQ P DB, plus 16-odd of offsets and masks: <4, 4> 32 + 128 + 128.  Float32 needs half of
// each.  The compiler's remarks for all 24 instantiations are in DESIGN section 4: no scratch, no spills, the same queue
// (sweep_small_queue) in both types and one pass over l.
//
// Stabilisation: k_sweep_f64's protocol (kernels_sweep_f64.h), in float or unchanged.  A block rescales its rows by 2^e,
// e = ilogb(mean |E'|), folded into the next site's weights x_s exactly, |e| <= kSweepSmallMaxExp / kSweep64MaxExp; per
// (replica, site, block) the kernel records e in rec_e and in rec_a the abs-sum of E' and - TWO - of C, both at the block's
// scale g[j][s - 1]; the abs-sums are sums over a lane's registers in a fixed order (4 P DB values of C, 4 DB of E'), then
// over the lanes by six shuffle levels - spread over the NEXT site's k-steps, behind its MFMAs: only that site's epilogue
// needs e -: no barrier, no atomics, the same bits every run.  k_sweep64_z<TWO> and k_sweep64_finish<T, TWO> rebuild the
// reference's per-step rescale factors from the records.  !TWO: one entry per site (the member step); the absorbed marker
// has no entry and reports 0.
//
// Conditions (fused_forms.h, sweep_small_match): fp32 or fp64, 8 <= |l| = |r| <= 64 a multiple of 4, |p| = 2 or 4, W_s and
// x_s network inputs with r (TR: l) and p unit-stride, E row-major, ldIn, ldOut, ldWl, ldWp multiples of 4 in float32 (16-byte
// accesses of the state's rows), even in float64.
// ---------------------------------------------------------------------------
struct SweepSmallArgs {
  void* const* ptrs;         // [R][n_tensors]
  int32_t n_tensors;
  const int32_t* site_ids;   // [S][2]: tensor ids of (W_s, x_s)
  int32_t idIn, idOut;       // the chain's input E [b][l] and its output E' [b][r]
  int32_t S, J, M, D;        // sites, row blocks (ceil(rows / 16)), rows, bond dimension
  int64_t ldIn, ldOut;       // row strides of input and output (elements)
  int64_t ldWl, ldWp;        // W_s[l][p][r]: strides of l and p (r unit-stride); <TR>: of r and p (l unit-stride)
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

// per element type: the bits of a value of W (the AND masks), a tile of accumulators, |e| of one site at most
template <typename T> struct SweepSmallType;
template <> struct SweepSmallType<float> { typedef uint32_t bits; typedef f32x4 acc; static constexpr int max_exp = kSweepSmallMaxExp; };
template <> struct SweepSmallType<double> { typedef uint64_t bits; typedef f64x4 acc; static constexpr int max_exp = kSweep64MaxExp; };

// Transposed cores, float32: whole GROUPS of W in flight per wave (a 16-byte request is a group's four k-steps of one
// (p, r-block)): a divisor of the DB groups of a site, one group where its 4 P DB MFMAs x 32 cycles cover an L2 hit (or
// DB = 1 leaves no other divisor), else all DB - 64 registers (<4, 4>), 72 (<3, 2>) at the most
template <int DB, int P>
constexpr int sweep_small_queue_tr() { return P * DB >= 8 || DB == 1 ? 1 : DB; }

typedef uint32_t sws_u32x4 __attribute__((ext_vector_type(4)));
// one 16-byte request of a transposed float32 core: the lane's four values of l of a group (`from`: the core at the group's
// first l, wave-uniform; `off`: the lane's own bytes), cleared where the group or the lane's row lies past D
__device__ __forceinline__ f32x4 sweep_small_group(sw_gptr from, uint32_t off, uint32_t lmask, uint32_t cmask, bool last_g, bool last_q) {
  sws_u32x4 v = *reinterpret_cast<const __attribute__((address_space(1))) sws_u32x4*>(from + off);
  if (last_g) v &= lmask;
  if (last_q) v &= cmask;
  return __builtin_bit_cast(f32x4, v);
}

template <typename T, int DB, int P, bool TWO, bool TR = false>
__global__ __launch_bounds__(64) void k_sweep_small(SweepSmallArgs a) {
  static_assert(DB >= 1 && DB <= 4 && (P == 2 || P == 4), "shape");
  constexpr bool F32 = sizeof(T) == 4;
  static_assert(F32 || TWO, "a float64 plan has two-step sites only");
  typedef typename SweepSmallType<T>::bits bits_t;
  constexpr int ES = sizeof(T);               // bytes per element
  constexpr int NK = 4 * DB;                  // k-steps per site
  constexpr int SSQ = sweep_small_queue<DB, P>();
  static_assert(NK % SSQ == 0 && SSQ <= NK, "queue");
  constexpr bool TRG = TR && F32;             // the queue holds groups (16-byte requests), not k-steps
  constexpr int SG = sweep_small_queue_tr<DB, P>();
  static_assert(DB % SG == 0, "queue of groups");
  const int lane = threadIdx.x;
  const int i16 = lane & 15, kg = lane >> 4;
  const int j = blockIdx.x, r = blockIdx.y;
  const int D = a.D;
  void* const* tp = a.ptrs + (size_t)r * a.n_tensors;
  const int row = SWR * j + i16;              // this lane's input
  const bool row_ok = row < a.M;              // the last block of a batch that is not a multiple of 16: its other rows stay zero

  // the chain's input, normalised by its producer's mean (the lazy rescale: reference einsum.py:387 on the step before):
  // register e of group G is E[b][16 G + 4 kg + e] (float32) or E[b][16 G + 4 e + kg] (float64)
  T st[DB][4];
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
    const T nI = (T)pv;
    const T inv = (a.partIn && nI > (T)a.min_norm) ? (T)1 / (nI / (T)a.numelIn) : (T)1;
    const T* __restrict__ Ein = (const T*)tp[a.idIn] + (int64_t)row * a.ldIn;
#pragma unroll
    for (int G = 0; G < DB; ++G) {
      if constexpr (F32) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row_ok && 16 * G + 4 * kg < D) v = *reinterpret_cast<const float4*>(Ein + 16 * G + 4 * kg);
        st[G][0] = v.x * inv; st[G][1] = v.y * inv; st[G][2] = v.z * inv; st[G][3] = v.w * inv;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          double v = 0.0;
          if (row_ok && 16 * G + 4 * e < D) v = Ein[16 * G + 4 * e + kg];   // (D % 4 == 0: the four lane groups together)
          st[G][e] = v * inv;
        }
      }
    }
  }

  // a lane's own offsets into a core (bytes): its column of every (p, r-block) in row 0 of a group of l, and its own row of
  // the group - float32: row 4 kg, k-step u = 4 G + t reads row 16 G + 4 kg + t; float64: row kg of a k-step's four,
  // k-step u = 4 G + e reads rows 16 G + 4 e + kg.  Nothing of W at or beyond D is used, and every request is in bounds
  // WITHOUT a branch (a conditional load makes the compiler wait for each request where it is made): only the last r-block
  // can hold columns past D - such a lane reads column 0 - and only the last group rows past D - such a lane reads row
  // 16 G + t (float32), such a k-step rows 16 G + kg (float64), which are < D because D > 16 (DB - 1) is a multiple of 4 -,
  // and what they read is cleared by an AND with an all-zero mask
  const bool c_ok = 16 * (DB - 1) + i16 < D;
  bits_t cmask = c_ok ? ~(bits_t)0 : (bits_t)0;
  uint32_t voff[P][DB];
#pragma unroll
  for (int p = 0; p < P; ++p)
#pragma unroll
    for (int q = 0; q < DB; ++q) {
      if constexpr (TR) {
        // transposed cores W_s[r][p][l], l unit-stride: the lane's ROW 16 q + i16 of r (stride ldWl) of every (p, r-block) -
        // a row at or beyond D reads row 0 - and, float64, its position kg among a k-step's four values of l
        const int64_t at = (int64_t)p * a.ldWp + (int64_t)(q < DB - 1 || c_ok ? 16 * q + i16 : 0) * a.ldWl;
        voff[p][q] = F32 ? (uint32_t)(at * 4) : (uint32_t)((at + kg) * 8);
      } else if constexpr (F32) voff[p][q] = (uint32_t)(((int64_t)p * a.ldWp + (q < DB - 1 || c_ok ? 16 * q + i16 : 0)) * 4);
      else voff[p][q] = (uint32_t)(((int64_t)p * a.ldWp + (q < DB - 1 || c_ok ? 16 * q + i16 : 0) + (int64_t)kg * a.ldWl) * 8);
    }
  bits_t lmask[4];                            // the last group's four k-steps (float64: the same in every lane)
  uint32_t kgoff, lko[4];                     // float32: the lane's row 4 kg of a group, and of the last group's k-steps
  int lrow[4];                                // float64: the first row of the last group's k-steps
  if constexpr (TRG) {
    // the lane's four values of l of a group, 16 G + 4 kg + 0 .. 3, are 16 consecutive bytes of its row: valid or not as a
    // whole in the last group (D % 4 == 0); an invalid lane reads the group's first four, which are < D
    kgoff = 16u * (uint32_t)kg;
    const bool l_ok = 16 * (DB - 1) + 4 * kg < D;
    lmask[0] = l_ok ? ~0u : 0u;
    lko[0] = l_ok ? kgoff : 0u;
    asm volatile("" : "+v"(lmask[0]));
  } else if constexpr (F32) {
    kgoff = (uint32_t)((int64_t)(4 * kg) * a.ldWl * 4);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const bool l_ok = 16 * (DB - 1) + 4 * kg + t < D;
      lmask[t] = l_ok ? ~0u : 0u;
      lko[t] = l_ok ? kgoff : 0u;
      asm volatile("" : "+v"(lmask[t]));      // (opaque: the masks stay masks, the loads unconditional)
    }
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool l_ok = 16 * (DB - 1) + 4 * e < D;
      lmask[e] = l_ok ? ~0ull : 0ull;
      lrow[e] = l_ok ? 4 * e : 0;
      asm volatile("" : "+v"(lmask[e]));
    }
  }
  asm volatile("" : "+v"(cmask));
  const int64_t stepW = TR ? ES : a.ldWl * ES;   // next value of l (bytes): a row of the core, or - transposed - an element

  sw_gptr Wcur = (sw_gptr)tp[a.site_ids[0]];
  sw_gptr Xcur = (sw_gptr)tp[a.site_ids[1]];
  // (transposed float32: SG whole groups, component t of an entry is its k-step t)
  typename std::conditional<TRG, f32x4, T>::type wq[TRG ? SG : SSQ][P][DB];
  auto wrequest = [&](T (&dst)[P][DB], sw_gptr core, int u) {     // k-step u of `core` (u a compile-time value)
    const bool last_g = (u >> 2) == DB - 1;
    uint32_t ko = 0;                          // (float64: the lane's row is in voff)
    sw_gptr from;                             // (wave-uniform)
    if constexpr (F32) {
      ko = last_g ? lko[u & 3] : kgoff;
      from = core + (int64_t)(16 * (u >> 2) + (u & 3)) * stepW;
    } else {
      from = core + (int64_t)(16 * (u >> 2) + (last_g ? lrow[u & 3] : 4 * (u & 3))) * stepW;
    }
#pragma unroll
    for (int p = 0; p < P; ++p)
#pragma unroll
      for (int q = 0; q < DB; ++q) {
        bits_t v = *reinterpret_cast<const __attribute__((address_space(1))) bits_t*>(from + (voff[p][q] + ko));
        if (last_g) v &= lmask[u & 3];
        if (q == DB - 1) v &= cmask;
        dst[p][q] = __builtin_bit_cast(T, v);
      }
  };
  if constexpr (TRG) {
#pragma unroll
    for (int G = 0; G < SG; ++G)
#pragma unroll
      for (int p = 0; p < P; ++p)
#pragma unroll
        for (int q = 0; q < DB; ++q)
          wq[G][p][q] = sweep_small_group(Wcur + 64 * G, voff[p][q] + (G == DB - 1 ? lko[0] : kgoff), (uint32_t)lmask[0], (uint32_t)cmask, G == DB - 1, q == DB - 1);
  } else {
#pragma unroll
    for (int u = 0; u < SSQ; ++u) wrequest(wq[u], Wcur, u);
  }

  // a block's record of site s: the abs-sums of C and E' (each lane's own share, then over the lanes by shuffles in a
  // fixed order) and the exponent it applies.  Only the NEXT site's epilogue needs the exponent, so the six shuffle levels of
  // site s are spread over the k-steps of site s + 1, behind its MFMAs; after the last site they are done at once.
  auto record = [&](int s, double totC, double totE, T inv_before, bool last) {
    constexpr int max_exp = SweepSmallType<T>::max_exp;
    int ex = 0;                               // an all-zero (or non-finite) block keeps its scale: the exponent stays finite
    if (!last && totE > 0.0 && totE < INFINITY) ex = max(-max_exp, min(max_exp, ilogb(totE / (double)(SWR * D))));
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
  T inv_s = 1;                                // 2^-e of the site before: the state in registers is the un-rescaled one
  double pendC = 0.0, pendE = 0.0;            // the site before: this lane's share of its abs-sums, being summed over the lanes
  sw_gptr Wnext = Wcur, Xnext = Xcur;
  for (int s = 0; s < a.S; ++s) {
    const bool last = s + 1 == a.S;
    // next site's tensors (the last site re-requests its own first k-steps: in bounds, never used)
    const int sn = last ? s : s + 1;
    Wnext = (sw_gptr)tp[a.site_ids[2 * sn]];
    Xnext = (sw_gptr)tp[a.site_ids[2 * sn + 1]];
    T xr[P];                                   // the input's weights of this site
    {
      sw_gptr xp = Xcur + (int64_t)min(row, a.M - 1) * a.ldX * ES;
#pragma unroll
      for (int p = 0; p < P; ++p) xr[p] = *reinterpret_cast<const __attribute__((address_space(1))) T*>(xp + ES * p);
    }
    typename SweepSmallType<T>::acc acc[P][DB];
#pragma unroll
    for (int p = 0; p < P; ++p)
#pragma unroll
      for (int q = 0; q < DB; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[p][q][e] = 0;
    if constexpr (TRG) {
      // a group at a time: the four k-steps of one (p, r-block) free its entry of the queue, which is requested again at
      // once for SG groups on - every accumulator still meets its k-steps in the order u = 0 .. NK - 1
#pragma unroll
      for (int G = 0; G < DB; ++G) {
#pragma unroll
        for (int p = 0; p < P; ++p)
#pragma unroll
          for (int q = 0; q < DB; ++q) {
#pragma unroll
            for (int t = 0; t < 4; ++t)
              acc[p][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(wq[G % SG][p][q][t], st[G][t], acc[p][q], 0, 0, 0);
            const int Gn = (G + SG) % DB;         // the group SG on: of this core, or of the next site's
            wq[G % SG][p][q] = sweep_small_group((G + SG < DB ? Wcur : Wnext) + 64 * Gn, voff[p][q] + (Gn == DB - 1 ? lko[0] : kgoff),
                                                 (uint32_t)lmask[0], (uint32_t)cmask, Gn == DB - 1, q == DB - 1);
          }
#pragma unroll
        for (int lv = 0; lv < 6; ++lv)         // (the levels that the k-steps of this group carry in the forward kernel)
          if (lv * NK / 6 >= 4 * G && lv * NK / 6 < 4 * G + 4) {
            if (TWO) pendC += __shfl_xor(pendC, 32 >> lv, 64);
            pendE += __shfl_xor(pendE, 32 >> lv, 64);
          }
      }
    } else {
#pragma unroll
    for (int u = 0; u < NK; ++u) {
#pragma unroll
      for (int p = 0; p < P; ++p)
#pragma unroll
        for (int q = 0; q < DB; ++q) {
          if constexpr (F32) acc[p][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(wq[u % SSQ][p][q], st[u >> 2][u & 3], acc[p][q], 0, 0, 0);
          else acc[p][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(wq[u % SSQ][p][q], st[u >> 2][u & 3], acc[p][q], 0, 0, 0);
        }
      if (u + SSQ < NK) wrequest(wq[u % SSQ], Wcur, u + SSQ);
      else wrequest(wq[u % SSQ], Wnext, u + SSQ - NK);
#pragma unroll
      for (int lv = 0; lv < 6; ++lv)           // (site 0: sums of zeros)
        if (lv * NK / 6 == u) {
          if (TWO) pendC += __shfl_xor(pendC, 32 >> lv, 64);
          pendE += __shfl_xor(pendE, 32 >> lv, 64);
        }
    }
    }
    if (s > 0) {
      const int ex = record(s - 1, pendC, pendE, inv_s, false);   // (inv_s: still the one site s - 1 worked with)
      inv_s = std::ldexp((T)1, -ex);
    }
    // ---- the site's epilogue.  A lane has the complete sum over l of C[b = i16][p][16 q + 4 kg + e] (float32) or of
    // C[b = i16][p][16 q + kg + 4 e] (float64).  The state is the un-rescaled one: its scale 2^-e goes into the weights (exact)
    T xs[P];
#pragma unroll
    for (int p = 0; p < P; ++p) xs[p] = (row_ok ? xr[p] : (T)0) * inv_s;
    T asumC = 0, asumE = 0;
#pragma unroll
    for (int q = 0; q < DB; ++q) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        T v = xs[0] * acc[0][q][e];
        T ac = std::fabs(acc[0][q][e]);
#pragma unroll
        for (int p = 1; p < P; ++p) {
          v = std::fma(xs[p], acc[p][q][e], v);
          ac += std::fabs(acc[p][q][e]);
        }
        st[q][e] = v;
        if (TWO) asumC += ac;
        asumE += std::fabs(v);
        // the last site's rows leave with this block's own scale (k_sweep64_finish brings them to the common one)
        if constexpr (!F32) {
          if (last) {
            if (row_ok && 16 * q + 4 * e < D) {
              sw_gout64 og = (sw_gout64)tp[a.idOut] + (int64_t)row * a.ldOut + 16 * q + 4 * e + kg;
              *og = v;
            }
          }
        }
      }
      if constexpr (F32) {
        if (last) {
          if (row_ok && 16 * q + 4 * kg < D) {
            sw_gout og = (sw_gout)tp[a.idOut] + (int64_t)row * a.ldOut + 16 * q + 4 * kg;
            *reinterpret_cast<__attribute__((address_space(1))) f32x4*>(og) = f32x4{st[q][0], st[q][1], st[q][2], st[q][3]};
          }
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
