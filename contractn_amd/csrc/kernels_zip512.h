// kernels_zip512.h - the fused zipper site pair of kernels_zip.h for bond 512: both GEMMs of a site as ONE launch, the
// intermediate kept in v_mfma_f32_16x16x4_f32 accumulators.  Part of the gfx950 contraction engine (see engine.hip).
#pragma once
#include "kernels_zip.h"

namespace ctn {

// ---------------------------------------------------------------------------
// K-zip512-f32.  The pair of kernels_zip.h,
//
//     T[m1, (q, u)] = sum_k1  E[k1, m1] * X[q, k1, u]          E'[u, n2] = sum_(m1, q)  T[m1, q, u] * Y[q, m1, n2]
//
// with |m1| = |n2| = 512, in fp32.  As two launches the 4 MiB T of a site (|u| = 512, Q = 4) is written and read again
// per network.  Here ONE workgroup owns 64 values of u and walks q: phase 1 forms Tq[m1, u-block] in accumulators,
// phase 2 multiplies those accumulators - used directly as MFMA operands - into E'[u-block, 0..511], and T never exists
// outside the register file: one prologue and one epilogue per 268 MFLOP (K1 = 512, Q = 4).
//
// Why 16 x 16 x 4 and not the 32 x 32 x 2 of the other fp32 forms: with 32 x 32 blocks the phase-2 accumulators of a
// wave - 32 values of u x 512 n2 - alone are 256 registers.  With 16 x 16 blocks a wave owns 16 values of u: 128
// registers in phase 2, 64 in phase 1 for half of m1.  A row of 512 floats is byte for byte a row of 256 doubles, so the
// accumulator count, the LDS rows and the tile bytes are those of k_zip_f64 (kernels_zip_f64.h), and so is the shape.
//
// How an accumulator becomes an operand (the fp32 16 x 16 x 4 layout, as in kernels_zipl.h): a result block D[i][j]
// leaves lane (j = lane & 15, h = lane >> 4) with row i = 4 h + e in register e (e = 0 .. 3).  Its A fragment is "row
// i = lane & 15, k = lane >> 4", its B fragment "column j = lane & 15, k = lane >> 4", one float per lane.  Which m1 (or
// n2) a row i stands for is the choice of the fragment read alone, and here a lane reads FOUR consecutive floats with one
// 16-byte LDS read and feeds them to four MFMAs t = 0 .. 3 (a "quad" g of 64 values): row i of MFMA t is 64 g + 4 i + t.
// Phase 1 computes D1[i = m1][j = u] that way; register e of lane (u, h) of accumulator 4 g + t is then
// T[m1 = 64 g + 16 h + 4 e + t][u] - exactly the B-side fragment "column u, k = h" of a k-step over the FOUR values
// m1 = 64 g + 16 h + 4 e + t, h = 0 .. 3 (rows 16 apart: that is what a phase-2 tile holds, see below), and the matching
// A-side fragment of lane (i, h) is Y[that m1][n2(i)].  Phase 2 accumulates D2^T[i = n2][j = u] (operands swapped, as in the
// other forms) with the same quads: register e of lane (u, h) of accumulator 4 G + t holds n2 = 64 G + 16 h + 4 e + t, so the
// registers e of the four accumulators of a quad are four consecutive floats of one row u - 16-byte stores, no shuffle.
//
// 8 waves = 4 u-blocks of 16 x 2 halves of m1.  Wave (ub, kh) forms Tq[m1 in half kh (4 quads), u-block ub] in phase 1
// (16 accumulators = 64 registers; 16 MFMAs per k-step: 4 E fragment reads + 1 X fragment) and in phase 2 sums ITS 256
// values of m1 into a partial E'[u-block ub, all 512 n2] (32 accumulators = 128 registers; 32 MFMAs per k-step: 8 Y
// fragment reads, the other operand from registers).  The two halves' partial sums meet once, after the last q, through
// LDS (fixed order: first half + second half), eight accumulators per round, four rounds.  A fragment read runs one group
// of 4 MFMAs (128 cycles of the matrix pipe) ahead; nothing else is scheduled by hand.  The register file is what bounds
// all of this: 192 accumulator registers leave 64 at two waves per SIMD.  With 4-byte fragment reads a group of 16 ahead
// (k_zip_f64's 32 fragment registers) the compiler spilled 12 registers, a group of 8 ahead still 10; what fits is 8
// fragment registers, the lane's LDS addresses kept as two pointers (the Yq address a wave-uniform distance from the E
// address), LDS-DMA addresses as scalar base + 32-bit lane offset, and the epilogue's lane values derived after the loop.
//
// Operand tiles arrive by LDS-DMA (glds16: 4 floats per lane, one instruction = 256 floats) in a 3-stage ring, one raw
// s_barrier per 8-deep tile in the middle of its MFMAs; only the four waves of the first m1 half issue requests, with
// running wave-uniform pointers (k_zip_f32's two choices).  Phase-1 tile: E 8 x 512 + Xq 8 x 64 (32 MFMAs per wave).
// Phase-2 tile: 8 rows of each m1 half of Yq x 512 (64 MFMAs per wave) - tile ms = 8 g + 2 e + tp holds the rows
// 64 g + 16 h + 4 e + 2 tp + ks (h = 0 .. 3, k-step ks = 0, 1) in LDS row 4 ks + h: the four rows that one fragment read
// touches are consecutive LDS rows, as the four k-rows of an E fragment read are.  k-rows of both images are 512 floats
// apart, NOT padded: a 16-byte LDS read is served in groups of 16 lanes made of 8 lanes of one k-row and 4 + 4 of the
// next (lanes 0-3, 12-15, 20-27; 4-11, 16-19, 28-31; ...), banked modulo 64, and a lane's 4 banks are 4 (lane & 15) +
// the row's offset: rows a whole bank row (a multiple of 64 floats) apart make every group cover all 64 banks once.  (A
// padded row - 528 floats, right for 4-byte reads, which are banked modulo 32 within each half of the wave - would put
// lanes 20-27 on the banks of lanes 12-15.)  The Xq image's rows are 64 floats apart - one request fills four of them -
// and its one 4-byte read per 16 MFMAs is 2-way conflicted.
// 8 deep is what fits: a stage is 16 rows x 512 floats = 32 KiB, the ring 96 KiB; 16 deep would be 192 KiB.
// A requesting wave issues 4 requests for E and - waves 0 and 1 only, four rows of 64 floats each - 1 for Xq, or 8 for
// Yq; the counts differ between waves, and every tile's barrier waits with vmcnt(0) for requests that are a whole tile
// old, as in k_zip_f32.
//
// Conditions (fused_forms.h, zip_match with zm = 512): |m1| = |n2| = 512, |u| a multiple of 64, K1 a multiple of 16 and
// >= 32 (the tile depth divides 16), every operand dense along its innermost index with uniform strides that are
// multiples of 4 (16-byte requests and stores), X and Y network inputs, fp32.  The intermediate's rescale is not
// applied, as in the other fused forms: the register reports 0 for the first step and the magnitude moves into the
// second step's rescale.  No atomics; every sum in a fixed order: bit-reproducible.
// ---------------------------------------------------------------------------
constexpr int Z5M = 512, Z5U = 64, Z5K = 8, Z5ST = 3;
constexpr int Z5ROW = Z5M;                      // floats between k-rows of the E and Y images: no padding (16-byte reads, see above)
constexpr int Z5X0 = Z5K * Z5ROW;               // where the Xq image [8][64] of a phase-1 tile begins
constexpr int Z5STG = 2 * Z5K * Z5ROW;          // stage: a phase-2 tile, 8192 floats = 32 KiB (a phase-1 tile takes 4608)
constexpr int Z5XA = 2048;                      // a wave's hand-over area: 8 blocks x 64 lanes x 4 floats = 8 KiB
static_assert(Z5ROW % 64 == 0, "16-byte fragment reads of consecutive k-rows: conflict-free with rows a whole bank row apart");
static_assert(8 * Z5XA <= Z5ST * Z5STG, "the hand-over goes through the ring's area");

typedef float z5_f4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(512, 1) void k_zip512_f32(ZipArgs a) {
  __shared__ __attribute__((aligned(16))) float smem[Z5ST * Z5STG + 16];
  double* red = reinterpret_cast<double*>(smem + Z5ST * Z5STG);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kh = w >> 2, ub = w & 3;
  const int l15 = lane & 15, h = lane >> 4;
  const int pid = zipq_pid(blockIdx.x, gridDim.x);
  const int per = a.U / Z5U;                   // workgroups per replica
  const int r = pid / per;
  const int t_ = pid - r * per;
  const int u0 = t_ * Z5U;
  CTN_ZIP_STAMP(0);
  void* const* tp = a.ptrs + (size_t)r * a.n_tensors;
  const float* __restrict__ E = (const float*)tp[a.idE];
  const float* __restrict__ X = (const float*)tp[a.idX] + u0;
  const float* __restrict__ Y = (const float*)tp[a.idY];
  float* __restrict__ C = (float*)tp[a.idC];

  const int T1 = a.K1 / Z5K;                   // phase-1 tiles per q
  constexpr int T2 = (Z5M / 2) / Z5K;          // phase-2 tiles per q: 8 rows of each m1 half at a time
  const int TQ = T1 + T2, TT = a.Q * TQ;

  // the LDS-DMA requests of the next tile not yet asked for: a cursor with running, wave-uniform pointers, and only the
  // four waves of the first m1 half issue them, each for both halves (see k_zip_f32 for both choices).
  // E: wave ub takes rows 2 ub, 2 ub + 1 of the tile, two requests of 256 floats per row.  Xq: waves 0 and 1 take rows
  // 4 ub .. 4 ub + 3 in one request (lane -> row lane >> 4, 4 floats at 4 (lane & 15)).  Yq: wave ub takes, of both m1
  // halves, the rows 64 g + 16 ub + 4 e + 2 tp, + 1 of tile ms = 8 g + 2 e + tp - consecutive in memory - into LDS rows
  // ub and 4 + ub; from one tile to the next its pointer moves on by 2 rows, or by 50 into the next group of 64.
  const float* const rE0 = E + (int64_t)(2 * ub) * a.ldE;
  const float* rE = rE0;
  const float* rX = X + (int64_t)(4 * ub) * a.ldXk;          // (read by waves 0 and 1 only)
  const float* rY = Y + (int64_t)(16 * ub) * a.ldYm;
  // (a lane's own part of a request's address is an unsigned 32-bit byte offset: the instruction adds it to the scalar pointer)
  const unsigned offE = 16u * lane, offX = 4u * (unsigned)(h * (int)a.ldXk + 4 * l15);
  auto at = [](const float* p, unsigned bytes) { return reinterpret_cast<const float*>(reinterpret_cast<const char*>(p) + bytes); };
  const int64_t stepE = (int64_t)Z5K * a.ldE, stepX = (int64_t)Z5K * a.ldXk;
  const int64_t stepY0 = 2 * a.ldYm, stepY1 = 50 * a.ldYm;
  const int64_t nextX = a.ldXq - (int64_t)a.K1 * a.ldXk, nextY = a.ldYq - (int64_t)(Z5M / 2) * a.ldYm;
  const int64_t halfY = (int64_t)(Z5M / 2) * a.ldYm;
  int rq_s = 0, rq_left = TT;
  auto request_issue = [&](int stage) {
    float* st = smem + stage * Z5STG;
    if (rq_s < T1) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int c = 0; c < 2; ++c) glds16(at(rE + i * a.ldE + 256 * c, offE), st + (2 * ub + i) * Z5ROW + 256 * c);
      if (ub < 2) glds16(at(rX, offX), st + Z5X0 + (4 * ub) * Z5U);
    } else {
#pragma unroll
      for (int hf = 0; hf < 2; ++hf)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int c = 0; c < 2; ++c)
            glds16(at(rY + hf * halfY + i * a.ldYm + 256 * c, offE), st + (hf * Z5K + 4 * i + ub) * Z5ROW + 256 * c);
    }
  };
  auto request_step = [&]() {                  // (plain selects: the running pointers stay in scalar registers)
    const bool p1 = rq_s < T1;
    const bool last8 = ((rq_s - T1) & 7) == 7; // the last phase-2 tile of a group of 64 values of m1
    --rq_left;
    ++rq_s;
    const bool wrap = rq_s == TQ;
    rq_s = wrap ? 0 : rq_s;
    rE = wrap ? rE0 : rE + (p1 ? stepE : 0);
    rX += (p1 ? stepX : 0) + (wrap ? nextX : 0);
    rY += (p1 ? 0 : (last8 ? stepY1 : stepY0)) + (wrap ? nextY : 0);
  };

  z5_f4 acc1[16], acc2[32];
#pragma unroll
  for (int i = 0; i < 16; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc1[i][e] = 0.f;
#pragma unroll
  for (int i = 0; i < 32; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc2[i][e] = 0.f;

#pragma unroll
  for (int i = 0; i < Z5ST - 1; ++i) {         // (TT >= 36 tiles)
    if (kh == 0) request_issue(i);
    request_step();
  }
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_waitcnt(0x0F70);          // vmcnt(0): once per pair - no need to count
  __builtin_amdgcn_s_barrier();
  CTN_ZIP_STAMP(1);

  int st_cur = 0, st_nxt = 1, st_req = Z5ST - 1;
#ifdef CTN_STAMPS
  unsigned long long wait_vm = 0, wait_bar = 0;
#endif
  auto middle = [&]() {                        // the barrier of a tile, in the middle of its MFMA phase
    __builtin_amdgcn_sched_barrier(0);
#ifdef CTN_STAMPS
    const unsigned long long s0 = __builtin_amdgcn_s_memtime();
#endif
    // vmcnt(0): tile t + 1 has landed - this wave's requests, a tile old
    __builtin_amdgcn_s_waitcnt(0x0F70);
#ifdef CTN_STAMPS
    const unsigned long long s1 = __builtin_amdgcn_s_memtime();
#endif
    __builtin_amdgcn_s_barrier();
#ifdef CTN_STAMPS
    const unsigned long long s2 = __builtin_amdgcn_s_memtime();
    wait_vm += s1 - s0;
    wait_bar += s2 - s1;
#endif
    if (kh == 0 && rq_left > 0) request_issue(st_req);
    __builtin_amdgcn_sched_barrier(0);
  };
  auto advance = [&]() {
    st_req = st_cur;
    st_cur = st_nxt;
    st_nxt = st_nxt == Z5ST - 1 ? 0 : st_nxt + 1;
  };
  // a lane's fragments in stage 0 (the loop keeps these two addresses and nothing else of the lane's):
  // E image [k1][512]: row h, column kh 256 + 4 (lane & 15); Yq image [half][4 ks + h][512]: row kh 8 + h, column
  // 4 (lane & 15) - a wave-uniform distance from the former; Xq image [k1][64]
  const float* const pA = smem + h * Z5ROW + kh * (Z5M / 2) + 4 * l15;
  const float* const pB = smem + Z5X0 + h * Z5U + ub * 16 + l15;
  const int dY = kh * (Z5K * Z5ROW - Z5M / 2);
  z5_f4 fa[2];
  float fb[2];

  for (int q = 0; q < a.Q; ++q) {
    // ---- phase 1: Tq[m1 half kh, u-block ub] = sum_k1 E[k1][m1] Xq[k1][u] ------------------------------------
    for (int s = 0; s < T1; ++s) {
      const float* cA = pA + st_cur * Z5STG;
      const float* cB = pB + st_cur * Z5STG;
      fa[0] = *reinterpret_cast<const z5_f4*>(cA);
      fb[0] = cB[0];
#pragma unroll
      for (int gp = 0; gp < 8; ++gp) {           // group gp = (k-step kk: rows 4 kk + h of the tile, quad g)
        const int c = gp & 1, nx = c ^ 1, kk = gp >> 2, g = gp & 3;
        if (gp + 1 < 8) {
          fa[nx] = *reinterpret_cast<const z5_f4*>(cA + 4 * ((gp + 1) >> 2) * Z5ROW + 64 * ((gp + 1) & 3));
          if (gp == 3) fb[1] = cB[4 * Z5U];
        }
        if (gp == 4) request_step();             // the cursor moves on in the shadow of this group's MFMAs
#pragma unroll
        for (int t = 0; t < 4; ++t)              // D1[m1 = 64 g + 4 i + t][u]
          acc1[4 * g + t] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[c][t], fb[kk], acc1[4 * g + t], 0, 0, 0);
        if (gp == 3) middle();
      }
      advance();
    }
    // ---- phase 2: E'[u-block ub, :] += sum over this half's m1 of Tq[m1][u] Yq[m1][n2] -------------------------
#pragma unroll
    for (int ms = 0; ms < T2; ++ms) {
      // tile ms = 8 g + 2 e + tp: its k-step ks pairs lane group h with m1 = 64 g + 16 h + 4 e + 2 tp + ks - register e
      // of accumulator 4 g + 2 tp + ks; a group of 4 MFMAs is an eighth of a k-step: gp = (k-step ks, quad G)
      const float* cY = pA + (st_cur * Z5STG + dY);
      fa[0] = *reinterpret_cast<const z5_f4*>(cY);
#pragma unroll
      for (int gp = 0; gp < 16; ++gp) {
        const int c = gp & 1, nx = c ^ 1, G = gp & 7;
        if (gp + 1 < 16) fa[nx] = *reinterpret_cast<const z5_f4*>(cY + 4 * ((gp + 1) >> 3) * Z5ROW + 64 * ((gp + 1) & 7));
        const float tq = acc1[4 * (ms >> 3) + 2 * (ms & 1) + (gp >> 3)][(ms >> 1) & 3];
        if (gp == 8) request_step();
#pragma unroll
        for (int t = 0; t < 4; ++t)              // D2^T[n2 = 64 G + 4 i + t][u]
          acc2[4 * G + t] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[c][t], tq, acc2[4 * G + t], 0, 0, 0);
        if (gp == 7) middle();
      }
      advance();
    }
#pragma unroll
    for (int i = 0; i < 16; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc1[i][e] = 0.f;
  }
#ifdef CTN_STAMPS
  if (a.dbg && tid == 0) {
    a.dbg[(size_t)pid * 8 + 2] = __builtin_amdgcn_s_memtime();
    a.dbg[(size_t)pid * 8 + 5] = wait_vm;
    a.dbg[(size_t)pid * 8 + 6] = wait_bar;
  }
  if (a.dbg && tid == 448) a.dbg[(size_t)pid * 8 + 7] = wait_vm + wait_bar;
#endif

  // What the lanes need from here on is derived anew from the lane number (read again, so that no register carries
  // any of it across the main loop: the loop has none to spare).
  // E's producer partials, for the epilogue: asked for here, after the main loop, and in flight during the hand-over
  int lane_e;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane_e));
  double pve = 0.0;
  if (a.partE) {
    const double* __restrict__ pr = a.partE + (size_t)r * a.strideE;
    pve = pr[min(lane_e, a.PE - 1)];
    if (a.PE > 64)
      for (int i = lane_e + 64; i < a.PE; i += 64) pve += pr[i];
  }

  // ---- the two m1 halves meet: half kh finishes n2 blocks 16 kh .. 16 kh + 15 and hands the other sixteen over, eight
  // per round through the ring's LDS (a wave's area: 8 blocks x 64 lanes x 4 floats = 8 KiB): first half + second half,
  // whichever wave adds
#pragma unroll
  for (int round = 0; round < 4; ++round) {
    __builtin_amdgcn_s_waitcnt(0xC07F);        // lgkmcnt(0): this wave's own LDS reads are done
    __builtin_amdgcn_s_barrier();              // ... and everybody's: the area is free
    if (kh != (round >> 1)) {
      z5_f4* xo = reinterpret_cast<z5_f4*>(smem + w * Z5XA) + lane_e;
#pragma unroll
      for (int i = 0; i < 8; ++i) xo[i * 64] = acc2[8 * round + i];
    }
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_s_barrier();
    if (kh == (round >> 1)) {
      const z5_f4* xi = reinterpret_cast<const z5_f4*>(smem + (w ^ 4) * Z5XA) + lane_e;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const z5_f4 o = xi[i * 64];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float m = acc2[8 * round + i][e];
          acc2[8 * round + i][e] = kh == 0 ? m + o[e] : o[e] + m;
        }
      }
    }
  }
  CTN_ZIP_STAMP(4);

  // ---- epilogue: lazy rescale by E's producer (X, Y are inputs), 16-byte stores, abs-sum partial ---------------
  pve = lane_e < a.PE ? pve : 0.0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) pve += __shfl_xor(pve, o, 64);
  const float nE = (float)pve;
  const float scE = (a.partE && nE > (float)a.min_norm) ? nE / (float)a.numelE : 1.f;
  const float iE = 1.0f / scE;
  float asum = 0.f;
  float* __restrict__ row = C + (int64_t)(u0 + 16 * ub + (lane_e & 15)) * a.ldC + 16 * (lane_e >> 4);
#pragma unroll
  for (int G = 0; G < 8; ++G) {
    if (kh == (G >> 2)) {                      // the quads this wave finished: register e of accumulator 4 G + t is n2 = 64 G + 16 h + 4 e + t
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        z5_f4 v;
        v[0] = acc2[4 * G + 0][e] * iE; v[1] = acc2[4 * G + 1][e] * iE; v[2] = acc2[4 * G + 2][e] * iE; v[3] = acc2[4 * G + 3][e] * iE;
        *reinterpret_cast<z5_f4*>(row + 64 * G + 4 * e) = v;
        asum += (fabsf(v[0]) + fabsf(v[1])) + (fabsf(v[2]) + fabsf(v[3]));
      }
    }
  }
  double part = (double)asum;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
  if (lane_e == 0) red[w] = part;
  __builtin_amdgcn_s_waitcnt(0xC07F);
  __builtin_amdgcn_s_barrier();
  if (w == 0 && lane_e == 0) {
    double tot = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) tot += red[i];
    a.partC[(size_t)r * a.partC_stride + t_] = tot;
  }
  CTN_ZIP_STAMP(3);
}

}  // namespace ctn
