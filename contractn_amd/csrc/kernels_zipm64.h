// kernels_zipm64.h - the fused zipper site pair of kernels_zip.h for bond 64: both GEMMs of a site as ONE launch, the
// intermediate kept in the accumulators.  Part of the gfx950 contraction engine (see engine.hip for the overview).
#pragma once
#include "kernels_zip.h"

namespace ctn {

// ---------------------------------------------------------------------------
// K-zipm64-f32.  The pair of kernels_zip.h,
//
//     T[m1, (q, u)] = sum_k1  E[k1, m1] * X[q, k1, u]          E'[u, n2] = sum_(m1, q)  T[m1, q, u] * Y[q, m1, n2]
//
// with |m1| = |n2| = 64.  At bond 64 (K1 = |u| = 64, Q = 4: 4.2 MFLOP per network) the two launches move 288 KiB per
// network - 14 flop per byte - and the fused form 160 KiB (E, X, Y, E'): 26 flop per byte.  At the fp32 MFMA peak that
// would be 11 and 6 TB/s: the pair is MEMORY-bound in either form, and what this kernel is built around is not the
// matrix pipe but the number of bytes a CU has on request.  ONE workgroup owns 64 values of u and walks q: phase 1
// forms Tq[m1 = 0..63, u-block] = E^T Xq in accumulators, phase 2 multiplies those accumulators - used directly as MFMA
// operands, no LDS round trip - into E'[u-block, 0..63] += Tq^T Yq.
//
// How an accumulator becomes an operand (the derivation of kernels_zip.h, which holds for any |m1|): a
// v_mfma_f32_32x32x2_f32 result block D[i][j] leaves lane (j = lane & 31, h = lane >> 5) with rows i = 8 g + 4 h + e in
// register 4 g + e.  Phase 1 computes D1[i = m1][j = u]; register (g, e) of lane (u, h) is then exactly the B-side
// fragment "column u, k = m1" of a k-step that pairs m1 = 8 g + e (lower lane half) with m1 = 8 g + 4 + e (upper half),
// and the Y fragment is read from LDS row 8 g + 4 h + e accordingly.  Phase 2 accumulates D2^T[i = n2][j = u] (operands
// swapped), so a lane ends up with 4 consecutive n2 of one row u per register quad: 16-byte stores.
//
// 4 waves = 2 u-blocks of 32 x 2 halves of m1: wave (ub, kh) forms Tq[m1 in half kh (1 block), u-block ub] in phase 1
// (1 accumulator = 16 registers; 1 MFMA per k-step: 1 E fragment + 1 X fragment) and in phase 2 sums ITS 32 values of
// m1 into a partial E'[u-block ub, all 64 n2] (2 accumulators = 32 registers; 2 MFMAs per k-step: 2 Y fragments, the
// other operand from registers).  The two halves' partial sums meet once, after the last q, through LDS: each partner
// hands over one n2 block and finishes the other (first half + second half, whichever wave adds) - 4 KiB per wave,
// half the ring, ONE round.
//
// The calls this file makes:
//   * Tile depth 16 (Z4K): a phase-1 tile is E 16 x 64 + Xq 16 x 64, a phase-2 tile Yq 16 rows of each m1 half x 64 -
//     8 KiB either way, 8 / 16 MFMAs per wave, one raw s_barrier per tile in the middle of its MFMA phase.  Every row
//     of E, Xq and Yq is 64 floats: one 16-byte LDS-DMA request of a wave fetches FOUR rows (lanes 16 i .. 16 i + 15 row
//     i), and a tile is 8 such requests - 4 from each of the two requesting waves, of either phase (Z4RQ).
//   * Ring of 4 stages (Z4ST) = 32 KiB, requests two tiles ahead as in k_zip128_f32: the barrier of tile t waits for the
//     requests of tile t + 1 only (vmcnt(4)), not for those of t + 2.  A workgroup has 16 - 24 KiB on request.
//   * FOUR workgroups per CU, __launch_bounds__(256, 4): a workgroup alone cannot cover HBM latency with 24 KiB on
//     request; four of them keep 64 - 96 KiB per CU in flight (the estimate this aims at: 8 TB/s over 256 CUs at ~2 us
//     loaded latency = 64 KB; an estimate, not a measurement).  4 x 32.1 KiB of LDS fit the CU's 160 KB - a fifth stage
//     would not - and the registers are far below the 128 a wave may hold then (the compiler's resource remark: see
//     DESIGN section 4).
//   * E is streamed again for every q, as in the other forms, although at K1 <= 64 it would fit a fifth 16 KiB area of
//     LDS: that area costs the fourth workgroup per CU, and E's repeated reads (16 KiB, the same workgroup, microseconds
//     apart) are served by L2.  Not measured either way.
//
// Conditions (engine.hip, zip_match with zm = 64): |m1| = |n2| = 64, |u| a multiple of 64, K1 a multiple of 16 and
// >= 32, every operand dense along its innermost index with uniform strides that are multiples of 4 (16-byte requests
// and stores), X and Y network inputs, fp32.  The intermediate's rescale is not applied, as in the other fused forms:
// the register reports 0 for the first step and the magnitude moves into the second step's rescale.  No atomics; every
// sum in a fixed order: bit-reproducible.
// ---------------------------------------------------------------------------
constexpr int Z4M = 64, Z4U = 64, Z4K = 16, Z4STG = 2048;      // stage: 2048 floats = 8 KiB
constexpr int Z4ST = 4;                                         // ring depth: 32 KiB (the hand-over needs 16)
constexpr int Z4RQ = 4;    // LDS-DMA instructions a requesting wave issues per tile, of EITHER phase: the vmcnt of a tile's barrier

__global__ __launch_bounds__(256, 4) void k_zipm64_f32(ZipArgs a) {
  __shared__ __attribute__((aligned(16))) float smem[Z4ST * Z4STG + 8];
  double* red = reinterpret_cast<double*>(smem + Z4ST * Z4STG);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kh = w >> 1, ub = w & 1;
  const int l31 = lane & 31, h = lane >> 5;
  const int l15 = lane & 15, r4 = lane >> 4;   // a request's view of the wave: 4 rows of 16 lanes x 16 bytes
  const int nwg = gridDim.x, bid = blockIdx.x;
  const int xcd = bid & 7, slot = bid >> 3, q8 = nwg >> 3, r8 = nwg & 7;
  const int pid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + slot;
  const int per = a.U / Z4U;                   // workgroups per replica
  const int r = pid / per;
  const int t_ = pid - r * per;
  const int u0 = t_ * Z4U;
#ifdef CTN_STAMPS
  if (a.dbg && tid == 0) a.dbg[(size_t)pid * 8 + 0] = __builtin_amdgcn_s_memtime();
#endif
  void* const* tp = a.ptrs + (size_t)r * a.n_tensors;
  const float* __restrict__ E = (const float*)tp[a.idE];
  const float* __restrict__ X = (const float*)tp[a.idX] + u0;
  const float* __restrict__ Y = (const float*)tp[a.idY];
  float* __restrict__ C = (float*)tp[a.idC];

  const int T1 = a.K1 / Z4K;                   // phase-1 tiles per q
  constexpr int T2 = (Z4M / 2) / Z4K;          // phase-2 tiles per q: 16 rows of each m1 half at a time
  const int TQ = T1 + T2, TT = a.Q * TQ;

  // the LDS-DMA requests of the next tile not yet asked for: a cursor with running, wave-uniform pointers, and only the
  // two waves of the first m1 half issue them, each for both halves (see k_zip_f32 for both choices).  Wave ub asks for
  // rows 8 ub .. 8 ub + 7 of a 16-row image: two requests of four rows.
  const float* const rE0 = E + (int64_t)(8 * ub) * a.ldE;
  const float* rE = rE0;
  const float* rX = X + (int64_t)(8 * ub) * a.ldXk;
  const float* rY = Y + (int64_t)(8 * ub) * a.ldYm;
  const int offE = r4 * (int)a.ldE + 4 * l15, offX = r4 * (int)a.ldXk + 4 * l15, offY = r4 * (int)a.ldYm + 4 * l15;
  const int64_t stepE = (int64_t)Z4K * a.ldE, stepX = (int64_t)Z4K * a.ldXk, stepY = (int64_t)Z4K * a.ldYm;
  const int64_t nextX = a.ldXq - (int64_t)a.K1 * a.ldXk, nextY = a.ldYq - (int64_t)(Z4M / 2) * a.ldYm;
  const int64_t halfY = (int64_t)(Z4M / 2) * a.ldYm;
  int rq_s = 0, rq_left = TT;
  // request_issue emits exactly Z4RQ instructions whichever branch it takes - middle()'s vmcnt(Z4RQ) counts on it: a
  // wave's 8 rows of E, of Xq and of each half of Yq are 2 requests each
  constexpr int RQ_E = 2, RQ_X = 2, RQ_Y = 2;
  static_assert(RQ_E + RQ_X == Z4RQ && 2 * RQ_Y == Z4RQ && Z4RQ < 16, "middle() waits with vmcnt(Z4RQ): the requests per tile");
  static_assert(2 * 4 * RQ_E == Z4K && 2 * 4 * RQ_X == Z4K && 2 * 4 * RQ_Y == Z4K, "two requesting waves, four rows per request: a 16-row image");
  auto request_issue = [&](int stage) {
    float* st = smem + stage * Z4STG;
    if (rq_s < T1) {             // rows 8 ub .. 8 ub + 7 of E and of Xq
#pragma unroll
      for (int i = 0; i < RQ_E; ++i) glds16(rE + 4 * i * a.ldE + offE, st + (8 * ub + 4 * i) * Z4M);
#pragma unroll
      for (int i = 0; i < RQ_X; ++i) glds16(rX + 4 * i * a.ldXk + offX, st + 1024 + (8 * ub + 4 * i) * Z4U);
    } else {                     // rows 8 ub .. 8 ub + 7 of both m1 halves of Yq
#pragma unroll
      for (int hf = 0; hf < 2; ++hf)
#pragma unroll
        for (int i = 0; i < RQ_Y; ++i) glds16(rY + hf * halfY + 4 * i * a.ldYm + offY, st + hf * 1024 + (8 * ub + 4 * i) * Z4M);
    }
  };
  auto request_step = [&]() {                  // (plain selects: the running pointers stay in scalar registers)
    const bool p1 = rq_s < T1;
    --rq_left;
    ++rq_s;
    const bool wrap = rq_s == TQ;
    rq_s = wrap ? 0 : rq_s;
    rE = wrap ? rE0 : rE + (p1 ? stepE : 0);
    rX += (p1 ? stepX : 0) + (wrap ? nextX : 0);
    rY += (p1 ? 0 : stepY) + (wrap ? nextY : 0);
  };

  f32x16 acc1, acc2[2];
#pragma unroll
  for (int e = 0; e < 16; ++e) acc1[e] = 0.f;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc2[i][e] = 0.f;

#pragma unroll
  for (int i = 0; i < Z4ST - 1; ++i) {         // (TT >= 4 tiles: K1 >= 32)
    if (kh == 0) request_issue(i);
    request_step();
  }
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_waitcnt(0x0F70);          // vmcnt(0): once per pair - no need to count
  __builtin_amdgcn_s_barrier();
#ifdef CTN_STAMPS
  if (a.dbg && tid == 0) a.dbg[(size_t)pid * 8 + 1] = __builtin_amdgcn_s_memtime();
#endif

  constexpr int bar_at = 3;
  int st_cur = 0, st_nxt = 1, st_req = Z4ST - 1;
#ifdef CTN_STAMPS
  unsigned long long wait_vm = 0, wait_bar = 0;
#endif
  auto middle = [&]() {                        // the barrier of a tile, in the middle of its MFMA phase
    __builtin_amdgcn_sched_barrier(0);
#ifdef CTN_STAMPS
    const unsigned long long s0 = __builtin_amdgcn_s_memtime();
#endif
    // tile t + 1 has landed.  This wave's requests are at most those of tiles t + 1 and t + 2, Z4RQ = 4 instructions each
    // and completed in order: vmcnt(Z4RQ) while tile t + 2 was asked for (at the barrier of tile t - 1: rq_left was > 0 there,
    // and one request_step() has run since), vmcnt(0) for the last two tiles.
    if (rq_left >= 0) __builtin_amdgcn_s_waitcnt(0x0F70 | Z4RQ);
    else __builtin_amdgcn_s_waitcnt(0x0F70);
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
    st_nxt = st_nxt == Z4ST - 1 ? 0 : st_nxt + 1;
  };
  float fa[2], fb[2], fy[2][2];

  for (int q = 0; q < a.Q; ++q) {
    // ---- phase 1: Tq[m1 half kh, u-block ub] = sum_k1 E[k1][m1] Xq[k1][u] ------------------------------------
    for (int s = 0; s < T1; ++s) {
      const float* cA = smem + st_cur * Z4STG + h * Z4M + kh * (Z4M / 2) + l31;       // E image [k1][64]
      const float* cB = smem + st_cur * Z4STG + 1024 + h * Z4U + ub * 32 + l31;       // Xq image [k1][64]
      fa[0] = cA[0];
      fb[0] = cB[0];
#pragma unroll
      for (int kk = 0; kk < Z4K / 2; ++kk) {
        const int c = kk & 1, nx = c ^ 1;
        if (kk + 1 < Z4K / 2) {
          fa[nx] = cA[2 * (kk + 1) * Z4M];
          fb[nx] = cB[2 * (kk + 1) * Z4U];
        }
        if (kk == bar_at + 1) request_step();   // the cursor moves on in the shadow of this k-step's MFMA
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[c], fb[c], acc1, 0, 0, 0);     // D1[m1][u]
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
        if (kk == bar_at) middle();
      }
      advance();
    }
    // ---- phase 2: E'[u-block ub, :] += sum over this half's m1 of Tq[m1][u] Yq[m1][n2] -------------------------
#pragma unroll
    for (int ms = 0; ms < T2; ++ms) {
      // rows 16 ms .. 16 ms + 15 of the half = half of the accumulator block: its register groups g = 2 ms, 2 ms + 1
      const float* cY = smem + st_cur * Z4STG + kh * 1024 + (4 * h) * Z4M + l31;       // Yq image [half][16 rows][64]
#pragma unroll
      for (int nb = 0; nb < 2; ++nb) fy[0][nb] = cY[32 * nb];
#pragma unroll
      for (int kk = 0; kk < 8; ++kk) {           // k-step (g, e) = (kk / 4, kk % 4): row 8 (kk / 4) + 4 h + e of the tile
        const int c = kk & 1, nx = c ^ 1;
        if (kk + 1 < 8) {
#pragma unroll
          for (int nb = 0; nb < 2; ++nb) fy[nx][nb] = cY[(8 * ((kk + 1) / 4) + (kk + 1) % 4) * Z4M + 32 * nb];
        }
        const float tq = acc1[4 * (2 * ms + kk / 4) + kk % 4];
        if (kk == bar_at + 1) request_step();
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
          acc2[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(fy[c][nb], tq, acc2[nb], 0, 0, 0);       // D2^T[n2][u]
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        if (kk == bar_at) middle();
      }
      advance();
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) acc1[e] = 0.f;
  }
#ifdef CTN_STAMPS
  if (a.dbg && tid == 0) {
    a.dbg[(size_t)pid * 8 + 2] = __builtin_amdgcn_s_memtime();
    a.dbg[(size_t)pid * 8 + 5] = wait_vm;
    a.dbg[(size_t)pid * 8 + 6] = wait_bar;
  }
  if (a.dbg && tid == 192) a.dbg[(size_t)pid * 8 + 7] = wait_vm + wait_bar;
#endif

  // E's producer partials, for the epilogue: asked for here, after the main loop, and in flight during the hand-over
  double pve = 0.0;
  if (a.partE) {
    const double* __restrict__ pr = a.partE + (size_t)r * a.strideE;
    pve = pr[min(lane, a.PE - 1)];
    if (a.PE > 64)
      for (int i = lane + 64; i < a.PE; i += 64) pve += pr[i];
  }

  // ---- the two m1 halves meet: half kh finishes n2 block kh and hands the other one over - one round through the
  // ring's LDS (a wave's area: 16 registers x 64 lanes = 4 KiB): first half + second half, whichever wave adds
  f32x16 mine, give;
  if (kh == 0) { mine = acc2[0]; give = acc2[1]; }
  else { mine = acc2[1]; give = acc2[0]; }
  __builtin_amdgcn_s_waitcnt(0xC07F);          // lgkmcnt(0): this wave's own LDS reads are done
  __builtin_amdgcn_s_barrier();                // ... and everybody's: the area is free
  {
    float4* xo = reinterpret_cast<float4*>(smem + w * 1024) + lane;
#pragma unroll
    for (int qd = 0; qd < 4; ++qd)
      xo[qd * 64] = make_float4(give[4 * qd], give[4 * qd + 1], give[4 * qd + 2], give[4 * qd + 3]);
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_s_barrier();
    const float4* xi = reinterpret_cast<const float4*>(smem + (w ^ 2) * 1024) + lane;
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) {
      const float4 o = xi[qd * 64];
      const float ov[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float m = mine[4 * qd + e];
        mine[4 * qd + e] = kh == 0 ? m + ov[e] : ov[e] + m;
      }
    }
  }
#ifdef CTN_STAMPS
  if (a.dbg && tid == 0) a.dbg[(size_t)pid * 8 + 4] = __builtin_amdgcn_s_memtime();
#endif

  // ---- epilogue: lazy rescale by E's producer (X, Y are inputs), 16-byte stores, abs-sum partial ---------------
  pve = lane < a.PE ? pve : 0.0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) pve += __shfl_xor(pve, o, 64);
  const float nE = (float)pve;
  const float scE = (a.partE && nE > (float)a.min_norm) ? nE / (float)a.numelE : 1.f;
  const float iE = 1.0f / scE;
  float asum = 0.f;
  float* __restrict__ row = C + (int64_t)(u0 + 32 * ub + l31) * a.ldC + 4 * h + 32 * kh;   // n2 block kh is this wave's
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    float4 v;
    v.x = mine[4 * g + 0] * iE; v.y = mine[4 * g + 1] * iE; v.z = mine[4 * g + 2] * iE; v.w = mine[4 * g + 3] * iE;
    *reinterpret_cast<float4*>(row + 8 * g) = v;
    asum += (fabsf(v.x) + fabsf(v.y)) + (fabsf(v.z) + fabsf(v.w));
  }
  double part = (double)asum;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
  if (lane == 0) red[w] = part;
  __builtin_amdgcn_s_waitcnt(0xC07F);
  __builtin_amdgcn_s_barrier();
  if (tid == 0) {
    double tot = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) tot += red[i];
    a.partC[(size_t)r * a.partC_stride + t_] = tot;
  }
#ifdef CTN_STAMPS
  if (a.dbg && tid == 0) a.dbg[(size_t)pid * 8 + 3] = __builtin_amdgcn_s_memtime();
#endif
}

}  // namespace ctn
