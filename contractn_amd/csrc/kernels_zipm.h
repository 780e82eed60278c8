// kernels_zipm.h - the fused zipper site pair of kernels_zip.h for bond 128 and bond 64: both GEMMs of a site as ONE
// launch, the intermediate kept in the accumulators.  One kernel template, k_zipm_f32<M>, M = |m1| = |n2|; its two
// instantiations are k_zip128_f32 and k_zipm64_f32.  Part of the gfx950 contraction engine (see engine.hip for the overview).
#pragma once
#include "kernels_zip.h"

namespace ctn {

// ---------------------------------------------------------------------------
// K-zipm-f32<M>.  The pair of kernels_zip.h,
//
//     T[m1, (q, u)] = sum_k1  E[k1, m1] * X[q, k1, u]          E'[u, n2] = sum_(m1, q)  T[m1, q, u] * Y[q, m1, n2]
//
// with |m1| = |n2| = M, M = 128 or 64.  ONE workgroup owns M values of u and walks q: phase 1 forms
// Tq[m1 = 0..M-1, u-block] = E^T Xq in accumulators, phase 2 multiplies those accumulators - used directly as MFMA
// operands, no LDS round trip - into E'[u-block, 0..M-1] += Tq^T Yq.
//
// How an accumulator becomes an operand (the derivation of kernels_zip.h, which holds for any |m1|): a
// v_mfma_f32_32x32x2_f32 result block D[i][j] leaves lane (j = lane & 31, h = lane >> 5) with rows i = 8 g + 4 h + e in
// register 4 g + e.  Phase 1 computes D1[i = m1][j = u]; register (g, e) of lane (u, h) is then exactly the B-side
// fragment "column u, k = m1" of a k-step that pairs m1 = 8 g + e (lower lane half) with m1 = 8 g + 4 + e (upper half) -
// any pairing is fine as long as the other operand follows it, and the Y fragment is read from LDS row 8 g + 4 h + e
// accordingly.  Phase 2 accumulates D2^T[i = n2][j = u] (operands swapped, as in k_mfma_f32_g), so a lane ends up with
// 4 consecutive n2 of one row u per register quad: 16-byte stores.
//
// Everything that follows from M (the constants at the head of the kernel):
//   * M / 16 waves = M / 32 u-blocks of 32 x 2 halves of m1: wave (ub, kh) forms Tq[m1 in half kh (M / 64 blocks), u-block
//     ub] in phase 1 (M / 64 accumulators; per k-step M / 64 MFMAs: as many E fragments + 1 X fragment) and in phase 2
//     sums ITS M / 2 values of m1 into a partial E'[u-block ub, all M n2] (M / 32 accumulators; M / 32 MFMAs per k-step:
//     as many Y fragments, the other operand from registers).
//   * The two halves' partial sums meet once, after the last q, through LDS: each partner (w ^ M / 32) hands over half
//     of its n2 blocks and finishes the other half (first half + second half, whichever wave adds) - M / 64 blocks x 16
//     registers x 64 lanes = M / 64 x 4 KiB per wave, ONE round.
//   * Tile depth 16 (ZMK): a phase-1 tile is E 16 x M + Xq 16 x M, a phase-2 tile Yq 16 rows of each m1 half x M - a
//     stage of 32 M floats either way, the X image and the second half's Y image half a stage in; one raw s_barrier per
//     tile in the middle of its MFMA phase.  K1 a multiple of 16 and >= 32, k_zip_f32's condition.
//   * Every row of E, Xq and Yq is M floats = M / 4 lanes of a 16-byte LDS-DMA request, so a request of a wave fetches
//     64 / (M / 4) rows.  Only the M / 32 waves of the first m1 half issue requests, each for both halves (see k_zip_f32
//     for both choices): 16 / (M / 32) rows of a 16-row image per wave, which is 2 requests per image and 4 per tile of
//     either phase (ZMRQ) for both M.
//   * Ring of 4 stages (ZMST), requests TWO tiles ahead: the barrier of tile t waits for the requests of tile t + 1
//     only (vmcnt(4)), not for those of t + 2.
//
// What differs between the two, and why:
//   * M = 128 (k_zip128_f32).  At bond 128 (K1 = |u| = 128, Q = 4: 33.5 MFLOP per network) the two launches move 1152 KiB
//     per network - 29 flop per byte, 5.4 TB/s at the fp32 MFMA peak, more than this project has ever pulled from HBM -
//     and the fused form 640 KiB (E, X, Y, E'): 52 flop per byte, 3.0 TB/s.  8 waves, 32 + 64 accumulator registers,
//     16 / 32 MFMAs per wave and tile, stages of 16 KiB.  32-deep tiles would give k_zip_f32's 32 / 64 MFMAs between
//     barriers at 32 KiB per stage, but k_zip_f32's own 32-deep phase-1 tiles did not pay, and a ring of 32 KiB stages
//     that covers the hand-over does not leave room for two workgroups per CU.  The ring of 4 stages = 64 KiB is exactly
//     the area the one-round hand-over needs (8 KiB per wave), and a tile is half as long as k_zip_f32's - hence the
//     requests two tiles ahead.  TWO workgroups per CU, __launch_bounds__(512, 2): 96 accumulator + 14 fragment
//     registers fit the 128 a wave may hold then (the compiler's resource remark: see DESIGN section 4), 2 x 64.1 KiB of
//     LDS fit the CU's 160 KB, and one workgroup's prologue, barriers, hand-over and epilogue hide behind the other's
//     MFMAs.  The partials of E's producer are asked for after the main loop: two registers less across it, the budget
//     of two workgroups per CU.  (A CTN_STAMPS build needs 129 registers and runs ONE workgroup per CU: its stamps are
//     those of a workgroup alone.  Measured, DESIGN section 10: the launch of two co-resident workgroups per CU is ~5 %
//     shorter than two such workgroups back to back.)
//   * M = 64 (k_zipm64_f32).  At bond 64 (K1 = |u| = 64, Q = 4: 4.2 MFLOP per network) the two launches move 288 KiB per
//     network - 14 flop per byte - and the fused form 160 KiB (E, X, Y, E'): 26 flop per byte.  At the fp32 MFMA peak
//     that would be 11 and 6 TB/s: the pair is MEMORY-bound in either form, and what this instantiation is built around
//     is not the matrix pipe but the number of bytes a CU has on request.  4 waves, 16 + 32 accumulator registers,
//     8 / 16 MFMAs per wave and tile, stages of 8 KiB: a ring of 32 KiB (the hand-over needs 16), and a workgroup has
//     16 - 24 KiB on request.  FOUR workgroups per CU, __launch_bounds__(256, 4): a workgroup alone cannot cover HBM
//     latency with 24 KiB on request; four of them keep 64 - 96 KiB per CU in flight (the estimate this aims at: 8 TB/s
//     over 256 CUs at ~2 us loaded latency = 64 KB; an estimate, not a measurement).  4 x 32.1 KiB of LDS fit the CU's
//     160 KB - a fifth stage would not - and the registers are far below the 128 a wave may hold then (the compiler's
//     resource remark: see DESIGN section 4).  E is streamed again for every q, as in the other forms, although at
//     K1 <= 64 it would fit a fifth 16 KiB area of LDS: that area costs the fourth workgroup per CU, and E's repeated
//     reads (16 KiB, the same workgroup, microseconds apart) are served by L2.  Not measured either way (DESIGN
//     section 4).
//
// Conditions (engine.hip, zip_match with zm = M): |m1| = |n2| = M, |u| a multiple of M, K1 a multiple of 16 and >= 32,
// every operand dense along its innermost index with uniform strides that are multiples of 4 (16-byte requests and
// stores), X and Y network inputs, fp32.  The intermediate's rescale is not applied, as in the other fused forms: the
// register reports 0 for the first step and the magnitude moves into the second step's rescale.  No atomics; every sum
// in a fixed order: bit-reproducible.
// ---------------------------------------------------------------------------
constexpr int ZMK = 16;    // tile depth
constexpr int ZMST = 4;    // ring depth
constexpr int ZMRQ = 4;    // LDS-DMA instructions a requesting wave issues per tile, of EITHER phase: the vmcnt of a tile's barrier
// what the host's matcher is held to (engine.hip checks them against fused_forms.h): |m1|, values of u per workgroup, tile depth
constexpr int Z1M = 128, Z1U = Z1M, Z1K = ZMK;   // k_zip128_f32
constexpr int Z4M = 64, Z4U = Z4M, Z4K = ZMK;    // k_zipm64_f32

template <int M>
__global__ __launch_bounds__(4 * M, M == 128 ? 2 : 4) void k_zipm_f32(ZipArgs a) {
  static_assert(M == 64 || M == 128, "the two halves of m1 are whole 32 x 32 blocks, and a request is whole rows");
  constexpr int W = M / 16;                    // waves
  constexpr int UB = M / 32;                   // u-blocks of 32 = waves per m1 half = the requesting waves
  constexpr int A1 = M / 64, A2 = M / 32;      // accumulators of phase 1 and of phase 2; A2 / 2 = A1 of them are handed over
  constexpr int STG = 32 * M, HSTG = STG / 2;  // a stage in floats; the X image and the second half's Y image start half a stage in
  constexpr int LR = M / 4, RR = 64 / LR;      // lanes per requested row, rows per request
  constexpr int RW = ZMK / UB;                 // rows of a 16-row image per requesting wave
  constexpr int LOG_UB = M == 128 ? 2 : 1, LOG_LR = M == 128 ? 5 : 4;
  static_assert(1 << LOG_UB == UB && 1 << LOG_LR == LR, "wave and lane indices are split with shifts and masks");

  __shared__ __attribute__((aligned(16))) float smem[ZMST * STG + 2 * W];
  double* red = reinterpret_cast<double*>(smem + ZMST * STG);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kh = w >> LOG_UB, ub = w & (UB - 1);
  const int l31 = lane & 31, h = lane >> 5;
  const int lc = lane & (LR - 1), lr = lane >> LOG_LR;   // a request's view of the wave: RR rows of LR lanes x 16 bytes
  const int pid = zipq_pid(blockIdx.x, gridDim.x);
  const int per = a.U / M;                     // workgroups per replica
  const int r = pid / per;
  const int t_ = pid - r * per;
  const int u0 = t_ * M;
  CTN_ZIP_STAMP(0);
  void* const* tp = a.ptrs + (size_t)r * a.n_tensors;
  const float* __restrict__ E = (const float*)tp[a.idE];
  const float* __restrict__ X = (const float*)tp[a.idX] + u0;
  const float* __restrict__ Y = (const float*)tp[a.idY];
  float* __restrict__ C = (float*)tp[a.idC];

  const int T1 = a.K1 / ZMK;                   // phase-1 tiles per q
  constexpr int T2 = (M / 2) / ZMK;            // phase-2 tiles per q: 16 rows of each m1 half at a time
  const int TQ = T1 + T2, TT = a.Q * TQ;

  // the LDS-DMA requests of the next tile not yet asked for: a cursor with running, wave-uniform pointers, and only the
  // waves of the first m1 half issue them, each for both halves (see k_zip_f32 for both choices).  Wave ub asks for
  // rows RW ub .. RW ub + RW - 1 of a 16-row image, RR rows per request.
  const float* const rE0 = E + (int64_t)(RW * ub) * a.ldE;
  const float* rE = rE0;
  const float* rX = X + (int64_t)(RW * ub) * a.ldXk;
  const float* rY = Y + (int64_t)(RW * ub) * a.ldYm;
  const int offE = lr * (int)a.ldE + 4 * lc, offX = lr * (int)a.ldXk + 4 * lc, offY = lr * (int)a.ldYm + 4 * lc;
  const int64_t stepE = (int64_t)ZMK * a.ldE, stepX = (int64_t)ZMK * a.ldXk, stepY = (int64_t)ZMK * a.ldYm;
  const int64_t nextX = a.ldXq - (int64_t)a.K1 * a.ldXk, nextY = a.ldYq - (int64_t)(M / 2) * a.ldYm;
  const int64_t halfY = (int64_t)(M / 2) * a.ldYm;
  int rq_s = 0, rq_left = TT;
  // request_issue emits exactly ZMRQ instructions whichever branch it takes - middle()'s vmcnt(ZMRQ) counts on it: a
  // wave's RW rows of E, of Xq and of each half of Yq are 2 requests each
  constexpr int RQ_E = RW / RR, RQ_X = RW / RR, RQ_Y = RW / RR;
  static_assert(RQ_E + RQ_X == ZMRQ && 2 * RQ_Y == ZMRQ && ZMRQ < 16, "middle() waits with vmcnt(ZMRQ): the requests per tile");
  static_assert(UB * RR * RQ_E == ZMK && UB * RR * RQ_X == ZMK && UB * RR * RQ_Y == ZMK, "UB requesting waves, RR rows per request: a 16-row image");
  auto request_issue = [&](int stage) {
    float* st = smem + stage * STG;
    if (rq_s < T1) {             // this wave's rows of E and of Xq
#pragma unroll
      for (int i = 0; i < RQ_E; ++i) glds16(rE + RR * i * a.ldE + offE, st + (RW * ub + RR * i) * M);
#pragma unroll
      for (int i = 0; i < RQ_X; ++i) glds16(rX + RR * i * a.ldXk + offX, st + HSTG + (RW * ub + RR * i) * M);
    } else {                     // this wave's rows of both m1 halves of Yq
#pragma unroll
      for (int hf = 0; hf < 2; ++hf)
#pragma unroll
        for (int i = 0; i < RQ_Y; ++i) glds16(rY + hf * halfY + RR * i * a.ldYm + offY, st + hf * HSTG + (RW * ub + RR * i) * M);
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

  f32x16 acc1[A1], acc2[A2];
#pragma unroll
  for (int i = 0; i < A1; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc1[i][e] = 0.f;
#pragma unroll
  for (int i = 0; i < A2; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc2[i][e] = 0.f;

#pragma unroll
  for (int i = 0; i < ZMST - 1; ++i) {         // (TT >= 4 tiles: K1 >= 32)
    if (kh == 0) request_issue(i);
    request_step();
  }
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_waitcnt(0x0F70);          // vmcnt(0): once per pair - no need to count
  __builtin_amdgcn_s_barrier();
  CTN_ZIP_STAMP(1);

  constexpr int bar_at = 3;
  int st_cur = 0, st_nxt = 1, st_req = ZMST - 1;
#ifdef CTN_STAMPS
  unsigned long long wait_vm = 0, wait_bar = 0;
#endif
  auto middle = [&]() {                        // the barrier of a tile, in the middle of its MFMA phase
    __builtin_amdgcn_sched_barrier(0);
#ifdef CTN_STAMPS
    const unsigned long long s0 = __builtin_amdgcn_s_memtime();
#endif
    // tile t + 1 has landed.  This wave's requests are at most those of tiles t + 1 and t + 2, ZMRQ = 4 instructions each
    // and completed in order: vmcnt(ZMRQ) while tile t + 2 was asked for (at the barrier of tile t - 1: rq_left was > 0 there,
    // and one request_step() has run since), vmcnt(0) for the last two tiles.
    if (rq_left >= 0) __builtin_amdgcn_s_waitcnt(0x0F70 | ZMRQ);
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
    st_nxt = st_nxt == ZMST - 1 ? 0 : st_nxt + 1;
  };
  float fa[2][A1], fb[2], fy[2][A2];

  for (int q = 0; q < a.Q; ++q) {
    // ---- phase 1: Tq[m1 half kh, u-block ub] = sum_k1 E[k1][m1] Xq[k1][u] ------------------------------------
    for (int s = 0; s < T1; ++s) {
      const float* cA = smem + st_cur * STG + h * M + kh * (M / 2) + l31;          // E image [k1][M]
      const float* cB = smem + st_cur * STG + HSTG + h * M + ub * 32 + l31;        // Xq image [k1][M]
#pragma unroll
      for (int i = 0; i < A1; ++i) fa[0][i] = cA[32 * i];
      fb[0] = cB[0];
#pragma unroll
      for (int kk = 0; kk < ZMK / 2; ++kk) {
        const int c = kk & 1, nx = c ^ 1;
        if (kk + 1 < ZMK / 2) {
#pragma unroll
          for (int i = 0; i < A1; ++i) fa[nx][i] = cA[2 * (kk + 1) * M + 32 * i];
          fb[nx] = cB[2 * (kk + 1) * M];
        }
        if (kk == bar_at + 1) request_step();   // the cursor moves on in the shadow of this k-step's MFMAs
#pragma unroll
        for (int i = 0; i < A1; ++i)
          acc1[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[c][i], fb[c], acc1[i], 0, 0, 0);   // D1[m1][u]
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, A1 + 1, 0);
#pragma unroll
        for (int i = 0; i < A1 - 1; ++i) {
          __builtin_amdgcn_sched_group_barrier(0x004, 12, 0);
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        }
        if (kk == bar_at) middle();
      }
      advance();
    }
    // ---- phase 2: E'[u-block ub, :] += sum over this half's m1 of Tq[m1][u] Yq[m1][n2] -------------------------
#pragma unroll
    for (int ms = 0; ms < T2; ++ms) {
      // rows 16 ms .. 16 ms + 15 of the half = half of accumulator block ms / 2: its register groups g = 2 (ms & 1), + 1
      const float* cY = smem + st_cur * STG + kh * HSTG + (4 * h) * M + l31;       // Yq image [half][16 rows][M]
#pragma unroll
      for (int nb = 0; nb < A2; ++nb) fy[0][nb] = cY[32 * nb];
#pragma unroll
      for (int kk = 0; kk < 8; ++kk) {           // k-step (g, e) = (kk / 4, kk % 4): row 8 (kk / 4) + 4 h + e of the tile
        const int c = kk & 1, nx = c ^ 1;
        if (kk + 1 < 8) {
#pragma unroll
          for (int nb = 0; nb < A2; ++nb) fy[nx][nb] = cY[(8 * ((kk + 1) / 4) + (kk + 1) % 4) * M + 32 * nb];
        }
        const float tq = acc1[ms / 2][4 * (2 * (ms & 1) + kk / 4) + kk % 4];
        if (kk == bar_at + 1) request_step();
#pragma unroll
        for (int nb = 0; nb < A2; ++nb)
          acc2[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(fy[c][nb], tq, acc2[nb], 0, 0, 0);       // D2^T[n2][u]
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, A2, 0);
#pragma unroll
        for (int i = 0; i < A2 - 1; ++i) {
          if constexpr (M > 64) __builtin_amdgcn_sched_group_barrier(0x004, 6, 0);
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        }
        if (kk == bar_at) middle();
      }
      advance();
    }
#pragma unroll
    for (int i = 0; i < A1; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc1[i][e] = 0.f;
  }
#ifdef CTN_STAMPS
  if (a.dbg && tid == 0) {
    a.dbg[(size_t)pid * 8 + 2] = __builtin_amdgcn_s_memtime();
    a.dbg[(size_t)pid * 8 + 5] = wait_vm;
    a.dbg[(size_t)pid * 8 + 6] = wait_bar;
  }
  if (a.dbg && tid == (W - 1) * 64) a.dbg[(size_t)pid * 8 + 7] = wait_vm + wait_bar;
#endif

  // E's producer partials, for the epilogue: asked for here, after the main loop (two registers less across it - the
  // budget of two workgroups per CU at M = 128), and in flight during the hand-over
  double pve = 0.0;
  if (a.partE) {
    const double* __restrict__ pr = a.partE + (size_t)r * a.strideE;
    pve = pr[min(lane, a.PE - 1)];
    if (a.PE > 64)
      for (int i = lane + 64; i < a.PE; i += 64) pve += pr[i];
  }

  // ---- the two m1 halves meet: half kh finishes n2 blocks A1 kh .. A1 kh + A1 - 1 and hands the other A1 over - one
  // round through the ring's LDS (a wave's area: A1 blocks x 16 registers x 64 lanes = A1 x 4 KiB): first half + second
  // half, whichever wave adds
  f32x16 mine[A1], give[A1];
  if (kh == 0) {
#pragma unroll
    for (int i = 0; i < A1; ++i) { mine[i] = acc2[i]; give[i] = acc2[A1 + i]; }
  } else {
#pragma unroll
    for (int i = 0; i < A1; ++i) { mine[i] = acc2[A1 + i]; give[i] = acc2[i]; }
  }
  __builtin_amdgcn_s_waitcnt(0xC07F);          // lgkmcnt(0): this wave's own LDS reads are done
  __builtin_amdgcn_s_barrier();                // ... and everybody's: the area is free
  {
    float4* xo = reinterpret_cast<float4*>(smem + w * (A1 * 1024)) + lane;
#pragma unroll
    for (int i = 0; i < A1; ++i)
#pragma unroll
      for (int qd = 0; qd < 4; ++qd)
        xo[(i * 4 + qd) * 64] = make_float4(give[i][4 * qd], give[i][4 * qd + 1], give[i][4 * qd + 2], give[i][4 * qd + 3]);
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_s_barrier();
    const float4* xi = reinterpret_cast<const float4*>(smem + (w ^ UB) * (A1 * 1024)) + lane;
#pragma unroll
    for (int i = 0; i < A1; ++i)
#pragma unroll
      for (int qd = 0; qd < 4; ++qd) {
        const float4 o = xi[(i * 4 + qd) * 64];
        const float ov[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float m = mine[i][4 * qd + e];
          mine[i][4 * qd + e] = kh == 0 ? m + ov[e] : ov[e] + m;
        }
      }
  }
  CTN_ZIP_STAMP(4);

  // ---- epilogue: lazy rescale by E's producer (X, Y are inputs), 16-byte stores, abs-sum partial ---------------
  pve = lane < a.PE ? pve : 0.0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) pve += __shfl_xor(pve, o, 64);
  const float nE = (float)pve;
  const float scE = (a.partE && nE > (float)a.min_norm) ? nE / (float)a.numelE : 1.f;
  const float iE = 1.0f / scE;
  float asum = 0.f;
  float* __restrict__ row = C + (int64_t)(u0 + 32 * ub + l31) * a.ldC + 4 * h;
#pragma unroll
  for (int i = 0; i < A1; ++i) {
    const int nb = A1 * kh + i;                // the n2 block this accumulator holds
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float4 v;
      v.x = mine[i][4 * g + 0] * iE; v.y = mine[i][4 * g + 1] * iE; v.z = mine[i][4 * g + 2] * iE; v.w = mine[i][4 * g + 3] * iE;
      *reinterpret_cast<float4*>(row + 32 * nb + 8 * g) = v;
      asum += (fabsf(v.x) + fabsf(v.y)) + (fabsf(v.z) + fabsf(v.w));
    }
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
    for (int i = 0; i < W; ++i) tot += red[i];
    a.partC[(size_t)r * a.partC_stride + t_] = tot;
  }
  CTN_ZIP_STAMP(3);
}

// the names the launch table, the ABI's form names and DESIGN use
constexpr auto k_zip128_f32 = k_zipm_f32<128>;
constexpr auto k_zipm64_f32 = k_zipm_f32<64>;

}  // namespace ctn
