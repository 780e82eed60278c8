// kernels_zip_f64.h - the fused zipper site pair of kernels_zip.h in float64: both GEMMs of a site as ONE launch, the
// intermediate kept in v_mfma_f64_16x16x4_f64 accumulators.  Part of the gfx950 contraction engine (see engine.hip).
#pragma once
#include "kernels_zip.h"
#include "kernels_mfma_g64.h"

namespace ctn {

// ---------------------------------------------------------------------------
// K-zip-f64.  The pair of kernels_zip.h,
//
//     T[m1, (q, u)] = sum_k1  E[k1, m1] * X[q, k1, u]          E'[u, n2] = sum_(m1, q)  T[m1, q, u] * Y[q, m1, n2]
//
// with |m1| = |n2| = 256, in float64 - the dtype of the reference's examples and of its log register.  As two launches
// (k_mfma_f64_g) the 4 MiB T of a site is written and read again per network and the K = 256 step pays a prologue and an
// epilogue every 32 k-tiles.  Here ONE workgroup owns 64 values of u and walks q: phase 1 forms Tq[m1, u-block] in
// accumulators, phase 2 multiplies those accumulators - used directly as MFMA operands - into E'[u-block, 0..255], and T
// never exists outside the register file: one prologue and one epilogue per 67 MFLOP (K1 = 256, Q = 4).
//
// How an accumulator becomes an operand (16 x 16 x 4, not the 32 x 32 x 2 of the fp32 form): a v_mfma_f64_16x16x4_f64
// result block D[i][j] leaves lane (j = lane & 15, h = lane >> 4) with row i = h + 4 e in register e (e = 0 .. 3; the
// epilogues of k_mfma_f64 / k_mfma_f64_g store from the same layout: row = q + 4 e).  Its A fragment is "row i = lane & 15,
// k = lane >> 4", its B fragment "column j = lane & 15, k = lane >> 4", one double per lane.  Phase 1 computes
// D1[i = m1][j = u] block by block of 16 m1; register e of lane (u, h) is then T[m1 = 4 e + h][u] - exactly the B-side
// fragment "column u, k = h" of a k-step over m1 = 4 e .. 4 e + 3, and the matching A-side fragment of lane (i, h) is
// Y[m1 = 4 e + h][n2(i)].  Phase 2 accumulates D2^T[i][j = u] (operands swapped, as in the fp32 form).  Which n2 a row i
// stands for is the choice of the Y fragment read alone, and with n2(i) = 16 nb + 4 (i & 3) + (i >> 2) register e of lane
// (u, h) holds n2 = 16 nb + 4 h + e: four consecutive doubles of one row u per accumulator - 16-byte stores.  (The
// fragment read stays inside the same 128 bytes of the LDS row, so the permutation costs no bank conflict.)
//
// Shape (a) of the two that fit the register file: 8 waves = 4 u-blocks of 16 x 2 halves of m1.  Wave (ub, kh) forms
// Tq[m1 in half kh (8 blocks of 16), u-block ub] in phase 1 (8 accumulators = 64 registers; 8 MFMAs per k-step: 8 E
// fragments + 1 X fragment) and in phase 2 sums ITS 128 values of m1 into a partial E'[u-block ub, all 256 n2]
// (16 accumulators = 128 registers; 16 MFMAs per k-step: 16 Y fragments, the other operand from registers).  The two
// halves' partial sums meet once, after the last q, through LDS (fixed order: first half + second half).
// At the fp64 rate (78.6 TFLOP/s over 256 CUs: 2048 flop of one MFMA take a SIMD 64 cycles) a wave reads 8 fragments
// per ~500 cycles of MFMAs: the fragments are read one group of 8 MFMAs ahead and nothing else is scheduled by hand.
//
// Operand tiles arrive by LDS-DMA (glds16d: 2 doubles per lane, one instruction = 128 doubles) in a 3-stage ring, one raw
// s_barrier per 8-deep tile in the middle of its MFMAs; phase-1 tile: E 8 x 256 + Xq 8 x 64 (16 MFMAs per wave), phase-2
// tile: Yq 8 rows of each m1 half x 256 (32 MFMAs per wave).  k-rows of E and Y are 272 doubles apart in LDS (the rule of
// kernels_mfma_g64.h: an LDS-DMA destination is lane-linear only within one instruction, so the row distance is free):
// the four k-rows that one fragment read touches start 32 banks apart, rows h and h + 1 never on the same bank.
//
// Conditions (engine.hip, zip_match): |m1| = |n2| = 256, |u| a multiple of 64, K1 a multiple of 8 and >= 16, every operand
// dense along its innermost index with uniform EVEN strides (16-byte requests and stores), X and Y network inputs, fp64.
// The intermediate's rescale is not applied, as in the fp32 forms: the register reports 0 for the first step and the
// magnitude moves into the second step's rescale.  No atomics; every sum in a fixed order: bit-reproducible.
// ---------------------------------------------------------------------------
constexpr int ZDU = 64, ZDK = 8, ZDST = 3;
constexpr int ZDROW = ZM + 16;                  // doubles between k-rows of the E and Y images
constexpr int ZDX0 = ZDK * ZDROW;               // where the Xq image [8][64] of a phase-1 tile begins
constexpr int ZDSTG = 2 * ZDK * ZDROW;          // stage: a phase-2 tile, 4352 doubles = 34 KiB (a phase-1 tile takes 2688)

__global__ __launch_bounds__(512, 1) void k_zip_f64(ZipArgs a) {
  __shared__ __attribute__((aligned(16))) double smem[ZDST * ZDSTG + 8];
  double* red = smem + ZDST * ZDSTG;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kh = w >> 2, ub = w & 3;
  const int l15 = lane & 15, h = lane >> 4;
  const int pid = zipq_pid(blockIdx.x, gridDim.x);
  const int per = a.U / ZDU;                   // workgroups per replica
  const int r = pid / per;
  const int t_ = pid - r * per;
  const int u0 = t_ * ZDU;
  CTN_ZIP_STAMP(0);
  void* const* tp = a.ptrs + (size_t)r * a.n_tensors;
  const double* __restrict__ E = (const double*)tp[a.idE];
  const double* __restrict__ X = (const double*)tp[a.idX] + u0;
  const double* __restrict__ Y = (const double*)tp[a.idY];
  double* __restrict__ C = (double*)tp[a.idC];

  const int T1 = a.K1 / ZDK;                   // phase-1 tiles per q
  constexpr int T2 = (ZM / 2) / ZDK;           // phase-2 tiles per q: 8 rows of each m1 half at a time
  const int TQ = T1 + T2, TT = a.Q * TQ;

  // the LDS-DMA requests of the next tile not yet asked for: a cursor with running, wave-uniform pointers, and only the
  // four waves of the first m1 half issue them, each for both halves (see k_zip_f32 for both choices).
  const double* const rE0 = E + (int64_t)(2 * ub) * a.ldE;
  const double* rE = rE0;
  const double* rX = X + (int64_t)(2 * ub) * a.ldXk;
  const double* rY = Y + (int64_t)(2 * ub) * a.ldYm;
  const int offE = 2 * lane, offX = (lane >> 5) * (int)a.ldXk + 2 * (lane & 31);
  const int64_t stepE = (int64_t)ZDK * a.ldE, stepX = (int64_t)ZDK * a.ldXk, stepY = (int64_t)ZDK * a.ldYm;
  const int64_t nextX = a.ldXq - (int64_t)a.K1 * a.ldXk, nextY = a.ldYq - (int64_t)(ZM / 2) * a.ldYm;
  const int64_t halfY = (int64_t)(ZM / 2) * a.ldYm;
  int rq_s = 0, rq_left = TT;
  auto request_issue = [&](int stage) {
    double* st = smem + stage * ZDSTG;
    if (rq_s < T1) {             // rows 2 ub, 2 ub + 1 of E (two requests of 128 doubles each) and of Xq (both rows in one request)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int c = 0; c < 2; ++c) glds16d(rE + i * a.ldE + 128 * c + offE, st + (2 * ub + i) * ZDROW + 128 * c);
      glds16d(rX + offX, st + ZDX0 + (2 * ub) * ZDU);
    } else {                     // rows 2 ub, 2 ub + 1 of both m1 halves of Yq
#pragma unroll
      for (int hf = 0; hf < 2; ++hf)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int c = 0; c < 2; ++c)
            glds16d(rY + hf * halfY + i * a.ldYm + 128 * c + offE, st + (hf * ZDK + 2 * ub + i) * ZDROW + 128 * c);
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

  f64x4 acc1[8], acc2[16];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc1[i][e] = 0.0;
#pragma unroll
  for (int i = 0; i < 16; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc2[i][e] = 0.0;

#pragma unroll
  for (int i = 0; i < ZDST - 1; ++i) {
    if (kh == 0) request_issue(i);
    request_step();
  }
  double pve = 0.0;
  if (a.partE) {
    const double* __restrict__ pr = a.partE + (size_t)r * a.strideE;
    pve = pr[min(lane, a.PE - 1)];
    if (a.PE > 64)
      for (int i = lane + 64; i < a.PE; i += 64) pve += pr[i];
  }
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_waitcnt(0x0F70);          // vmcnt(0): once per pair - no need to count
  __builtin_amdgcn_s_barrier();
  CTN_ZIP_STAMP(1);

  int st_cur = 0, st_nxt = 1, st_req = ZDST - 1, t = 0;
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
    st_nxt = st_nxt == ZDST - 1 ? 0 : st_nxt + 1;
    ++t;
  };
  const int offA = h * ZDROW + kh * (ZM / 2) + l15;                          // E image [k1][272]
  const int offB = ZDX0 + h * ZDU + ub * 16 + l15;                           // Xq image [k1][64]
  const int offY = (kh * ZDK + h) * ZDROW + 4 * (l15 & 3) + (l15 >> 2);      // Yq image [half][8 rows][272], n2(i) of the header
  double fa[2][8], fb[2];

  for (int q = 0; q < a.Q; ++q) {
    // ---- phase 1: Tq[m1 half kh, u-block ub] = sum_k1 E[k1][m1] Xq[k1][u] ------------------------------------
    for (int s = 0; s < T1; ++s) {
      const double* cA = smem + st_cur * ZDSTG + offA;
      const double* cB = smem + st_cur * ZDSTG + offB;
#pragma unroll
      for (int i = 0; i < 8; ++i) fa[0][i] = cA[16 * i];
      fb[0] = cB[0];
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {           // k-step kk: rows 4 kk + h of the tile
        if (kk == 0) {
#pragma unroll
          for (int i = 0; i < 8; ++i) fa[1][i] = cA[4 * ZDROW + 16 * i];
          fb[1] = cB[4 * ZDU];
        }
        if (kk == 1) request_step();             // the cursor moves on in the shadow of this k-step's MFMAs
#pragma unroll
        for (int i = 0; i < 8; ++i)
          acc1[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[kk][i], fb[kk], acc1[i], 0, 0, 0);     // D1[m1][u]
        if (kk == 0) middle();
      }
      advance();
    }
    // ---- phase 2: E'[u-block ub, :] += sum over this half's m1 of Tq[m1][u] Yq[m1][n2] -------------------------
#pragma unroll
    for (int ms = 0; ms < T2; ++ms) {
      // rows 8 ms .. 8 ms + 7 of the half = registers e = 2 (ms & 1), + 1 of accumulator block ms / 2; a group of 8 MFMAs
      // is half a k-step: gp = (k-step, n2 half)
      const double* cY = smem + st_cur * ZDSTG + offY;
#pragma unroll
      for (int j = 0; j < 8; ++j) fa[0][j] = cY[16 * j];
#pragma unroll
      for (int gp = 0; gp < 4; ++gp) {
        const int c = gp & 1, nx = c ^ 1;
        if (gp + 1 < 4) {
#pragma unroll
          for (int j = 0; j < 8; ++j) fa[nx][j] = cY[4 * ((gp + 1) >> 1) * ZDROW + 16 * (8 * ((gp + 1) & 1) + j)];
        }
        const double tq = acc1[ms / 2][2 * (ms & 1) + (gp >> 1)];
        if (gp == 2) request_step();
#pragma unroll
        for (int j = 0; j < 8; ++j)
          acc2[8 * (gp & 1) + j] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[c][j], tq, acc2[8 * (gp & 1) + j], 0, 0, 0);   // D2^T[n2][u]
        if (gp == 1) middle();
      }
      advance();
    }
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc1[i][e] = 0.0;
  }
#ifdef CTN_STAMPS
  if (a.dbg && tid == 0) {
    a.dbg[(size_t)pid * 8 + 2] = __builtin_amdgcn_s_memtime();
    a.dbg[(size_t)pid * 8 + 5] = wait_vm;
    a.dbg[(size_t)pid * 8 + 6] = wait_bar;
  }
  if (a.dbg && tid == 448) a.dbg[(size_t)pid * 8 + 7] = wait_vm + wait_bar;
#endif

  // ---- the two m1 halves meet: half kh finishes n2 blocks 8 kh .. 8 kh + 7 and hands the other eight over, four per
  // round through the ring's LDS (a wave's area: 4 blocks x 64 lanes x 4 doubles = 8 KiB): first half + second half,
  // whichever wave adds
#pragma unroll
  for (int round = 0; round < 4; ++round) {
    __builtin_amdgcn_s_waitcnt(0xC07F);        // lgkmcnt(0): this wave's own LDS reads are done
    __builtin_amdgcn_s_barrier();              // ... and everybody's: the area is free
    if (kh != (round >> 1)) {
      double2* xo = reinterpret_cast<double2*>(smem + w * 1024) + lane;
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int p = 0; p < 2; ++p) xo[(2 * i + p) * 64] = make_double2(acc2[4 * round + i][2 * p], acc2[4 * round + i][2 * p + 1]);
    }
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_s_barrier();
    if (kh == (round >> 1)) {
      const double2* xi = reinterpret_cast<const double2*>(smem + (w ^ 4) * 1024) + lane;
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int p = 0; p < 2; ++p) {
          const double2 o = xi[(2 * i + p) * 64];
          const double m0 = acc2[4 * round + i][2 * p], m1 = acc2[4 * round + i][2 * p + 1];
          acc2[4 * round + i][2 * p] = kh == 0 ? m0 + o.x : o.x + m0;
          acc2[4 * round + i][2 * p + 1] = kh == 0 ? m1 + o.y : o.y + m1;
        }
    }
  }
  CTN_ZIP_STAMP(4);

  // ---- epilogue: lazy rescale by E's producer (X, Y are inputs), 16-byte stores, abs-sum partial ---------------
  pve = lane < a.PE ? pve : 0.0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) pve += __shfl_xor(pve, o, 64);
  const double scE = (a.partE && pve > a.min_norm) ? pve / a.numelE : 1.0;   // = producer_scale<double>()
  const double iE = 1.0 / scE;
  double asum = 0.0;
  double* __restrict__ row = C + (int64_t)(u0 + 16 * ub + l15) * a.ldC + 4 * h;
#pragma unroll
  for (int nb = 0; nb < 16; ++nb) {
    if (kh == (nb >> 3)) {                     // the n2 blocks this wave finished: n2 = 16 nb + 4 h + e
      double2 v0, v1;
      v0.x = acc2[nb][0] * iE; v0.y = acc2[nb][1] * iE; v1.x = acc2[nb][2] * iE; v1.y = acc2[nb][3] * iE;
      *reinterpret_cast<double2*>(row + 16 * nb) = v0;
      *reinterpret_cast<double2*>(row + 16 * nb + 2) = v1;
      asum += (fabs(v0.x) + fabs(v0.y)) + (fabs(v1.x) + fabs(v1.y));
    }
  }
  double part = asum;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
  if (lane == 0) red[w] = part;
  __builtin_amdgcn_s_waitcnt(0xC07F);
  __builtin_amdgcn_s_barrier();
  if (tid == 0) {
    double tot = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) tot += red[i];
    a.partC[(size_t)r * a.partC_stride + t_] = tot;
  }
  CTN_ZIP_STAMP(3);
}

}  // namespace ctn
