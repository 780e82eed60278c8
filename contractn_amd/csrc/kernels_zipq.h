// kernels_zipq.h - the zipper site pair of kernels_zip.h with two physical legs per pass over E and one wave per SIMD.
// Part of the gfx950 contraction engine (see engine.hip for the overview).
#pragma once
#include "kernels_zip.h"
#include "kernels_zipq_asm.inc"

namespace ctn {

// ---------------------------------------------------------------------------
// K-zipq-f32.  The same site pair as k_zip_f32 (same ZipArgs, grid, 128 values of u per workgroup, E' layout, one
// abs-sum partial per workgroup, lazy rescale by E's producer, XCD remap), in another shape: 4 waves, one per SIMD, each
// with the whole 512-register file.  Wave ub owns u-block ub (32 values of u) for ALL 256 m1 and all 256 n2, so the two
// m1 halves of k_zip_f32 never have to meet, and the physical legs go in pairs:
//
//   phase 1, legs (q, q + 1):  T_q, T_q+1 [256 m1 x 32 u] together in 16 accumulator blocks - the 256 AGPRs.  A k-step
//            reads 8 E fragments + 2 X fragments for 16 MFMAs (0.625 per MFMA; k_zip_f32: 1.25), and E comes from L2
//            and from LDS once per PAIR of legs.  Tile: 16 rows of k1 - E 16 KiB + X_q 8 KiB + X_q+1 8 KiB.
//   phase 2, q then q + 1:     E'^T [256 n2 x 32 u] += Y_q^T T_q over all 256 m1 in 8 accumulator blocks (128 VGPRs); the
//            B operand of a k-step is a phase-1 accumulator register read straight from the AGPR file (the layout
//            argument at the head of kernels_zip.h).  Tile: 32 rows of Y_q - 32 KiB, one accumulator block.
//
// Every tile is 128 MFMAs, one ring stage and one barrier: (K1 / 16 + 16) tiles per pair of legs.  The tiles are the
// generated asm statements of kernels_zipq_asm.inc (tools/gen_zipq_asm.py describes their schedule): the compiler can
// neither keep 384 accumulators in place (plain C++: 517 spilled registers) nor leave the AGPR blocks alone, so the
// phase-1 accumulators are named literally (a[0:255], listed as clobbers) and everything else is an operand.  What the
// kernel does between two statements is the ring bookkeeping and the cursor of the LDS-DMA requests, all scalar.
//
// Conditions: those of k_zip_f32, Q even, and every operand's span below 2^31 bytes (32-bit request offsets) - engine.hip.
// ---------------------------------------------------------------------------
constexpr int ZQT2 = 16;   // phase-2 tiles per pair of legs: 8 accumulator blocks x 2 legs

__global__ __launch_bounds__(256, 1) void k_zipq_f32(ZipArgs a) {
  __shared__ __attribute__((aligned(16))) float smem[ZST * ZSTG + 16];
  double* red = reinterpret_cast<double*>(smem + ZST * ZSTG);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int ub = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, h = lane >> 5;
  const int pid = zipq_pid(blockIdx.x, gridDim.x);
  const int per = a.U / ZU;                    // workgroups per replica
  const int r = pid / per;
  const int t_ = pid - r * per;
  const int u0 = t_ * ZU;
  CTN_ZIP_STAMP(0);
  void* const* tp = a.ptrs + (size_t)r * a.n_tensors;
  const float* __restrict__ E = (const float*)tp[a.idE];
  const float* __restrict__ X = (const float*)tp[a.idX] + u0;
  const float* __restrict__ Y = (const float*)tp[a.idY];
  float* __restrict__ C = (float*)tp[a.idC];

  const int T1 = a.K1 / ZK;                    // phase-1 tiles per pair of legs
  const int TP = T1 + ZQT2, NP = a.Q / 2;

  // ---- the LDS-DMA requests of a tile: 8 per wave, 1 KiB each, into [8 ub, 8 ub + 8) KiB of the stage.  A request is
  // base pointer (scalar) + 32-bit byte offset (vector: the cursor's scalar part + the lane's own); requests 0-3 walk
  // offset ra off base sa by ia, requests 4-7 walk rb off sb by ib1, ib2, ib1:
  //   phase-1 tile: E rows 4 ub .. + 3; rows 4 ub .. + 3 of X_q, then of X_q+1, two rows per request (lanes 0-31 / 32-63)
  //   phase-2 tile: rows 8 ub .. + 7 of the 32 rows of Y_q
  // The cursor (rq_p, rq_s) = (pair of legs, tile within the pair) runs two tiles ahead of the MFMAs and wraps to the
  // first tile behind the last one: the two tiles requested past the end are the first two again - in bounds, never read.
  const unsigned ldE4 = (unsigned)a.ldE * 4u, ldXk4 = (unsigned)a.ldXk * 4u, ldXq4 = (unsigned)a.ldXq * 4u;
  const unsigned ldYm4 = (unsigned)a.ldYm * 4u, ldYq4 = (unsigned)a.ldYq * 4u;
  const unsigned laneE = 16u * lane, laneX = (unsigned)h * ldXk4 + 16u * l31;
  int rq_p = 0, rq_s = 0;
  const float *sa, *sb;
  unsigned ra, rb, ia, ib1, ib2;
  auto request_setup = [&]() {                 // (plain selects: everything but the lane's own offset stays scalar)
    const bool p1 = rq_s < T1;
    const int j = rq_s - T1;
    const unsigned k1 = (unsigned)(rq_s * ZK + 4 * ub);
    const unsigned cE = k1 * ldE4, cX = (unsigned)(2 * rq_p) * ldXq4 + k1 * ldXk4;
    const unsigned cY = (unsigned)(2 * rq_p + (j >> 3)) * ldYq4 + (unsigned)(32 * (j & 7) + 8 * ub) * ldYm4;
    sa = p1 ? E : Y;
    sb = p1 ? X : Y;
    ra = (p1 ? cE : cY) + laneE;
    rb = p1 ? cX + laneX : cY + 4u * ldYm4 + laneE;
    ia = p1 ? ldE4 : ldYm4;
    ib1 = p1 ? 2u * ldXk4 : ldYm4;
    ib2 = p1 ? ldXq4 - 2u * ldXk4 : ldYm4;
    ++rq_s;
    const bool wrap = rq_s == TP;
    rq_s = wrap ? 0 : rq_s;
    rq_p = wrap ? (rq_p + 1 == NP ? 0 : rq_p + 1) : rq_p;
  };
  auto request_issue = [&](int stage) {        // the prologue's two tiles; the main loop's requests are in the asm tiles
    float* st = smem + stage * ZSTG + ub * 2048;
    const char *ca = reinterpret_cast<const char*>(sa), *cb = reinterpret_cast<const char*>(sb);
    unsigned oa = ra, ob = rb;
#pragma unroll
    for (int i = 0; i < 4; ++i) { glds16(reinterpret_cast<const float*>(ca + oa), st + i * 256); oa += ia; }
#pragma unroll
    for (int i = 0; i < 4; ++i) { glds16(reinterpret_cast<const float*>(cb + ob), st + (4 + i) * 256); ob += i == 1 ? ib2 : ib1; }
  };

  f32x16 acc2[8];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc2[i][e] = 0.f;

#pragma unroll
  for (int i = 0; i < ZST - 1; ++i) {
    request_setup();
    request_issue(i);
  }
  double pve = 0.0;
  if (a.partE) {
    const double* __restrict__ pr = a.partE + (size_t)r * a.strideE;
    pve = pr[min(lane, a.PE - 1)];
    if (a.PE > 64)
      for (int i = lane + 64; i < a.PE; i += 64) pve += pr[i];
  }
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_waitcnt(0x0F70);          // vmcnt(0)
  __builtin_amdgcn_s_barrier();
  CTN_ZIP_STAMP(1);

  // fragment double buffer: phase 1 f[10 b + mb] = E block mb, f[10 b + 8 + leg] = X; phase 2 f[10 b + nb] = Y block nb
  float f[20];
  {
    const float* cA = smem + h * 256 + l31;                      // first tile, k-step 0: row h of group 0
    const float* cB = smem + 1024 + h * 128 + ub * 32 + l31;
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = cA[32 * i];
    f[8] = cB[0];
    f[9] = cB[512];
#pragma unroll
    for (int i = 10; i < 20; ++i) f[i] = 0.f;
  }
  // this lane's fragment bases inside a stage (bytes): E (row h of a group of 4), X (behind the group's 4 KiB of E), Y (row 4 h)
  const unsigned smem0 = lds_addr(smem);
  const unsigned fA = (unsigned)(h * 1024 + l31 * 4), fB = (unsigned)(4096 + h * 512 + ub * 128 + l31 * 4);
  const unsigned fY = (unsigned)(h * 4096 + l31 * 4);
  int st_cur = 0, st_nxt = 1, st_req = ZST - 1;

#define CTN_ZQ_TILE(TEXT)                                                                                              \
  {                                                                                                                    \
    request_setup();                                                                                                   \
    const unsigned bc = smem0 + (unsigned)st_cur * (ZSTG * 4u), bn = smem0 + (unsigned)st_nxt * (ZSTG * 4u);           \
    const unsigned vA = bc + fA, vB = bc + fB, vY = bc + fY, nA = bn + fA, nB = bn + fB, nY = bn + fY;                  \
    const unsigned m0b = smem0 + (unsigned)st_req * (ZSTG * 4u) + (unsigned)ub * 8192u;                                \
    unsigned keep;                                                                                                     \
    __builtin_amdgcn_sched_barrier(0);                                                                                 \
    asm volatile(TEXT                                                                                                  \
                 : [c0] "+v"(acc2[0]), [c1] "+v"(acc2[1]), [c2] "+v"(acc2[2]), [c3] "+v"(acc2[3]), [c4] "+v"(acc2[4]), \
                   [c5] "+v"(acc2[5]), [c6] "+v"(acc2[6]), [c7] "+v"(acc2[7]), [f0] "+v"(f[0]), [f1] "+v"(f[1]),       \
                   [f2] "+v"(f[2]), [f3] "+v"(f[3]), [f4] "+v"(f[4]), [f5] "+v"(f[5]), [f6] "+v"(f[6]),                \
                   [f7] "+v"(f[7]), [f8] "+v"(f[8]), [f9] "+v"(f[9]), [f10] "+v"(f[10]), [f11] "+v"(f[11]),            \
                   [f12] "+v"(f[12]), [f13] "+v"(f[13]), [f14] "+v"(f[14]), [f15] "+v"(f[15]), [f16] "+v"(f[16]),      \
                   [f17] "+v"(f[17]), [f18] "+v"(f[18]), [f19] "+v"(f[19]), [ra] "+v"(ra), [rb] "+v"(rb),              \
                   [keep] "=&s"(keep)                                                                                  \
                 : [vA] "v"(vA), [vB] "v"(vB), [vY] "v"(vY), [nA] "v"(nA), [nB] "v"(nB), [nY] "v"(nY), [sa] "s"(sa),   \
                   [sb] "s"(sb), [ia] "s"(ia), [ib1] "s"(ib1), [ib2] "s"(ib2), [m0b] "s"(m0b)                          \
                 : "memory", "scc", CTN_ZQ_CLOBBERS);                                                                  \
    __builtin_amdgcn_sched_barrier(0);                                                                                 \
    st_req = st_cur;                                                                                                   \
    st_cur = st_nxt;                                                                                                   \
    st_nxt = st_nxt == ZST - 1 ? 0 : st_nxt + 1;                                                                       \
  }

  for (int p = 0; p < NP; ++p) {
    CTN_ZQ_TILE(CTN_ZQ_P1_FIRST)
    for (int s = 1; s + 1 < T1; ++s) CTN_ZQ_TILE(CTN_ZQ_P1_MID)
    CTN_ZQ_TILE(CTN_ZQ_P1_LAST)
    CTN_ZQ_TILE(CTN_ZQ_P2_0_0) CTN_ZQ_TILE(CTN_ZQ_P2_0_1) CTN_ZQ_TILE(CTN_ZQ_P2_0_2) CTN_ZQ_TILE(CTN_ZQ_P2_0_3)
    CTN_ZQ_TILE(CTN_ZQ_P2_0_4) CTN_ZQ_TILE(CTN_ZQ_P2_0_5) CTN_ZQ_TILE(CTN_ZQ_P2_0_6) CTN_ZQ_TILE(CTN_ZQ_P2_0_7)
    CTN_ZQ_TILE(CTN_ZQ_P2_1_0) CTN_ZQ_TILE(CTN_ZQ_P2_1_1) CTN_ZQ_TILE(CTN_ZQ_P2_1_2) CTN_ZQ_TILE(CTN_ZQ_P2_1_3)
    CTN_ZQ_TILE(CTN_ZQ_P2_1_4) CTN_ZQ_TILE(CTN_ZQ_P2_1_5) CTN_ZQ_TILE(CTN_ZQ_P2_1_6) CTN_ZQ_TILE(CTN_ZQ_P2_1_7)
  }
#undef CTN_ZQ_TILE
  // the last MFMAs' results -> their first reader below (18 wait states; nothing pads behind an asm statement), and the
  // two tiles requested past the end have to land before the workgroup gives its LDS back
  asm volatile("s_nop 15\n\ts_nop 7\n\ts_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
#ifdef CTN_STAMPS
  if (a.dbg && tid == 0) {
    const unsigned long long now = __builtin_amdgcn_s_memtime();
    a.dbg[(size_t)pid * 8 + 2] = now;
    a.dbg[(size_t)pid * 8 + 4] = now;          // (no hand-over: the slot k_zip_f32 stamps behind it)
  }
#endif

  // ---- epilogue: lazy rescale by E's producer (X, Y are inputs), 16-byte stores, abs-sum partial.  The partial is
  // added up as k_zip_f32 does - n2 blocks 0-3 and 4-7 of a lane apart in fp32, then float64 in that kernel's wave order
  pve = lane < a.PE ? pve : 0.0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) pve += __shfl_xor(pve, o, 64);
  const float nE = (float)pve;
  const float scE = (a.partE && nE > (float)a.min_norm) ? nE / (float)a.numelE : 1.f;
  const float iE = 1.0f / scE;
  float asum[2] = {0.f, 0.f};
  float* __restrict__ row = C + (int64_t)(u0 + 32 * ub + l31) * a.ldC + 4 * h;
#pragma unroll
  for (int nb = 0; nb < 8; ++nb) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float4 v;
      v.x = acc2[nb][4 * g + 0] * iE; v.y = acc2[nb][4 * g + 1] * iE; v.z = acc2[nb][4 * g + 2] * iE; v.w = acc2[nb][4 * g + 3] * iE;
      *reinterpret_cast<float4*>(row + 32 * nb + 8 * g) = v;
      asum[nb >> 2] += (fabsf(v.x) + fabsf(v.y)) + (fabsf(v.z) + fabsf(v.w));
    }
  }
#pragma unroll
  for (int hf = 0; hf < 2; ++hf) {
    double part = (double)asum[hf];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
    if (lane == 0) red[4 * hf + ub] = part;
  }
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
