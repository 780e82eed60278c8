// kernels_cmfma.h - k_cmfma_f32: a complex x complex step (the S step and the real GEMM behind it) as one launch
// Part of the gfx950 contraction engine (see engine.hip for the overview).
#pragma once
#include "cplx_match.h"
#include "kernel_args.h"
#include "kernels_mfma.h"

namespace ctn {

// ---------------------------------------------------------------------------
// A complex x complex step of a lowered complex network (einsum._complex_plan_cached) is two plan steps: the
// streaming step s-1 that contracts the 2 x 2 x 2 structure tensor S into the smaller operand,
//     mid[.., b, o] = sum_a S[a, b, o] small[.., a],
// and the real GEMM s over (shared labels, b) whose operands both have their unit-stride label on the pair leg - the
// 4-byte-gather form.  This kernel does both:
//     C[x, y, o] = sum_{k, a, b} S[a, b, o] small[x, k, a] big[k, y, b]
// reading `small` and `big` as what they are, arrays of (re, im) pairs, through pair-granular offset tables that
// cplx_match (cplx_match.h) derives from the tables of step s; `mid` never exists.  C goes where step s writes it.
//
// Tile: CX_TX = 64 pairs of `small` (x: the side of the GEMM that carries o) by CX_TY = 128 elements of `big`'s free
// group, both components of the result: 128 x 128 real outputs, 4 waves (2 x 2), a wave 32 x 64 x 2: 2 x 2 = 4
// accumulators of v_mfma_f32_32x32x2_f32 (64 registers).  k-tile: CX_BK = 16 pairs (32 real k), register-staged
// (global -> registers -> LDS), double-buffered, one barrier per k-tile, as k_mfma_f32.
//
// LDS images are INTERLEAVED: [k][rows + 1] of (re, im), written with one ds_write_b64 per 8-byte global load and read
// with one ds_read_b64 per fragment pair.  By the LDS bank rules of CDNA4 (64 banks of 4 bytes; a ds_read_b64 is served
// in two halves of 32 lanes over all 64 banks, a ds_write_b64 in groups of 16 lanes over 32): a
// ds_read_b64 of 32 consecutive rows covers the 64 banks once - conflict-free, 2 LDS cycles for 8 bytes a lane, twice
// the bytes per cycle of the two ds_read_b32 that separate re / im images need - and the write side saves the
// de-interleave (one 6-cycle ds_write_b64 against two 4-cycle ds_write_b32).  The odd row length (rows + 1 pairs)
// keeps the ds_write_b64 of the k-fast loader conflict-free (consecutive lanes = consecutive k: a stride of
// 2 (rows + 1) dwords = 2 mod 32, so a 16-lane group covers the 32 banks once; with an even row length all 16 lanes
// would meet on two banks); the row-fast loader writes consecutive pairs, conflict-free either way.
//
// Loads are 8 bytes a lane from an operand that is an array of pairs (every network input); an operand whose leg has
// another stride (an earlier step's result: [rows][o][columns]) gives its two components as two 4-byte loads, which
// are as well coalesced along the lanes.  Which index runs along the lanes is chosen per operand by the matcher: the k pairs
// when the operand is dense along them (KF = true: 16 lanes = one 128-byte line), else the rows.
//
// The widened fragment is formed in registers after the LDS read, with whatever S holds (its eight values arrive by
// wave-uniform loads): mid[b][o] = S[0][b][o] * x_re + S[1][b][o] * x_im (-ffp-contract=off: two products and a sum,
// exact for the true S, whose entries are 0 and +-1), then acc[o] += mid[b][o] * big_b for b = 0, 1: four MFMAs per
// (row block, column block) and pair of k, two accumulator sets and none for the subtraction.
// Epilogue as k_mfma_f32: v = (acc * iS) * iB with the scales of `small` and `big` from their producers' partials,
// stores through C's offset tables (8 bytes - both components - where o is unit-stride in C and everything else
// even, else two 4-byte stores), one abs-sum partial per workgroup in a fixed order: no atomics.
// ---------------------------------------------------------------------------
struct CplxArgs {
  const int32_t *txr, *txk;   // `small`: offsets of the x pairs (padded to CX_TX) and of the k pairs (padded, + 2 tiles)
  const int32_t *tyn, *tyk;   // `big`: offsets of its free entries (padded to CX_TY) and of the k pairs
  const int32_t *tcx, *tcy;   // C: offset of (x, o = 0) and of y
  void* const* ptrs;
  const double *partX, *partY;   // abs-sum partials of the producers of `small` and `big` (nullptr: scale 1)
  double* partC;
  double numelX, numelY, min_norm;
  int32_t Mx, Ny, Kc;            // pairs of `small`'s free group, entries of `big`'s, contracted pairs
  int32_t idX, idY, idS, idC, n_tensors;
  int32_t PX, PY, strideX, strideY, partC_stride;
  int32_t tiles_x, tiles_y, blocks_per_replica, R;
  int32_t sa, sb, so;            // strides of S along (the leg of `small`, the leg of `big`, o)
  int32_t sO;                    // stride of o in C
  int32_t c_vec2;                // 8-byte stores of (o = 0, o = 1) allowed
  int32_t legx, legy;            // strides of the legs of `small` and `big`: 1 = (re, im) pairs, one 8-byte load each
};

// Stages one ROWS x BK tile of pairs per k-step.  KF: consecutive lanes take consecutive k (else consecutive rows).
template <bool KF, int BK, int ROWS>
struct CplxLoader {
  static constexpr int NV = ROWS * BK / 256;     // pairs staged per thread
  static constexpr int KPP = 256 / ROWS;         // row-fast: k-rows covered per pass
  static constexpr int RPP = 256 / BK;           // k-fast: rows covered per pass
  static constexpr int LD = ROWS + 1;            // pairs per k-row of the LDS image
  static constexpr int kSize = BK * LD;          // pairs
  static_assert(NV >= 1 && 256 % ROWS == 0 && 256 % BK == 0, "tile shape");
  float2 v[NV];
  int kofs[KF ? 1 : NV];    // k-table entries of the NEXT tile to load
  int offr[KF ? NV : 1];
  bool okr[KF ? NV : 1];

  __device__ __forceinline__ void init(const int32_t* __restrict__ tr, int m0, int M, int tid) {
    if (KF) {
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int gm = m0 + tid / BK + RPP * i;
        offr[i] = tr[gm];
        okr[i] = gm < M;
      }
    } else {
      const int gm = m0 + (tid % ROWS);
      offr[0] = tr[gm];
      okr[0] = gm < M;
    }
  }
  __device__ __forceinline__ void tab(const int32_t* __restrict__ tk, int k0, int tid) {
    if (KF) {
      kofs[0] = tk[k0 + (tid % BK)];
    } else {
#pragma unroll
      for (int i = 0; i < NV; ++i) kofs[i] = tk[k0 + tid / ROWS + KPP * i];
    }
  }
  // unconditional: padded tables keep every address inside the tensor; masked in store()
  // `leg` (wave-uniform): 1 = the operand is an array of pairs; else its two components lie `leg` elements apart
  __device__ __forceinline__ void load(const float* __restrict__ base, int leg) {
    if (leg == 1) {
#pragma unroll
      for (int i = 0; i < NV; ++i) v[i] = *reinterpret_cast<const float2*>(base + offr[KF ? i : 0] + kofs[KF ? 0 : i]);
    } else {
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const float* p = base + offr[KF ? i : 0] + kofs[KF ? 0 : i];
        v[i] = make_float2(p[0], p[leg]);
      }
    }
  }
  template <bool FULL>
  __device__ __forceinline__ void store(float2* __restrict__ s, int k0, int K, int tid) const {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int kr = KF ? tid % BK : tid / ROWS + KPP * i;
      const int row = KF ? tid / BK + RPP * i : tid % ROWS;
      const bool in = FULL || (okr[KF ? i : 0] && (k0 + kr) < K);
      s[kr * LD + row] = in ? v[i] : make_float2(0.f, 0.f);
    }
  }
};

template <bool KFX, bool KFY, bool FULL>
__device__ __forceinline__ void cmfma_mainloop(CplxLoader<KFX, CX_BK, CX_TX>& lx, CplxLoader<KFY, CX_BK, CX_TY>& ly,
                                               const float* __restrict__ X, const float* __restrict__ Y,
                                               const int32_t* __restrict__ txk, const int32_t* __restrict__ tyk, int K, int legx,
                                               int legy, float2* sX, float2* sY, const float (&S)[2][2][2],
                                               f32x16 (&acc)[2][2], int tid) {
  using LX = CplxLoader<KFX, CX_BK, CX_TX>;
  using LY = CplxLoader<KFY, CX_BK, CX_TY>;
  constexpr int SZX = LX::kSize, SZY = LY::kSize;
  const int lane = tid & 63, w = tid >> 6;
  const int wm = (w >> 1) * 32, wn = (w & 1) * 64;
  const int l31 = lane & 31, h = lane >> 5;

  const int nkt = (K + CX_BK - 1) / CX_BK;
  lx.tab(txk, 0, tid);
  ly.tab(tyk, 0, tid);
  lx.load(X, legx);
  ly.load(Y, legy);
  lx.tab(txk, CX_BK, tid);
  ly.tab(tyk, CX_BK, tid);
  lx.template store<FULL>(sX, 0, K, tid);
  ly.template store<FULL>(sY, 0, K, tid);
  __syncthreads();

  const int fx = h * LX::LD + wm + l31;          // fragment bases (pairs): row l31 of the wave's block, k = 2 kk + h
  const int fy = h * LY::LD + wn + l31;
  for (int kt = 0; kt < nkt; ++kt) {
    const int cur = kt & 1;
    const bool more = kt + 1 < nkt;
    if (more) {
      lx.load(X, legx);
      ly.load(Y, legy);
      lx.tab(txk, (kt + 2) * CX_BK, tid);
      ly.tab(tyk, (kt + 2) * CX_BK, tid);
    }
    __builtin_amdgcn_sched_barrier(0);  // global loads stay in front of the MFMA phase
    const float2* cX = sX + cur * SZX;
    const float2* cY = sY + cur * SZY;
    float2 x[2], y[2][2];
    x[0] = cX[fx];
    y[0][0] = cY[fy];
    y[0][1] = cY[fy + 32];
#pragma unroll
    for (int kk = 0; kk < CX_BK / 2; ++kk) {
      const int c = kk & 1, nx = c ^ 1;
      if (kk + 1 < CX_BK / 2) {          // the LDS reads of step kk + 1 issue ahead of the MFMAs of step kk
        x[nx] = cX[fx + (kk + 1) * 2 * LX::LD];
        y[nx][0] = cY[fy + (kk + 1) * 2 * LY::LD];
        y[nx][1] = cY[fy + (kk + 1) * 2 * LY::LD + 32];
      }
      // the widened fragment: mid[b][o] = S[0][b][o] x_re + S[1][b][o] x_im
      float mid[2][2];
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int o = 0; o < 2; ++o) mid[b][o] = S[0][b][o] * x[c].x + S[1][b][o] * x[c].y;
#pragma unroll
      for (int o = 0; o < 2; ++o)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          acc[o][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(mid[0][o], y[c][j].x, acc[o][j], 0, 0, 0);
          acc[o][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(mid[1][o], y[c][j].y, acc[o][j], 0, 0, 0);
        }
    }
    __builtin_amdgcn_sched_barrier(0);  // the staged tile is consumed only after the MFMA phase
    if (more) {
      lx.template store<FULL>(sX + (cur ^ 1) * SZX, (kt + 1) * CX_BK, K, tid);
      ly.template store<FULL>(sY + (cur ^ 1) * SZY, (kt + 1) * CX_BK, K, tid);
    }
    __syncthreads();
  }
}

template <bool KFX, bool KFY>
__global__ __launch_bounds__(256, 2) void k_cmfma_f32(CplxArgs a) {
  using LX = CplxLoader<KFX, CX_BK, CX_TX>;
  using LY = CplxLoader<KFY, CX_BK, CX_TY>;
  __shared__ __attribute__((aligned(16))) float2 smem[2 * LX::kSize + 2 * LY::kSize];
  __shared__ double red[4];
  float2* sX = smem;
  float2* sY = smem + 2 * LX::kSize;

  const int tid = threadIdx.x;
  // XCD-aware remap, as k_mfma_f32: each XCD gets a contiguous range of tiles
  const int pid = zipq_pid(blockIdx.x, gridDim.x);
  const int r = pid / a.blocks_per_replica;
  const int t = pid - r * a.blocks_per_replica;
  const int m0 = (t / a.tiles_y) * CX_TX;
  const int n0 = (t % a.tiles_y) * CX_TY;

  void* const* tp = a.ptrs + (size_t)r * a.n_tensors;
  const float* __restrict__ X = (const float*)tp[a.idX];
  const float* __restrict__ Y = (const float*)tp[a.idY];
  const float* __restrict__ Sp = (const float*)tp[a.idS];
  float* __restrict__ C = (float*)tp[a.idC];

  LX lx;
  LY ly;
  lx.init(a.txr, m0, a.Mx, tid);
  ly.init(a.tyn, n0, a.Ny, tid);
  float S[2][2][2];
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int o = 0; o < 2; ++o) S[p][b][o] = Sp[p * a.sa + b * a.sb + o * a.so];
  const float scX = producer_scale<float>(a.partX, a.PX, a.strideX, a.numelX, a.min_norm, r);
  const float scY = producer_scale<float>(a.partY, a.PY, a.strideY, a.numelY, a.min_norm, r);

  const int lane = tid & 63, w = tid >> 6;
  const int wm = (w >> 1) * 32, wn = (w & 1) * 64;
  const int l31 = lane & 31, h = lane >> 5;

  f32x16 acc[2][2];   // [o][column block]
#pragma unroll
  for (int o = 0; o < 2; ++o)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[o][j][e] = 0.f;

  // FULL: the tile lies completely inside Mx x Ny and Kc is a multiple of the k-tile -> no masking
  const bool full = (m0 + CX_TX <= a.Mx) && (n0 + CX_TY <= a.Ny) && (a.Kc % CX_BK == 0);
  if (full) cmfma_mainloop<KFX, KFY, true>(lx, ly, X, Y, a.txk, a.tyk, a.Kc, a.legx, a.legy, sX, sY, S, acc, tid);
  else cmfma_mainloop<KFX, KFY, false>(lx, ly, X, Y, a.txk, a.tyk, a.Kc, a.legx, a.legy, sX, sY, S, acc, tid);

  // epilogue: lazy rescale, stores through C's offset tables straight from the accumulators (register e of a lane is
  // row (e & 3) + 8 (e >> 2) + 4 h, column l31 of the block), abs-sum partial
  const float iS = 1.0f / scX, iB = 1.0f / scY;
  float asum = 0.f;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int col = n0 + wn + j * 32 + l31;
    const bool cin = col < a.Ny;
    const int offy = a.tcy[col];          // (padded to the tile)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int row = m0 + wm + (e & 3) + 8 * (e >> 2) + 4 * h;
      const float v0 = (acc[0][j][e] * iS) * iB, v1 = (acc[1][j][e] * iS) * iB;
      if (cin && row < a.Mx) {
        float* dst = C + a.tcx[row] + offy;
        if (a.c_vec2) {
          *reinterpret_cast<float2*>(dst) = make_float2(v0, v1);
        } else {
          dst[0] = v0;
          dst[a.sO] = v1;
        }
        asum += fabsf(v0) + fabsf(v1);
      }
    }
  }
  const double tot = block_sum((double)asum, red);
  if (tid == 0) a.partC[(size_t)r * a.partC_stride + t] = tot;
}

}  // namespace ctn
