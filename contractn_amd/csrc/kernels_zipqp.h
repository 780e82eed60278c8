// kernels_zipqp.h - k_zipq_f32 (kernels_zipq.h) with a workgroup that walks several work items of ONE launch, and with
// tile seams that recompute nothing.  Part of the gfx950 contraction engine (see engine.hip for the overview).
#pragma once
#include "kernels_zipq.h"
#include "kernels_zipqp_asm.inc"
#include "zipq_items.h"

namespace ctn {

// ---------------------------------------------------------------------------
// K-zipqp-f32.  Per work item - one (replica, 128 values of u) - exactly k_zipq_f32: the same tiles in the same order, the
// same MFMAs, E' layout, lazy rescale and abs-sum partial, so the same bits.  Two things differ.
//
//   * The grid is min(items, CUs) (zipq_items.h) and workgroup pid walks items pid, pid + G, pid + 2 G, ...  No workgroup
//     waits for another.  The request cursor, two tiles ahead of the MFMAs, moves on from an item's last tile to the NEXT
//     ITEM's first two tiles (k_zipq_f32: back to its own first two, never read), so only a workgroup's first item has a
//     prologue; the last phase-2 tile already reads the next tile's first phase-1 fragments from the next ring stage.  An
//     item's epilogue runs between its last statement and the next item's first one, and its stores are waited for by
//     that item's first tile barrier, thousands of cycles later; the accumulators of E' are zeroed behind the stores.
//     The last item of a workgroup wraps to its own first tiles, as before.
//   * The statements advance the cursor themselves (%[ja], %[jb]: a fourth add per offset register).  Between two
//     statements the kernel re-bases it only where the KIND of the requested tile changes - the first Y tile of a pair of
//     legs, the second leg's first Y tile, the next pair's (or item's) first E / X tile: 3 of TP seams - and otherwise
//     rotates the ring indices.  Everything but the lane's own offset stays scalar (selects, never if / else).
//
// Conditions: those of k_zipq_f32.  a.n_items = R U / 128.
// ---------------------------------------------------------------------------
// An entry of the pointer table [R][n_tensors].  The table is written by host copies only, never by a kernel, so it is read
// through the constant address space: a scalar load wherever it stands - a plain load behind the first store of the
// kernel would be a vector load, and the seam would wait for it.
__device__ __forceinline__ void* zqp_ptr(void* const* tab, size_t i) {
  typedef const __attribute__((address_space(4))) unsigned long long* ctab_t;
  return reinterpret_cast<void*>(((ctab_t)tab)[i]);
}

__global__ __launch_bounds__(256, 1) void k_zipqp_f32(ZipArgs a) {
  __shared__ __attribute__((aligned(16))) float smem[ZST * ZSTG + 16];
  double* red = reinterpret_cast<double*>(smem + ZST * ZSTG);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int ub = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, h = lane >> 5;
  const int G = gridDim.x;
  const int pid = zipq_pid(blockIdx.x, G);
  const int per = a.U / ZU;                    // items per replica
  const int items = a.n_items;
  if (pid >= items) return;                    // (never: the grid is min(items, CUs))

  const int T1 = a.K1 / ZK;                    // phase-1 tiles per pair of legs
  const int NP = a.Q / 2;

  // ---- the request cursor (kernels_zipq.h: 8 requests per wave and tile, offsets ra / rb off the bases sa / sb).  The steps
  // of a tile's kind: ia, ib1, ib2 between the rows of a tile, ja, jb from its last row to the next tile's first.
  const unsigned ldE4 = (unsigned)a.ldE * 4u, ldXk4 = (unsigned)a.ldXk * 4u, ldXq4 = (unsigned)a.ldXq * 4u;
  const unsigned ldYm4 = (unsigned)a.ldYm * 4u, ldYq4 = (unsigned)a.ldYq * 4u;
  // this lane's offset in the first tile of a kind, its wave's rows included: E rows 4 ub .., X likewise, Y rows 8 ub ..
  const unsigned laneE = (unsigned)(4 * ub) * ldE4 + 16u * lane, laneX = (unsigned)(4 * ub + h) * ldXk4 + 16u * l31;
  const unsigned laneY = (unsigned)(8 * ub) * ldYm4 + 16u * lane;
  // (the steps are worked out where a kind begins, from copies the compiler cannot see through: hoisted out of the loops
  // they would be five more scalar registers alive across every statement, and the kernel has none to spare)
#define CTN_ZQP_P1_STEPS                                                                                               \
  {                                                                                                                    \
    unsigned e4 = ldE4, k4 = ldXk4, q4 = ldXq4;                                                                        \
    asm volatile("" : "+s"(e4), "+s"(k4), "+s"(q4));                                                                   \
    ia = e4;                                                                                                           \
    ib1 = 2u * k4;                                                                                                     \
    ib2 = q4 - 2u * k4;                                                                                                \
    ja = (unsigned)(ZK - 3) * e4;                                                                                      \
    jb = (unsigned)(ZK - 2) * k4 - q4; /* (mod 2^32) */                                                                \
  }

  // the first item's operands (every later item's arrive as the "next item" of the one before)
  int item = pid;
  const float *E, *X, *Y;
  float* C;
  {
    int r0, t0;
    zipq_item_rt(item, per, &r0, &t0);
    const size_t tp = (size_t)r0 * a.n_tensors;
    E = (const float*)zqp_ptr(a.ptrs, tp + a.idE);
    X = (const float*)zqp_ptr(a.ptrs, tp + a.idX) + t0 * ZU;
    Y = (const float*)zqp_ptr(a.ptrs, tp + a.idY);
    C = (float*)zqp_ptr(a.ptrs, tp + a.idC);
  }
  const float mnf = (float)a.min_norm, nef = (float)a.numelE;
#ifdef CTN_STAMPS
  if (a.dbg && tid == 0) a.dbg[(size_t)item * 8 + 0] = __builtin_amdgcn_s_memtime();
#endif

  const float *sa = E, *sb = X;
  unsigned ra = laneE, rb = laneX;
  unsigned ia, ib1, ib2, ja, jb;
  CTN_ZQP_P1_STEPS

  f32x16 acc2[8];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc2[i][e] = 0.f;

  // ---- prologue, once per workgroup: the first item's first two tiles (both phase 1: K1 >= 2 ZK)
#pragma unroll
  for (int i = 0; i < ZST - 1; ++i) {
    float* st = smem + i * ZSTG + ub * 2048;
    const char *ca = reinterpret_cast<const char*>(sa), *cb = reinterpret_cast<const char*>(sb);
    unsigned oa = ra, ob = rb;
#pragma unroll
    for (int j = 0; j < 4; ++j) { glds16(reinterpret_cast<const float*>(ca + oa), st + j * 256); oa += ia; }
#pragma unroll
    for (int j = 0; j < 4; ++j) { glds16(reinterpret_cast<const float*>(cb + ob), st + (4 + j) * 256); ob += j == 1 ? ib2 : ib1; }
    ra += (unsigned)ZK * ldE4;
    rb += (unsigned)ZK * ldXk4;
  }
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_waitcnt(0x0F70);          // vmcnt(0)
  __builtin_amdgcn_s_barrier();
#ifdef CTN_STAMPS
  if (a.dbg && tid == 0) a.dbg[(size_t)item * 8 + 1] = __builtin_amdgcn_s_memtime();
#endif

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
  const unsigned smem0 = lds_addr(smem);
  const unsigned fA = (unsigned)(h * 1024 + l31 * 4), fB = (unsigned)(4096 + h * 512 + ub * 128 + l31 * 4);
  const unsigned fY = (unsigned)(h * 4096 + l31 * 4);
  int st_cur = 0, st_nxt = 1, st_req = ZST - 1;

  // SEAM: what has to change before the statement's requests - nothing, or the re-base at a change of kind
#define CTN_ZQP_TILE(TEXT, SEAM)                                                                                       \
  {                                                                                                                    \
    SEAM                                                                                                               \
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
                   [sb] "s"(sb), [ia] "s"(ia), [ib1] "s"(ib1), [ib2] "s"(ib2), [ja] "s"(ja), [jb] "s"(jb),             \
                   [m0b] "s"(m0b)                                                                                      \
                 : "memory", "scc", CTN_ZQP_CLOBBERS);                                                                 \
    __builtin_amdgcn_sched_barrier(0);                                                                                 \
    st_req = st_cur;                                                                                                   \
    st_cur = st_nxt;                                                                                                   \
    st_nxt = st_nxt == ZST - 1 ? 0 : st_nxt + 1;                                                                       \
  }
#define CTN_ZQP_NONE
  // phase-1 tile S requests tile S + 2: the first Y tile of this pair of legs when that is past phase 1
#define CTN_ZQP_TO_Y(S)                                                                                                \
  {                                                                                                                    \
    const bool ys = (S) + 2 == T1;                                                                                     \
    const unsigned yv = (unsigned)(2 * p) * ldYq4 + laneY;                                                             \
    unsigned m4 = ldYm4;                                                                                               \
    asm volatile("" : "+s"(m4));                                                                                       \
    const unsigned p2_j = 29u * m4;                                                                                    \
    sa = ys ? Y : sa;                                                                                                  \
    sb = ys ? Y : sb;                                                                                                  \
    ia = ys ? ldYm4 : ia;                                                                                              \
    ib1 = ys ? ldYm4 : ib1;                                                                                            \
    ib2 = ys ? ldYm4 : ib2;                                                                                            \
    ja = ys ? p2_j : ja;                                                                                               \
    jb = ys ? p2_j : jb;                                                                                               \
    ra = ys ? yv : ra;                                                                                                 \
    rb = ys ? yv + 4u * ldYm4 : rb;                                                                                    \
  }
  // tile 6 of the first leg requests the second leg's first Y tile
#define CTN_ZQP_TO_LEG                                                                                                 \
  {                                                                                                                    \
    ra = (unsigned)(2 * p + 1) * ldYq4 + laneY;                                                                        \
    rb = ra + 4u * ldYm4;                                                                                              \
  }
  // tile 6 of the second leg requests the first E / X tile of the next pair of legs - the next item's after the last pair
#define CTN_ZQP_TO_P1                                                                                                  \
  {                                                                                                                    \
    const bool last = p + 1 == NP;                                                                                     \
    int xo = tn * ZU; /* (added here, through a copy the compiler cannot hoist: at the item's start the add would */  \
    asm volatile("" : "+s"(xo)); /* wait for the scalar load of Xn) */                                                 \
    sa = last ? En : E;                                                                                                \
    sb = last ? Xn + xo : X;                                                                                           \
    CTN_ZQP_P1_STEPS                                                                                                   \
    ra = laneE;                                                                                                        \
    rb = (last ? 0u : (unsigned)(2 * p + 2) * ldXq4) + laneX;                                                                        \
  }

  for (;;) {
    // ---- the item behind this one (scalar loads, first used at the last pair's seam): its own again for the last item
    const int nitem = item + G < items ? item + G : item;
    int r, t_, rn, tn;
    zipq_item_rt(item, per, &r, &t_);
    zipq_item_rt(nitem, per, &rn, &tn);
    const size_t tpn = (size_t)rn * a.n_tensors;
    const float* En = (const float*)zqp_ptr(a.ptrs, tpn + a.idE);
    const float* Xn = (const float*)zqp_ptr(a.ptrs, tpn + a.idX);           // (without its block of u: CTN_ZQP_TO_P1)
    const float* Yn = (const float*)zqp_ptr(a.ptrs, tpn + a.idY);
    float* Cn = (float*)zqp_ptr(a.ptrs, tpn + a.idC);
    // what the epilogue needs of this item: its rows of E', its partial's slot, E's producer partials
    float* __restrict__ row = C + (int64_t)(t_ * ZU + 32 * ub + l31) * a.ldC + 4 * h;
    const int pci = r * a.partC_stride + t_;
    double pve = 0.0;
    if (a.partE) {
      const double* __restrict__ pr = a.partE + (size_t)r * a.strideE;
      pve = pr[min(lane, a.PE - 1)];
      if (a.PE > 64)
        for (int i = lane + 64; i < a.PE; i += 64) pve += pr[i];
    }

    for (int p = 0; p < NP; ++p) {
      CTN_ZQP_TILE(CTN_ZQP_P1_FIRST, CTN_ZQP_TO_Y(0))
      for (int s = 1; s + 1 < T1; ++s) CTN_ZQP_TILE(CTN_ZQP_P1_MID, CTN_ZQP_TO_Y(s))
      CTN_ZQP_TILE(CTN_ZQP_P1_LAST, CTN_ZQP_NONE)
      CTN_ZQP_TILE(CTN_ZQP_P2_0_0, CTN_ZQP_NONE) CTN_ZQP_TILE(CTN_ZQP_P2_0_1, CTN_ZQP_NONE) CTN_ZQP_TILE(CTN_ZQP_P2_0_2, CTN_ZQP_NONE)
      CTN_ZQP_TILE(CTN_ZQP_P2_0_3, CTN_ZQP_NONE) CTN_ZQP_TILE(CTN_ZQP_P2_0_4, CTN_ZQP_NONE)
      CTN_ZQP_TILE(CTN_ZQP_P2_0_5, CTN_ZQP_NONE) CTN_ZQP_TILE(CTN_ZQP_P2_0_6, CTN_ZQP_TO_LEG)
      CTN_ZQP_TILE(CTN_ZQP_P2_0_7, CTN_ZQP_NONE)
      CTN_ZQP_TILE(CTN_ZQP_P2_1_0, CTN_ZQP_NONE) CTN_ZQP_TILE(CTN_ZQP_P2_1_1, CTN_ZQP_NONE)
      CTN_ZQP_TILE(CTN_ZQP_P2_1_2, CTN_ZQP_NONE) CTN_ZQP_TILE(CTN_ZQP_P2_1_3, CTN_ZQP_NONE)
      CTN_ZQP_TILE(CTN_ZQP_P2_1_4, CTN_ZQP_NONE) CTN_ZQP_TILE(CTN_ZQP_P2_1_5, CTN_ZQP_NONE)
      CTN_ZQP_TILE(CTN_ZQP_P2_1_6, CTN_ZQP_TO_P1) CTN_ZQP_TILE(CTN_ZQP_P2_1_7, CTN_ZQP_NONE)
    }
    // the last MFMAs' results -> their first reader below (18 wait states; nothing pads behind an asm statement)
    asm volatile("s_nop 15\n\ts_nop 7" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
#ifdef CTN_STAMPS
    if (a.dbg && tid == 0) {
      const unsigned long long now = __builtin_amdgcn_s_memtime();
      a.dbg[(size_t)item * 8 + 2] = now;
      a.dbg[(size_t)item * 8 + 4] = now;
    }
#endif

    // ---- epilogue: k_zipq_f32's, between this item's last statement and the next item's first
    pve = lane < a.PE ? pve : 0.0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) pve += __shfl_xor(pve, o, 64);
    const float nE = (float)pve;
    const float scE = (a.partE && nE > mnf) ? nE / nef : 1.f;
    const float iE = 1.0f / scE;
    float asum[2] = {0.f, 0.f};
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
    if (tid == 0) {                              // (red[] lies outside the ring; a whole item's tile barriers before its reuse)
      double tot = 0.0;
#pragma unroll
      for (int i = 0; i < 8; ++i) tot += red[i];
      a.partC[pci] = tot;
    }
    // E' is stored: zero again for the next item (64 moves; a C = 0 form of the first phase-2 tile would have to be
    // chosen by a branch between two statements with 150 tied registers each, which the register allocator answers
    // with copies and spills)
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc2[i][e] = 0.f;
#ifdef CTN_STAMPS
    if (a.dbg && tid == 0) {
      const unsigned long long now = __builtin_amdgcn_s_memtime();
      a.dbg[(size_t)item * 8 + 3] = now;
      if (nitem != item) a.dbg[(size_t)nitem * 8 + 0] = a.dbg[(size_t)nitem * 8 + 1] = now;     // (no prologue behind the first item)
    }
#endif
    if (nitem == item) break;
    item = nitem; E = En; X = Xn + tn * ZU; Y = Yn; C = Cn;
  }
#undef CTN_ZQP_TILE
#undef CTN_ZQP_NONE
#undef CTN_ZQP_P1_STEPS
#undef CTN_ZQP_TO_Y
#undef CTN_ZQP_TO_LEG
#undef CTN_ZQP_TO_P1
  // the two tiles requested past the end have to land before the workgroup gives its LDS back
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

}  // namespace ctn
