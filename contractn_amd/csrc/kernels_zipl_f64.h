// kernels_zipl_f64.h - the latency form of the zipper site pair (kernels_zipl.h) in float64: both GEMM steps of a site as
// ONE launch when only a FEW float64 networks are in flight, on v_mfma_f64_16x16x4_f64, with a request schedule of its
// own.  Part of the gfx950 contraction engine (see engine.hip for the overview).
#pragma once
#include "kernels_zipl.h"

namespace ctn {

// ---------------------------------------------------------------------------
// K-zip-lat-f64.  The pair of kernels_zipl.h,
//
//     T[m1, (q, u)] = sum_k1  E[k1, m1] * X[q, k1, u]          E'[u, n2] = sum_(m1, q)  T[m1, q, u] * Y[q, m1, n2]
//
// with |m1| = |n2| = K1 = 256, in float64 - the dtype of `tn.contract()`'s examples - for ONE network (or a few) in
// flight, where the chain is otherwise two dependent k_mfma_lat<double> launches per site.  The cut is k_zip_lat's with
// MP = 32 only: a workgroup (8 waves) owns 16 values of u and 32 of m1, its partial E'[u-block, all n2] leaves as slab
// number `mp` of S = 8, and the NEXT pair's workgroups add the slabs up in slab order while they load their piece of E
// (k_zip_slab_sum_f64 behind the last pair of a run).  128 workgroups per network at |u| = 256.  (MP = 64 does not
// fit: the E piece alone would be 128 KiB of LDS.)
//
// Phase 1 keeps the fp32 form's shape: wave (q, kp) owns one q and one of the NKP = 8 / Q parts of k1 and forms both
// 16 x 16 blocks of T for its q (E from LDS, where the slab sums were left; X straight from global memory into operand
// registers, one double per lane and k-step: lane (u, h) takes X[q][4 s + h][u0 + u]).  The register <-> row
// correspondence is k_zip_f64's (kernels_zip_f64.h), not the fp32 one: D[i = m1][j = u] leaves lane (j = lane & 15,
// h = lane >> 4) with row i = h + 4 e in register e.  A block goes to LDS in register order, [part][block][u][h][e],
// 32 bytes per lane; a phase-2 k-step e then pairs lane group h with m1 = 16 hh + 4 e + h: its B operand is the double
// at [u][h][e] (the parts of k1 added in their order), and the matching A operand of lane (i, h) is
// Y[q'][16 hh + 4 e + h][n2(i)].  Phase 2 cuts the other way: wave w owns n2 in [32 w, 32 w + 32) of every block, nothing
// is added across waves.  With n2(i, t) = 32 w + 2 (4 (i & 3) + (i >> 2)) + t for the two tiles t, one 16-byte load of Y
// feeds both tiles and lane (u, h) ends with n2 = 32 w + 8 h + 2 e + t: eight consecutive doubles of row u, four
// 16-byte stores.
//
// The request schedule.  k_zip_lat asks for everything it reads up front; at 8 bytes an element that would be 256 (E: 8
// slabs x 64 KiB) + 64 (X) + 128 (Y) registers per lane.  Here k1 is cut into NEP = 4 parts of 64 whole rows (finer than
// the waves' own NKP parts where NKP = 2) and at most TWO parts of slabs are in flight (2 x 64 registers): part 0, then X
// (whole), then part 1 up front; when a part has been added up in slab order and written to LDS its registers take the
// part after the next, and after the last part they take the Y fragments - the first half of the blocks behind the last
// barrier of phase 1, the rest behind phase 1 (when X's registers are free as well).  The waves of a part start their
// MFMAs as soon as THEIR rows of E are in LDS; barriers wait for LDS traffic only (zl_lds_barrier).  Whether E arrives as
// slabs is a template parameter (FROM_SLABS = slabs_in is set): a pair whose E is a tensor holds no slab registers.
//
// Stabilisation, epilogue and slabs are the fp32 form's arithmetic in double: lazy rescale by E's producer partials
// (iE = 1.0 exactly when partE is null), sum |slab piece| as ONE partial per workgroup - (U / 16) * 8 per replica, the
// waves' sums added in wave order - so that every consumer derives the triangle bound (see kernels_zipl.h).  No atomics;
// every sum has a fixed order: bit-reproducible.  Plain vector stores only.
//
// Conditions (fused_forms.h, zip_lat_form): |m1| = |n2| = K1 = 256, |u| a multiple of 16, Q = 4 or 2, operands dense
// along their innermost index with EVEN leading dimensions (16-byte requests), X and Y network inputs, fp64.  LDS:
// 96 KiB (E piece, rows 48 doubles apart) + 40 KiB (T blocks) = 136 KiB, one workgroup per CU.
// ---------------------------------------------------------------------------
struct ZipLat64Args {
  void* const* ptrs;        // [R][n_tensors]
  int32_t n_tensors, idE, idX, idY;
  const double* slabs_in;   // nullptr: E is tensor idE (rows ldE apart); else [R][S][K1][ZM] slabs of the pair before
  double* slabs_out;        // [R][S][U][ZM]
  int64_t ldE;
  int64_t ldXq, ldXk;       // X[q][k1][u]
  int64_t ldYq, ldYm;       // Y[q][m1][n2]
  int32_t U, R;
  const double* partE;      // E's producer partials (nullptr: a network input, or eager mode)
  int32_t PE, strideE;
  double numelE, min_norm;
  double* partC;            // [R][partC_stride]: one partial per workgroup, (U / 16) * S per replica
  int32_t partC_stride;
};

typedef double zl_d4 __attribute__((ext_vector_type(4)));
typedef double zl_d2 __attribute__((ext_vector_type(2)));

template <int V> using zl_ic = std::integral_constant<int, V>;   // a compile-time index handed to a lambda

constexpr int ZLD_MP = 32;                     // the part of m1 a workgroup owns
constexpr int ZLD_S = ZM / ZLD_MP;             // slabs of a result

template <int Q, bool FROM_SLABS>
__global__ __launch_bounds__(512, 1) void k_zip_lat_f64(ZipLat64Args a) {
  static_assert(Q == 4 || Q == 2, "a wave owns one q and one part of k1");
  constexpr int MP = ZLD_MP, S = ZLD_S;
  constexpr int NBQ = MP / 16;                 // 16 x 16 blocks of T per q: every wave of that q forms both ...
  constexpr int NKP = 8 / Q;                   // ... over ITS part of k1
  constexpr int NBLK = NBQ * Q;                // blocks of T per workgroup: (hh, q), hh slowest
  constexpr int LDE = MP + 16;                 // LDS row of the E piece: rows h and h + 1 of a fragment read start 32 banks apart
  constexpr int LDT = 20;                      // LDS row of a T block [u][h][e]: 16 doubles, 16-byte aligned, padded
  constexpr int NEP = 4;                       // parts of k1 the E piece is requested in: 64 whole rows each
  constexpr int PPE = 2;                       // 16-byte pieces of a part per thread: 64 rows x 16 pieces / 512
  constexpr int KSP = ZM / 4 / NEP;            // k-steps of a part (16)
  constexpr int EPW = NEP / NKP;               // parts of E per wave part of k1
  constexpr int KSW = KSP * EPW;               // k-steps of one wave
  constexpr int NY0 = NBLK / 2;                // blocks whose Y fragments are requested behind the last barrier of phase 1
  static_assert(NEP % NKP == 0, "a wave's part of k1 is whole parts of E");
  __shared__ __attribute__((aligned(16))) double sE[ZM * LDE];
  __shared__ __attribute__((aligned(16))) double sT[NKP * NBLK * 16 * LDT];
  __shared__ double red[8];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int q = w % Q, kp = w / Q;
  const int i16 = lane & 15, h = lane >> 4;
  // every XCD a contiguous range of work items; items are ordered (m1 part, replica, u block), as in k_zip_lat (the
  // grid is a multiple of 8 here: S = 8)
  const int pid = zipq_pid(blockIdx.x, gridDim.x);
  const int nub = a.U / 16, per_mp = a.R * nub;
  const int mp = pid / per_mp;
  const int rem = pid - mp * per_mp;
  const int r = rem / nub;
  const int ub = rem - r * nub;
  const int u0 = 16 * ub;

  void* const* tp = a.ptrs + (size_t)r * a.n_tensors;
  constexpr bool from_slabs = FROM_SLABS;       // (a.slabs_in != nullptr; compile-time, so that no slab register exists without slabs)

  // ---- the E piece [k1 = 0..255][m1 part], 16 bytes at a time, every slab of it: piece f = tid + 512 p is row
  // tid / 16 + 32 p, doubles 2 (tid % 16), + 1; part ep is the pieces 2 ep, 2 ep + 1 = rows [64 ep, 64 ep + 64)
  const int erow = tid >> 4, ec2 = tid & 15;
  zl_d2 sv[2][PPE][from_slabs ? S : 1];        // two parts in flight
  // (the slabs' address is a kernel argument: these requests do not wait for the pointer table)
  auto erequest = [&](auto ep_, auto buf_) {
    constexpr int ep = decltype(ep_)::value, buf = decltype(buf_)::value;
    if constexpr (from_slabs) {
      const double* __restrict__ Es = a.slabs_in + (size_t)r * S * ZM * ZM + mp * MP + 2 * ec2;
#pragma unroll
      for (int pp = 0; pp < PPE; ++pp)
#pragma unroll
        for (int s = 0; s < S; ++s)
          sv[buf][pp][s] = *reinterpret_cast<const zl_d2*>(Es + (size_t)s * ZM * ZM + (int64_t)(erow + 32 * (PPE * ep + pp)) * ZM);
    } else {
      const double* __restrict__ Es = (const double*)tp[a.idE] + mp * MP + 2 * ec2;
#pragma unroll
      for (int pp = 0; pp < PPE; ++pp)
        sv[buf][pp][0] = *reinterpret_cast<const zl_d2*>(Es + (int64_t)(erow + 32 * (PPE * ep + pp)) * a.ldE);
    }
  };
  erequest(zl_ic<0>{}, zl_ic<0>{});
  // this wave's X fragments: lane (u = i16, h) holds X[q][k1 = 4 s + h][u0 + u] of its k-steps s
  const double* __restrict__ X = (const double*)tp[a.idX] + u0;
  const double* __restrict__ Y = (const double*)tp[a.idY] + (int64_t)(mp * MP) * a.ldYm + 32 * w + 2 * (4 * (i16 & 3) + (i16 >> 2));
  double xb[KSW];
  {
    const double* __restrict__ px = X + (int64_t)q * a.ldXq + (int64_t)(4 * kp * KSW + h) * a.ldXk + i16;
#pragma unroll
    for (int s = 0; s < KSW; ++s) xb[s] = px[(int64_t)(4 * s) * a.ldXk];
  }
  erequest(zl_ic<1>{}, zl_ic<1>{});
  // E's producer partials (the lazy rescale of the epilogue)
  double pve = 0.0;
  if (a.partE) {
    const double* __restrict__ pr = a.partE + (size_t)r * a.strideE;
    pve = pr[min(lane, a.PE - 1)];
    if (a.PE > 64)
      for (int i = lane + 64; i < a.PE; i += 64) pve += pr[i];
  }
  // the Y fragments of phase 2, where this wave owns the columns n2 in [32 w, 32 w + 32) of EVERY block (hh, q'): lane
  // (i, h) takes Y[q'][m1 = 16 hh + 4 e + h][n2(i, 0), n2(i, 1)] - row i of the two tiles - as one 16-byte load
  zl_d2 yv[NBLK][4];
  auto yrequest = [&](int blk) {
    const int hh = blk / Q, qq = blk % Q;
    const double* __restrict__ py = Y + (int64_t)qq * a.ldYq + (int64_t)(16 * hh + h) * a.ldYm;
#pragma unroll
    for (int e = 0; e < 4; ++e) yv[blk][e] = *reinterpret_cast<const zl_d2*>(py + (int64_t)(4 * e) * a.ldYm);
  };

  // ---- phase 1: T_block[m1 = 16 b + i][u] += sum over this wave's k1 of E[k1][m1] Xq[k1][u], both blocks of its q.  The
  // parts of E become available one after the other (slab sums -> LDS -> barrier); the waves whose part of k1 holds
  // them start at once, while the later rows are still on their way
  zl_d4 acc1[NBQ];
#pragma unroll
  for (int b = 0; b < NBQ; ++b) acc1[b] = zl_d4{0.0, 0.0, 0.0, 0.0};
  auto part_step = [&](auto ep_) {               // (a compile-time part: every register array is indexed by constants)
    constexpr int ep = decltype(ep_)::value, buf = ep & 1;
#pragma unroll
    for (int pp = 0; pp < PPE; ++pp) {
      zl_d2 ev = sv[buf][pp][0];
      if constexpr (from_slabs) {
#pragma unroll
        for (int s = 1; s < S; ++s) ev += sv[buf][pp][s];            // slab order: fixed
      }
      *reinterpret_cast<zl_d2*>(sE + (erow + 32 * (PPE * ep + pp)) * LDE + 2 * ec2) = ev;
    }
    __builtin_amdgcn_sched_barrier(0);           // (no request of the next part moves up into the sums: its registers are these)
    if constexpr (ep + 2 < NEP) erequest(zl_ic<ep + 2>{}, zl_ic<buf>{});   // the registers just added up take the part after the next
    zl_lds_barrier();
    if constexpr (ep == NEP - 1) {
      // both parts' registers are free: the first half of the Y fragments, in the shadow of the last part's MFMAs
#pragma unroll
      for (int blk = 0; blk < NY0; ++blk) yrequest(blk);
    }
    if (kp == ep / EPW) {                        // (wave-uniform)
      const double* cA = sE + (4 * KSP * ep + h) * LDE + i16;
#pragma unroll
      for (int s = 0; s < KSP; ++s)
#pragma unroll
        for (int b = 0; b < NBQ; ++b)
          acc1[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(cA[4 * s * LDE + 16 * b], xb[(ep % EPW) * KSP + s], acc1[b], 0, 0, 0);
    }
  };
  static_assert(NEP == 4, "the four parts, spelled out");
  part_step(zl_ic<0>{});
  part_step(zl_ic<1>{});
  part_step(zl_ic<2>{});
  part_step(zl_ic<3>{});
  // D[i = m1][j = u] leaves lane (u, h) with m1 = h + 4 e in register e: 32 bytes per lane into [kp][blk][u][h][e]
#pragma unroll
  for (int b = 0; b < NBQ; ++b) {
    const int blk = b * Q + q;
    double* pt = sT + ((kp * NBLK + blk) * 16 + i16) * LDT + 4 * h;
    *reinterpret_cast<zl_d2*>(pt) = zl_d2{acc1[b][0], acc1[b][1]};
    *reinterpret_cast<zl_d2*>(pt + 2) = zl_d2{acc1[b][2], acc1[b][3]};
  }
#pragma unroll
  for (int blk = NY0; blk < NBLK; ++blk) yrequest(blk);
  zl_lds_barrier();

  // ---- phase 2: E'^T[n2][u] = sum over the blocks of Y[q'][m1][n2] T[m1][q'][u] for this wave's 32 columns: the B operand
  // of k-step e is the double at [u][h][e] - m1 = 16 hh + 4 e + h, the parts of k1 added in their order - and Y was
  // requested to match
  zl_d4 acc2[2] = {zl_d4{0.0, 0.0, 0.0, 0.0}, zl_d4{0.0, 0.0, 0.0, 0.0}};
#pragma unroll
  for (int blk = 0; blk < NBLK; ++blk) {
    const double* pt = sT + (blk * 16 + i16) * LDT + 4 * h;
    zl_d2 t01 = *reinterpret_cast<const zl_d2*>(pt), t23 = *reinterpret_cast<const zl_d2*>(pt + 2);
#pragma unroll
    for (int k2 = 1; k2 < NKP; ++k2) {
      t01 += *reinterpret_cast<const zl_d2*>(pt + k2 * NBLK * 16 * LDT);
      t23 += *reinterpret_cast<const zl_d2*>(pt + k2 * NBLK * 16 * LDT + 2);
    }
    const double tv[4] = {t01[0], t01[1], t23[0], t23[1]};
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int t = 0; t < 2; ++t) acc2[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(yv[blk][e][t], tv[e], acc2[t], 0, 0, 0);
  }

  // ---- epilogue: lane (u, h') holds n2 = 32 w + 8 h' + 2 e' + t in acc2[t][e']; lazy rescale, 16-byte stores, abs-sum
  pve = lane < a.PE ? pve : 0.0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) pve += __shfl_xor(pve, o, 64);
  const double scE = (a.partE && pve > a.min_norm) ? pve / a.numelE : 1.0;   // = producer_scale<double>()
  const double iE = 1.0 / scE;
  double* __restrict__ out = a.slabs_out + ((size_t)(r * S + mp) * a.U + u0 + i16) * ZM + 32 * w + 8 * h;
  double asum = 0.0;
  {
    zl_d2 v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[e] = zl_d2{acc2[0][e], acc2[1][e]} * iE;
      *reinterpret_cast<zl_d2*>(out + 2 * e) = v[e];
    }
    asum = ((fabs(v[0][0]) + fabs(v[0][1])) + (fabs(v[1][0]) + fabs(v[1][1]))) +
           ((fabs(v[2][0]) + fabs(v[2][1])) + (fabs(v[3][0]) + fabs(v[3][1])));
  }
  double part = asum;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
  if (lane == 0) red[w] = part;
  zl_lds_barrier();                              // (not __syncthreads: that would wait for the stores above to be acknowledged)
  if (tid == 0) {
    double tot = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) tot += red[i];
    a.partC[(size_t)r * a.partC_stride + mp * nub + ub] = tot;
  }
}

// The slabs of the LAST pair of a run (or of every pair, in the eager rescale mode) added up into the step's ordinary
// result tensor C[u][n2] (rows ldC apart, ldC even), with its true abs-sum partials: `slots` workgroups per replica, each
// a range of rows; slab order, fixed; 16 bytes at a time.
__global__ __launch_bounds__(256) void k_zip_slab_sum_f64(const double* __restrict__ slabs, int S, int U, void* const* ptrs,
                                                          int n_tensors, int idC, int64_t ldC, double* __restrict__ partC,
                                                          int partC_stride) {
  __shared__ double red[4];
  const int r = blockIdx.y, j = blockIdx.x, slots = gridDim.x;
  const int rows = (U + slots - 1) / slots;
  const int u_lo = j * rows, u_hi = min(U, u_lo + rows);
  double* __restrict__ C = (double*)ptrs[(size_t)r * n_tensors + idC];
  const double* __restrict__ sl = slabs + (size_t)r * S * U * ZM;
  double asum = 0.0;
  for (int f = threadIdx.x; f < (u_hi - u_lo) * (ZM / 2); f += 256) {
    const int u = u_lo + f / (ZM / 2), c2 = f % (ZM / 2);
    zl_d2 v = *reinterpret_cast<const zl_d2*>(sl + (size_t)u * ZM + 2 * c2);
    for (int s = 1; s < S; ++s) v += *reinterpret_cast<const zl_d2*>(sl + ((size_t)s * U + u) * ZM + 2 * c2);
    *reinterpret_cast<zl_d2*>(C + (int64_t)u * ldC + 2 * c2) = v;
    asum += fabs(v[0]) + fabs(v[1]);
  }
  const double tot = block_sum(asum, red);
  if (threadIdx.x == 0) partC[(size_t)r * partC_stride + j] = tot;
}

}  // namespace ctn
