// kernels_chain.h - k_chain_lds: the chain walker of kernels_stream.h (k_chain) with the walk kept on chip.
//
// One workgroup per replica executes every step of a chain plan in order, as k_chain does, and forms the same numbers
// operation for operation (bit-identical results, step_rescales and register).  What differs is where a step finds its
// data.  chain_pack.h packs the plan into a program of compact records; the kernel keeps a ring of kClRing record slots
// in LDS and runs, next to the arithmetic of step s, one stage for each of three later steps:
//   R  the words of record s + 3 are copied from the program into slot (s + 3) % kClRing
//   P  the pointers of step s + 2's three tensors are read from the pointer table into its record
//   D  the images of step s + 1's staged network inputs are gathered behind its record
// Each stage reads only what an EARLIER iteration wrote and every iteration ends with a workgroup barrier, so every
// prefetched byte is ordered before its first read by a barrier the reader takes, and slot (s + 3) % kClRing - last
// read by step s - 1 - is refilled only behind the barrier that ended that step.  The three stages' loads are
// independent of each other: a step costs one round trip to memory where k_chain pays three dependent ones plus the
// store and reload of the intermediate.  Intermediates stay in an LDS arena (chain_pack.h places them); one that does
// not fit keeps its workspace slot and is stored, then loaded after the barrier, as in k_chain.
//
// A step with at most kClSmall outputs is computed by wave 0 alone while waves 1 - 3 run the stages; a larger step
// runs the stages on all threads first.  Waves meet only at workgroup barriers: no flags, no spinning, and no workgroup
// reads another's data.
//
// The abs-sum of a step is the value block_sum (kernel_args.h) gives k_chain: lane t holds the double sum of |acc[o]|
// over o = t, t + 256, ... ascending; an xor-shuffle tree over offsets 32 ... 1 combines the 64 lanes of a wave; waves
// 0 ... 3 are added in order to +0.0.  A small step has terms in wave 0 only, the other waves' +0.0 change nothing.
#pragma once
#include <hip/hip_runtime.h>

#include "chain_pack.h"

namespace ctn {

template <typename T>
struct ChainLds {
  double red[4];
  double ptot[2];                               // the abs-sums of the last two steps, on their way to `partials`
  T one[16 / sizeof(T)];
  T sc[kChainMaxSteps];                         // rescale factor of every step's result
  alignas(16) int32_t ring[kClRing][kClSlotWords];
  alignas(16) unsigned char arena[kClArenaBytes];
};
static_assert(sizeof(ChainLds<double>) <= 160 * 1024, "k_chain_lds: static LDS");

__device__ __forceinline__ int cl_off(const int32_t* rec, const ClTab& t, int i) {
  return t.pos < 0 ? t.base + i * t.stride : rec[t.pos + i];
}

// The MAC loop of one step and this lane's share of its abs-sum: k_chain's operations in k_chain's order.  PA / PB / PC are
// plain pointers, or LDS pointers when all three tensors live on chip (ds_read / ds_write instead of flat accesses).
template <typename T, typename PA, typename PB, typename PC>
__device__ __forceinline__ double cl_mac(const int32_t* rec, const ClRec* c, PA A, PB B, PC C, T sA, T sB, bool divA, bool divB,
                                         int tid, int total) {
  const int M = c->M, N = c->N, K = c->K;
  const bool kprog = c->okA.pos < 0 && c->okB.pos < 0;
  const int ka0 = c->okA.base, kas = c->okA.stride, kb0 = c->okB.base, kbs = c->okB.stride;
  double absv = 0;
  for (int o = tid; o < total; o += 256) {
    const int n = o % N;
    const int q = o / N;
    const int m = q % M;
    const int b = q / M;
    PA pa = A + cl_off(rec, c->obA, b) + cl_off(rec, c->omA, m);
    PB pb = B + cl_off(rec, c->obB, b) + cl_off(rec, c->onB, n);
    T acc = 0;
    if (kprog) {
      pa += ka0; pb += kb0;
      if (divA && divB)      for (int k = 0; k < K; ++k) acc = fma(pa[k * kas] / sA, pb[k * kbs] / sB, acc);
      else if (divA)         for (int k = 0; k < K; ++k) acc = fma(pa[k * kas] / sA, pb[k * kbs], acc);
      else if (divB)         for (int k = 0; k < K; ++k) acc = fma(pa[k * kas], pb[k * kbs] / sB, acc);
      else                   for (int k = 0; k < K; ++k) acc = fma(pa[k * kas], pb[k * kbs], acc);
    } else {
      for (int k = 0; k < K; ++k) {
        T a = pa[cl_off(rec, c->okA, k)], bb = pb[cl_off(rec, c->okB, k)];
        if (divA) a = a / sA;
        if (divB) bb = bb / sB;
        acc = fma(a, bb, acc);
      }
    }
    C[cl_off(rec, c->obC, b) + cl_off(rec, c->omC, m) + cl_off(rec, c->onC, n)] = acc;
    absv += (double)fabs(acc);
  }
  return absv;
}

template <typename T>
__global__ __launch_bounds__(256) void k_chain_lds(const int32_t* __restrict__ prog, int len0, int n_steps,
                                                   void* const* ptrs, int n_tensors, double* partials,
                                                   int R, double min_norm, int stabilize) {
  __shared__ ChainLds<T> L;
  const int tid = threadIdx.x;
  const int r = blockIdx.x;
  void* const* tp = ptrs + (size_t)r * n_tensors;
  if (tid == 0) L.one[0] = (T)1;
  for (int s = -kClD; s < n_steps; ++s) {
    const int32_t* rec = L.ring[s & (kClRing - 1)];
    const ClRec* c = reinterpret_cast<const ClRec*>(rec);
    const int total = s >= 0 ? c->Bt * c->M * c->N : kClSmall + 1;
    const bool small = total <= kClSmall;

    // ---- the stages of the steps ahead (waves 1 - 3 next to a small step, else everybody)
    if (!small || tid >= 64) {
      const int pt = small ? tid - 64 : tid, pn = small ? 192 : 256;
      const int sr = s + 3, sp = s + 2, sd = s + 1;
      // the abs-sum of the step before leaves for memory now: its store is in flight while this step computes, not in
      // front of the barrier that ended its own step
      if (s >= 1 && pt == 3) partials[(size_t)(s - 1) * R + r] = L.ptot[(s - 1) & 1];
      // Every stage reads LDS that earlier iterations wrote and writes LDS nobody reads before the barrier below; the
      // compiler cannot know that, so the loads of all three stages are issued here, into registers, BEFORE the first
      // LDS store - one round trip for the three together.  (A stage with more than one element per thread - a record
      // with long explicit tables, a large image - finishes in the loops behind.)
      const bool doR = sr < n_steps, doP = sp >= 0 && sp < n_steps && pt < 3, doD = sd >= 0 && sd < n_steps;
      int r_off = 0, r_len = 0, r_val = 0;
      if (doR) {                                                                 // R
        r_len = len0;
        if (sr > 0) {
          const ClRec* p = reinterpret_cast<const ClRec*>(L.ring[(sr - 1) & (kClRing - 1)]);
          r_off = p->next_off; r_len = p->next_len;
        }
        if (pt < r_len) r_val = prog[r_off + pt];
      }
      uint64_t p_val = 0;
      if (doP) {                                                                 // P
        const ClRec* p = reinterpret_cast<const ClRec*>(L.ring[sp & (kClRing - 1)]);
        p_val = (uint64_t)tp[pt == 0 ? p->idA : pt == 1 ? p->idB : p->idC];
      }
      int32_t* drec = L.ring[sd & (kClRing - 1)];
      const ClRec* dp = reinterpret_cast<const ClRec*>(drec);
      const T *srcA = nullptr, *srcB = nullptr;
      int nA = 0, nB = 0;
      T a_val = 0, b_val = 0;
      auto offA = [&](int i) { const int k = i % dp->K, q = i / dp->K;
                               return cl_off(drec, dp->sbA, q / dp->M) + cl_off(drec, dp->smA, q % dp->M) + cl_off(drec, dp->skA, k); };
      auto offB = [&](int i) { const int nn = i % dp->N, q = i / dp->N;
                               return cl_off(drec, dp->sbB, q / dp->K) + cl_off(drec, dp->snB, nn) + cl_off(drec, dp->skB, q % dp->K); };
      if (doD) {                                                                 // D
        nA = dp->imgA; nB = dp->imgB;
        srcA = (const T*)dp->ptr[0]; srcB = (const T*)dp->ptr[1];
        if (pt < nA) a_val = srcA[offA(pt)];
        if (pt < nB) b_val = srcB[offB(pt)];
      }
      // ---- the stores, and what is left of long stages
      if (doR) {
        int32_t* dst = L.ring[sr & (kClRing - 1)];
        if (pt < r_len) dst[pt] = r_val;
        for (int i = pt + pn; i < r_len; i += pn) dst[i] = prog[r_off + i];
      }
      if (doP) reinterpret_cast<ClRec*>(L.ring[sp & (kClRing - 1)])->ptr[pt] = p_val;
      if (doD) {
        if (nA > 0) {
          T* img = reinterpret_cast<T*>(drec + dp->locA);
          if (pt < nA) img[pt] = a_val;
          for (int i = pt + pn; i < nA; i += pn) img[i] = srcA[offA(i)];
        }
        if (nB > 0) {
          T* img = reinterpret_cast<T*>(drec + dp->locB);
          if (pt < nB) img[pt] = b_val;
          for (int i = pt + pn; i < nB; i += pn) img[i] = srcB[offB(i)];
        }
      }
    }

    // ---- step s
    if (s >= 0 && (!small || tid < 64)) {
      const T sA = c->prodA >= 0 ? L.sc[c->prodA] : (T)1;
      const T sB = c->prodB >= 0 ? L.sc[c->prodB] : (T)1;
      auto home = [&](int h, int loc, uint64_t p) -> T* {
        return h == CL_HOME_ARENA ? reinterpret_cast<T*>(L.arena + loc)
             : h == CL_HOME_IMAGE ? reinterpret_cast<T*>(L.ring[s & (kClRing - 1)] + loc)
             : h == CL_HOME_ONE   ? L.one
                                  : reinterpret_cast<T*>(p);
      };
      T* A = home(c->homeA, c->locA, c->ptr[0]);
      T* B = home(c->homeB, c->locB, c->ptr[1]);
      T* C = home(c->homeC, c->locC, c->ptr[2]);
      bool divA = c->prodA >= 0, divB = c->prodB >= 0;
      if (c->normA | c->normB) {   // (large steps only: all threads are here) each element divided once, in place
        if (c->normA) { for (int i = tid; i < c->numelA; i += 256) A[i] = A[i] / sA; divA = false; }
        if (c->normB) { for (int i = tid; i < c->numelB; i += 256) B[i] = B[i] / sB; divB = false; }
        __syncthreads();
      }
      typedef __attribute__((address_space(3))) T LdsT;
      double absv;
      if (c->homeA != CL_HOME_GLOBAL && c->homeB != CL_HOME_GLOBAL && c->homeC != CL_HOME_GLOBAL)
        absv = cl_mac<T>(rec, c, (LdsT*)A, (LdsT*)B, (LdsT*)C, sA, sB, divA, divB, tid, total);
      else
        absv = cl_mac<T>(rec, c, A, B, C, sA, sB, divA, divB, tid, total);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) absv += __shfl_xor(absv, o, 64);
      double tot = 0;
      if (small) {
        tot += absv;                       // (+ three waves of +0.0)
      } else {
        if ((tid & 63) == 0) L.red[tid >> 6] = absv;
        __syncthreads();
        if (tid == 0) for (int i = 0; i < 4; ++i) tot += L.red[i];
      }
      if (tid == 0) {
        L.ptot[s & 1] = tot;                 // -> partials[s * R + r] (chain plans: one slot per step and replica)
        const T norm = (T)tot;
        L.sc[s] = (stabilize && norm > (T)min_norm) ? norm / (T)c->numelC : (T)1;
      }
    }
    // ends step s: its result and scale, and this iteration's three stages, are visible behind it
    __syncthreads();
  }
  if (tid == 0) partials[(size_t)(n_steps - 1) * R + r] = L.ptot[(n_steps - 1) & 1];
}

}  // namespace ctn
