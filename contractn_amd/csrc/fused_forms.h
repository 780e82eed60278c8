// fused_forms.h - which fused launches an executor takes: the launches that run two or more plan steps as one kernel
// (zipper pairs in their throughput and latency forms, complex x complex pairs, sweeps, leaf groups) or replace a plain
// step's kernel on a match of the plan's tables (the resident-left-operand kernel, the transposed dot).
// Pure host code (no HIP, no kernel header): the descriptors the launchers read, the matchers with the measurements
// behind them, and fused_forms(), the ONE place that walks them in order and lays out the partial sums.  engine.hip calls
// it once, when an executor is created, and allocates what the record asks for; forms_check.cpp drives it on the CPU
// under a sanitizer (make forms_check).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "cplx_match.h"
#include "launch_form.h"
#include "plan.h"
#include "zipq_items.h"

namespace ctn {

// What the rules below know of the kernels (engine.hip asserts that these are the kernels' own values): the zipper-pair
// kernels' |m1| = |n2|, values of u per workgroup and phase-1 tile depth (ZM, ZU, ZK of kernels_zip.h; ZD*: kernels_zip_f64.h,
// Z6*: kernels_zip64.h, Z1* and Z4*: kernels_zipm.h, Z5*: kernels_zip512.h), the sweeps' inputs per workgroup and most sites
// (SWR, kSweepMaxSites of kernels_sweep.h), and the resident-operand kernel's M, K and column tile (AR_M, AR_K, AR_TN of
// kernels_mfma_ares.h)
constexpr int kFormZM = 256, kFormZU = 128, kFormZK = 16;
constexpr int kFormZDU = 64, kFormZDK = 8;
constexpr int kFormZLD_MP = 32;                 // the part of m1 a workgroup of k_zip_lat_f64 owns (ZLD_MP of kernels_zipl_f64.h)
constexpr int kFormZ6U = 64, kFormZ6K = 32;
constexpr int kFormZ1M = 128, kFormZ1U = 128, kFormZ1K = 16;
constexpr int kFormZ4M = 64, kFormZ4U = 64, kFormZ4K = 16;
constexpr int kFormZ5M = 512, kFormZ5U = 64, kFormZ5K = 8;
constexpr int kFormSWR = 16, kFormSweepMaxSites = 1024;
constexpr int kFormArM = 256, kFormArK = 256, kFormArTN = 128;
static_assert(kFormZ1K == kFormZK, "zip_match checks K1 against ZK; k_zip128_f32's tile depth must be the same");
static_assert(kFormZ4K == kFormZK, "zip_match checks K1 against ZK; k_zipm64_f32's tile depth must be the same");
static_assert(kFormZK % kFormZ5K == 0, "zip_match checks K1 against ZK; k_zip512_f32's tile depth must divide it");

// A zipper pair (kernels_zip.h): the fused launch of steps (s2 - 1, s2); the first step of such a pair is never launched
// (its result only exists in the fused kernel's registers)
struct ZipDesc { bool on = false; int64_t ldE = 0, ldXq = 0, ldXk = 0, ldYq = 0, ldYm = 0, ldC = 0; int Q = 0, U = 0, K1 = 0;
                 int zu = 128; bool f64 = false;      // zu: values of u per workgroup (128: k_zip_f32, 64: k_zip64_f32, k_zip_f64)
                 int zm = 256;                        // zm: |m1| = |n2| (256; 128: k_zip128_f32, zu = 128; 64: k_zipm64_f32, zu = 64; 512: k_zip512_f32, zu = 64)
                 bool zq = false, zqp = false;        // zq: k_zipq_f32 runs the pair (zu = 128, zm = 256, Q even); zqp: as k_zipqp_f32
                 int form = CTN_FORM_NONE; };         // the kernel that runs the pair (ctn_step_form), set where it is chosen
// The same pair in its latency form (kernels_zipl.h; float64: kernels_zipl_f64.h, mp = 32 always): the fused launch of
// steps (s2 - 1, s2), whose result leaves as slabs; from_prev = its E is the slabs of the pair before, feeds_next = the next pair adds its slabs up (else
// k_zip_slab_sum does); buf: which of the two slab buffers it writes (ping-pong along the chain)
struct ZipLat { bool on = false, from_prev = false, feeds_next = false; int buf = 0, mp = 32; ZipDesc d; };
// A sweep (kernels_sweep.h): a run of epilogue-summed GEMM steps, each on the result of the one before, walked by ONE
// launch at the position of its last member
struct SweepDesc {
  bool on = false;
  std::vector<int> steps;          // the members' step indices, in chain order
  int64_t ldIn = 0, ldOut = 0, ldWl = 0, ldWp = 0, ldX = 0;
  int J = 0, M = 0, D = 0, Pd = 0;     // row blocks, rows, bond and physical dimension
  // every form: ids = [S][2] tensor ids (W_s, x_s), idIn the chain's input E, idOut the last site's E'
  int idIn = -1, idOut = -1;
  std::vector<int32_t> ids;
  // float64 (kernels_sweep_f64.h): the members are the 2 S steps of S sites - (GEMM, streaming sum over p) pairs, both
  // reporting a rescale factor (`two`)
  bool f64 = false;
  // small bonds (kernels_sweep_small.h): `two` - the members are the 2 S steps of S two-step sites, as in float64; else
  // the S epilogue-summed steps (float32 only).  small && f64: k_sweep_small<double>, always `two`.
  // tr (small only): every core of the run is stored TRANSPOSED - the bond contracted with the state is its unit-stride
  // axis and the bond it keeps has the stride ldWl (k_sweep_small<.., TR = true>); else the kept bond is unit-stride and
  // ldWl is the contracted one's.  ldWl is the stride of the core's non-unit bond either way.
  bool small = false, two = false, tr = false;
  int entries() const { return two ? 2 : 1; }                     // member steps - and abs-sum records - per site
  int sites() const { return (int)steps.size() / entries(); }
};
// A full dot of a tensor with a transposed one (k_dot_tr), found on the plan's tables
struct DotTr { bool on = false; int Ka = 0, Kb = 0, x_is_a = 1; int64_t ldY = 0; };
// Grouped leaf steps: runs of consecutive streaming steps whose operands are all network inputs (independent of
// each other and of everything before them) go out as ONE launch of k_stream_group; their arguments never
// change, so they are built on the first enqueue and kept in device memory (`ready`: that has happened - the one field
// of the record that the launcher writes).
struct LeafGroup { int len = 0, vw = 1, u = 1, blocks = 1, off = 0; bool ready = false; };

// Is k_zip_f64 taken without CTN_ZIP=1 when its launch fills the chip?  Decided by measurement.
static constexpr bool kZipF64Default = false;
// Is k_zip128_f32 taken without CTN_ZIP=1 when its launch fills the chip?  Decided by measurement.
static constexpr bool kZip128Default = false;
// Is k_zipm64_f32 taken without CTN_ZIP=1 when its launch fills the chip?  Decided by measurement.
static constexpr bool kZipM64Default = false;
// Is k_zip512_f32 taken without CTN_ZIP=1 when its launch fills the chip?  Decided by measurement (DESIGN sections 10 and 11).
static constexpr bool kZip512Default = false;

// Do steps (s2 - 1, s2) form a zipper pair that k_zip_f32 (`dtype` CTN_F32; `zm` = 128: k_zip128_f32, 64: k_zipm64_f32, 512: k_zip512_f32) or k_zip_f64 (CTN_F64)
// can run as one launch?
// Checked on the plan's own offset tables (every operand dense along its innermost index with uniform strides), so
// nothing about the network's labels is assumed: T = E . X with |m1| = zm rows from E, columns (q, u) from X;
// E' = T . Y contracting (m1, q), |n2| = zm.  The element type decides the kernel kind of the two steps, the depth of a
// phase-1 tile and - fp64: 16-byte requests and stores of pairs of doubles - that every leading dimension is even.
inline bool zip_match(const Plan& P, int s2, ZipDesc* z, int dtype, int u_mult = kFormZU, int zm = kFormZM) {
  if (s2 < 1 || s2 + 1 >= P.n_steps || P.dtype != dtype || (dtype != CTN_F32 && dtype != CTN_F64)) return false;
  const bool f64 = dtype == CTN_F64;
  const int kt = f64 ? kFormZDK : kFormZK;
  const Step& a = P.steps[s2 - 1];
  const Step& b = P.steps[s2];
  auto plain = [&](const Step& st) {
    return st.kernel == (f64 ? CTN_KERNEL_MFMA_F64 : CTN_KERNEL_MFMA_F32) && st.Bt == 1 && st.rhs >= 0 && st.lhs2 < 0 && !st.epw && st.modeA == 1 &&
           st.modeB == 1 && !st.collapse;
  };
  if (!plain(a) || !plain(b) || b.lhs != a.out || !b.cvec) return false;
  if (a.rhs >= P.n_inputs || b.rhs >= P.n_inputs) return false;            // X and Y: network inputs (scale 1)
  if (a.M != zm || b.N != zm || a.K % kt != 0 || a.K < 2 * kt || a.N % u_mult != 0) return false;
  const int32_t* T = P.tables.data();
  const int32_t *omA = T + a.t.omA, *okA = T + a.t.okA, *onB = T + a.t.onB, *okB = T + a.t.okB, *omC = T + a.t.omC, *onC = T + a.t.onC;
  const int64_t N1 = a.N;
  for (int i = 0; i < zm; ++i) if (omA[i] != i || omC[i] != (int64_t)i * N1) return false;     // E rows dense, T = [m1][N1]
  for (int64_t n = 0; n < N1; ++n) if (onC[n] != n) return false;
  int64_t U = N1;
  for (int64_t n = 1; n < N1; ++n) if (onB[n] != onB[0] + n) { U = n; break; }
  if (onB[0] != 0 || U % u_mult != 0 || N1 % U != 0) return false;
  const int64_t Q = N1 / U, ldXq = Q > 1 ? onB[U] : 0;
  for (int64_t n = 0; n < N1; ++n) if (onB[n] != (n / U) * ldXq + n % U) return false;
  const int64_t ldE = okA[1] - okA[0], ldXk = okB[1] - okB[0];
  for (int64_t k = 0; k < a.K; ++k) if (okA[k] != k * ldE || okB[k] != k * ldXk) return false;
  if (ldE < zm || b.M != U || b.K != (int64_t)zm * Q) return false;
  const int32_t *omA2 = T + b.t.omA, *okA2 = T + b.t.okA, *onB2 = T + b.t.onB, *okB2 = T + b.t.okB, *omC2 = T + b.t.omC, *onC2 = T + b.t.onC;
  for (int64_t u = 0; u < U; ++u) if (omA2[u] != u) return false;                                   // T dense along u
  for (int i = 0; i < zm; ++i) if (onB2[i] != i || onC2[i] != i) return false;
  const int64_t ldC = U > 1 ? omC2[1] - omC2[0] : zm;
  for (int64_t u = 0; u < U; ++u) if (omC2[u] != u * ldC) return false;
  if (ldC < zm) return false;
  // the contracted group of the second step enumerates (m1, q) in some order: read each entry's (m1, q) off T's offset
  int64_t ldYm = -1, ldYq = Q > 1 ? -1 : 0;
  for (int64_t k = 0; k < b.K; ++k) {
    const int64_t off = okA2[k], m1 = off / N1, q = (off % N1) / U;
    if (off % U != 0 || m1 >= zm) return false;
    if (m1 == 1 && q == 0) ldYm = okB2[k];
    if (m1 == 0 && q == 1) ldYq = okB2[k];
  }
  if (ldYm < zm || ldYq < 0) return false;
  std::vector<char> seen((size_t)b.K, 0);
  for (int64_t k = 0; k < b.K; ++k) {
    const int64_t off = okA2[k], m1 = off / N1, q = (off % N1) / U;
    if (okB2[k] != q * ldYq + m1 * ldYm || seen[(size_t)(m1 * Q + q)]) return false;
    seen[(size_t)(m1 * Q + q)] = 1;
  }
  if (f64 && ((ldE | ldXq | ldXk | ldYq | ldYm | ldC) & 1)) return false;
  z->on = true; z->f64 = f64; z->ldE = ldE; z->ldXq = ldXq; z->ldXk = ldXk; z->ldYq = ldYq; z->ldYm = ldYm; z->ldC = ldC;
  z->Q = (int)Q; z->U = (int)U; z->K1 = (int)a.K;
  return true;
}

// Is k_zipq_f32 taken without CTN_ZIPQ=1 where k_zip_f32 would be by its own default rule (fp32, one round of workgroups at
// least, rounds filled)?  Decided by measurement: +3.3 % on the headline at R = 512, +3.0 % at 128, +3.1 % at 256,
// fourteen times the larger spread.
static constexpr bool kZipQDefault = true;
// Can k_zipq_f32 run a pair that zip_match took for k_zip_f32?  Its legs go in pairs, and its LDS-DMA requests address
// every operand with an unsigned 32-bit byte offset off the tensor's base.
// Of the two forms of that kernel, is k_zipqp_f32 (a workgroup walks its work items; kernels_zipqp.h) taken without
// CTN_ZIPQ=2 where the rule above takes k_zipq_f32 and the launch has two rounds of workgroups at least (fewer: nothing
// to walk)?  Decided by measurement: +1.7 % on the headline at R = 512 (5,302.8 -> 5,391.9 contractions/s,
// spreads 7.9 and 5.0: eleven times the larger), +2.0 % at R = 256; the same bits.
static constexpr bool kZipQPDefault = true;
inline bool zipq_fits(const ZipDesc& z) {
  const int64_t lim = (int64_t)1 << 31;
  return z.Q >= 2 && z.Q % 2 == 0 && (int64_t)z.K1 * z.ldE * 4 < lim && ((int64_t)z.Q * z.ldXq + (int64_t)z.K1 * z.ldXk + z.U) * 4 < lim &&
         ((int64_t)z.Q * z.ldYq + (int64_t)kFormZM * z.ldYm) * 4 < lim;
}

// Is k_cmfma_f32 taken without CTN_CPLX=1 wherever cplx_match takes a pair?  Decided by measurement (DESIGN sections 10
// and 11): tools/cplx_step_timing.py has to show the fused form ahead of the two launches by more than the larger spread
// at every one of its shapes, and the complex GPU suite has to be green with CTN_CPLX=1.
static constexpr bool kCplxDefault = false;

// One site of a sweep, E'[b, r] = sum_p x[b, p] sum_l E[b, l] W[l, p, r], as either reader below finds it in the plan: the
// tensors, the row strides of E (ldA), E' (ldC) and x, the core's two non-unit strides, rows, bond and physical dimension,
// whether the core is stored transposed (SweepDesc::tr) and the site's member steps - sa alone, or the pair (sa, sb).
struct SweepSite { int idE = -1, idW = -1, idX = -1, idOut = -1; int64_t ldA = 0, ldC = 0, ldWl = 0, ldWp = 0, ldX = 0, M = 0;
                   int D = 0, Pd = 0; bool tr = false; int sa = -1, sb = -1; };

// The one-step reader: is step s an epilogue-summed GEMM step that k_sweep_f32 can take as one site of a sweep?  Checked on the plan's own
// offset tables: E row-major [b][l], W[l][p][r] with r unit-stride, x[b][p] with p unit-stride, result rows [b][r].
// `small`: as one site of k_sweep_small<float> instead - any bond 8 ... 64 that is a multiple of 4, x rows of any stride >= |p|.
inline bool sweep_site_one(const Plan& P, int s, SweepSite* sh, bool small) {
  const Step& st = P.steps[s];
  const int D = (int)st.K, Pd = st.epw;
  const bool bond_ok = small ? (st.K >= 8 && st.K <= 64 && st.K % 4 == 0) : (st.K == 64 || st.K == 128 || st.K == 256 || st.K == 512);
  if (P.dtype != CTN_F32 || st.kernel != CTN_KERNEL_MFMA_F32 || (Pd != 2 && Pd != 4) || st.Bt != 1 || !bond_ok ||
      st.N != (int64_t)D * Pd || s + 1 >= P.n_steps)
    return false;
  if (small && st.M >= ((int64_t)1 << 31) - kFormSWR) return false;
  // (st.collapse - the step's OWN launch would have more workgroups than partial slots and leave one collapsed slot - is
  // no obstacle: a member is never launched, and k_sweep_finish fills however many slots the step has, slot 0 first)
  if (st.rhs < 0 || st.rhs >= P.n_inputs || st.lhs2 < 0 || st.lhs2 >= P.n_inputs) return false;   // W, x: network inputs
  const int32_t* T = P.tables.data();
  const int32_t *omA = T + st.t.omA, *okA = T + st.t.okA, *onB = T + st.t.onB, *okB = T + st.t.okB, *omC = T + st.t.omC,
                *onC = T + st.t.onC, *omX = T + st.t.omA2;
  const int64_t M = st.M;
  const int64_t ldA = M > 1 ? omA[1] : D, ldC = M > 1 ? omC[1] : D, ldX = M > 1 ? omX[1] : Pd;
  // `small` alone: a TRANSPOSED core W[r][p][l] - l, the bond contracted with E, unit-stride and r at the stride ldWl
  const bool tr = small && okB[1] == 1;
  int64_t ldWl = okB[1];
  for (int64_t m = 0; m < M; ++m)
    if (omA[m] != m * ldA || omC[m] != m * ldC || omX[m] != m * ldX) return false;
  for (int k = 0; k < D; ++k)
    if (okA[k] != k || okB[k] != (int64_t)k * okB[1]) return false;
  int64_t ldWp = INT64_MAX;
  std::vector<char> seen((size_t)D * Pd, 0);
  if (tr) {
    // column n of C is (pp, rr) with rr = onC[n] its place in a row of E': onB[n] = pp ldWp + rr ldWl, so the stride of r
    // is the offset of (0, 1) and that of p the smallest nonzero offset of a column with rr = 0
    ldWl = INT64_MAX;
    for (int n = 0; n < D * Pd; ++n) {
      if (onC[n] == 1) ldWl = std::min<int64_t>(ldWl, onB[n]);
      if (onC[n] == 0 && onB[n] > 0) ldWp = std::min<int64_t>(ldWp, onB[n]);
    }
    if (ldWl == INT64_MAX || ldWp == INT64_MAX || ldWl <= 0) return false;
    for (int n = 0; n < D * Pd; ++n) {
      const int64_t rr = onC[n], rest = rr >= 0 && rr < D ? onB[n] - rr * ldWl : -1, pp = rest / ldWp;
      if (rest < 0 || rest % ldWp || pp >= Pd || seen[(size_t)(pp * D + rr)]) return false;
      seen[(size_t)(pp * D + rr)] = 1;
    }
  } else {
    for (int n = 0; n < D * Pd; ++n)
      if (onB[n] >= D) ldWp = std::min<int64_t>(ldWp, onB[n]);
    if (ldWp == INT64_MAX) return false;
    for (int n = 0; n < D * Pd; ++n) {
      const int64_t off = onB[n], pp = off / ldWp, rr = off % ldWp;
      if (off < 0 || pp >= Pd || rr >= D || onC[n] != rr || seen[(size_t)(pp * D + rr)]) return false;
      seen[(size_t)(pp * D + rr)] = 1;
    }
  }
  if (ldA < D || ldC < D || ldA % 4 || ldC % 4 || (!small && ldX % Pd) || ldX < Pd || ldWl % 4 || ldWp % 4 || ldWl < D) return false;
  // a lane's offsets into a core: 32 bits.  (Transposed: the largest is row D - 1 of r, p = 3 and the lane's four values
  // of l, ((D - 1) ldWl + 3 ldWp + 12) 4 bytes - below the same bound, which is kept for both.)
  if (((D + 12) * ldWl + 3 * ldWp + D) * 4 >= ((int64_t)1 << 31)) return false;
  sh->tr = tr; sh->sa = sh->sb = s;
  sh->idE = st.lhs; sh->idW = st.rhs; sh->idX = st.lhs2; sh->idOut = st.out;
  sh->ldA = ldA; sh->ldC = ldC; sh->ldWl = ldWl; sh->ldWp = ldWp; sh->ldX = ldX; sh->M = M; sh->D = D; sh->Pd = Pd;
  return true;
}

// The two-step reader: the float64 plan keeps a site as TWO steps (plan.cpp fuses them for fp32 only): sa a GEMM of E[b, l] with a network
// input W carrying {l, p, r}, sb the streaming step that sums p against a network input x[b, p].  Can k_sweep_f64 take
// the pair as one site?  Matched on the tensors' labels, dims and strides: E and E' row-major [b][.], r unit-stride in W,
// p unit-stride in x, every stride even (16-byte accesses).  The layout the planner gave C does not matter: C is never
// written.
// `small`: the same pair in float32 at a small bond, as one site of k_sweep_small<float> (kernels_sweep_small.h) - the planner
// keeps a float32 site as two steps too while its epilogue-summed step would be small (plan.cpp: M >= 64, N >= 32, K >= 8,
// M N >= 65536): any bond 8 ... 64 that is a multiple of 4, every stride of E, E' and W a multiple of 4 (16-byte accesses
// of the state's rows), x rows of any stride >= |p|.
// `small` on a float64 plan: the float64 pair at a small bond, as one site of k_sweep_small<double>: the same bonds, x
// rows of any stride >= |p| (8-byte loads), and every stride of E, E' and W even.  (`small` takes the plan's own type,
// float32 or float64 and nothing else.)  Why, stride by stride - the kernel's own accesses are all 8-byte: ldC (E') because k_sweep64_finish<double> rewrites
// the result's rows as double2; ldA (E) because a member's E is the E' of the site before (cur.ldA == last.ldC) and the run's
// input may be the very region its result lands on, with the same row stride (the aliasing rule of sweep_run) - one parity for
// both; ldWl and ldWp so that each 128-byte run that the 16 lanes of a group read of a core starts 16-byte aligned, as
// k_sweep_f64's own condition has it (a bond-64 plan is refused by both kernels or by neither on its strides).
inline bool sweep_site_two(const Plan& P, int sa, int sb, SweepSite* sh, bool small) {
  if ((P.dtype != CTN_F64 && !(small && P.dtype == CTN_F32)) || sb + 1 >= P.n_steps) return false;   // a step must follow the last member
  const Step& a = P.steps[sa];
  const Step& b = P.steps[sb];
  // (small: whichever kernels the planner gave the two steps - at a few rows the GEMM is a streaming step itself; what the
  // steps compute is read off the labels below, and neither is launched)
  if (small ? (a.kernel == CTN_KERNEL_FUSED || b.kernel == CTN_KERNEL_FUSED) : (a.kernel != CTN_KERNEL_MFMA_F64 || b.kernel != CTN_KERNEL_ELEMENT))
    return false;
  if (a.rhs < 0 || b.rhs < 0 || a.lhs2 >= 0 || b.lhs2 >= 0 || a.epw || b.epw) return false;
  auto axis = [](const Tensor& t, int32_t lab) {
    int found = -1;
    for (size_t i = 0; i < t.labels.size(); ++i)
      if (t.labels[i] == lab) { if (found >= 0) return -1; found = (int)i; }   // (a repeated label: no)
    return found;
  };
  const int idW = P.tensors[a.lhs].labels.size() == 3 ? a.lhs : a.rhs, idE = idW == a.lhs ? a.rhs : a.lhs;
  if (b.lhs != a.out && b.rhs != a.out) return false;
  const int idX = b.lhs == a.out ? b.rhs : b.lhs;
  if (idW >= P.n_inputs || idX >= P.n_inputs || idE == idW) return false;    // W, x: network inputs
  const Tensor &tE = P.tensors[idE], &tW = P.tensors[idW], &tX = P.tensors[idX], &tC = P.tensors[a.out], &tO = P.tensors[b.out];
  if (tE.labels.size() != 2 || tW.labels.size() != 3 || tX.labels.size() != 2 || tC.labels.size() != 3 || tO.labels.size() != 2) return false;
  const int el = axis(tW, tE.labels[0]) >= 0 ? 0 : 1;                        // E = {b, l}: l is the label W carries
  const int32_t ll = tE.labels[el], lb = tE.labels[1 - el];
  if (ll == lb || axis(tW, ll) < 0 || axis(tW, lb) >= 0 || axis(tX, lb) < 0) return false;
  const int32_t lp = tX.labels[1 - axis(tX, lb)];
  if (lp == lb || lp == ll || axis(tW, lp) < 0) return false;
  const int32_t lr = tW.labels[3 - axis(tW, ll) - axis(tW, lp)];
  if (lr == ll || lr == lp || lr == lb) return false;
  if (axis(tC, lb) < 0 || axis(tC, lp) < 0 || axis(tC, lr) < 0 || axis(tO, lb) < 0 || axis(tO, lr) < 0) return false;
  const int64_t D = tE.dims[el], Pd = tW.dims[axis(tW, lp)], M = tE.dims[1 - el];
  const bool bond_ok = small ? (D >= 8 && D <= 64 && D % 4 == 0) : (D == 64 || D == 128 || D == 256 || D == 512);
  if (!bond_ok || (Pd != 2 && Pd != 4) || tW.dims[axis(tW, lr)] != D || M >= ((int64_t)1 << 31) - kFormSWR)
    return false;
  // `small`: exactly one of the core's two bonds is unit-stride - r, or (tr: a transposed core) l; ldWl is the other's stride
  const bool tr = small && tW.strides[axis(tW, ll)] == 1 && tW.strides[axis(tW, lr)] != 1;
  if (tE.strides[el] != 1 || tW.strides[axis(tW, tr ? ll : lr)] != 1 || tX.strides[axis(tX, lp)] != 1 || tO.strides[axis(tO, lr)] != 1) return false;
  const int64_t ldA = tE.strides[1 - el], ldC = tO.strides[axis(tO, lb)], ldX = tX.strides[axis(tX, lb)];
  const int64_t ldWl = tW.strides[axis(tW, tr ? lr : ll)], ldWp = tW.strides[axis(tW, lp)];
  if (ldA < D || ldC < D || ldX < Pd || ldWl <= 0 || ldWp <= 0) return false;
  if (small ? ((ldA | ldC | ldWl | ldWp) & (P.dtype == CTN_F64 ? 1 : 3)) != 0 : ((ldA | ldC | ldX | ldWl | ldWp) & 1) != 0) return false;
  // a lane's offsets into a core: 32 bits, in bytes.  (8-byte elements: the largest a lane of k_sweep_small<double> forms is
  // (3 ldWl + 3 ldWp + D) 8 < 2^28 x 8 = 2^31; the rows 16 G + 4 e go into the 64-bit base.  Transposed: row D - 1 of r,
  // p = 3 and the lane's place in a group, ((D - 1) ldWl + 3 ldWp + 12) 4 or ((D - 1) ldWl + 3 ldWp + 3) 8 bytes - both
  // below the same bound.)
  if ((D + 12) * ldWl + 3 * ldWp + D >= ((int64_t)1 << 28)) return false;
  sh->tr = tr; sh->sa = sa; sh->sb = sb;
  sh->idE = idE; sh->idW = idW; sh->idX = idX; sh->idOut = b.out;
  sh->ldA = ldA; sh->ldC = ldC; sh->ldWl = ldWl; sh->ldWp = ldWp; sh->ldX = ldX; sh->M = M; sh->D = (int)D; sh->Pd = (int)Pd;
  return true;
}

// The longest run of sites, each taking the result of the one before as its E - `two`: of (GEMM, streaming) pairs, as
// sweep_site_two reads them, else of epilogue-summed steps (sweep_site_one); `small`: see the readers - and the ONE place
// that fills a SweepDesc.  Steps that launch nothing (CTN_KERNEL_FUSED, the markers of absorbed steps) are stepped over.
inline bool sweep_run(const Plan& P, SweepDesc* d, bool two, bool small) {
  auto next_launched = [&](int s) { do ++s; while (s < P.n_steps && P.steps[s].kernel == CTN_KERNEL_FUSED); return s; };
  auto site_at = [&](int sa, SweepSite* sh) {
    if (sa >= P.n_steps || P.steps[sa].kernel == CTN_KERNEL_FUSED) return false;
    if (!two) return sweep_site_one(P, sa, sh, small);
    const int sb = next_launched(sa);
    return sb < P.n_steps && sweep_site_two(P, sa, sb, sh, small);
  };
  std::vector<SweepSite> best;
  std::vector<char> used((size_t)P.n_steps, 0);
  for (int s0 = 0; s0 < P.n_steps; ++s0) {
    SweepSite first, cur;
    if (used[s0] || !site_at(s0, &first)) continue;
    std::vector<SweepSite> run{first};
    // Only markers of absorbed steps (nothing is launched for them) may lie between two members: the ONE launch of
    // the run sits at its last member's position and reads the first member's input there, which the plan's arena
    // released right after the first member - any launched step in between (the other half of an interleaved
    // left / right chain, say) could have been given that region.  So the next LAUNCHED step is a member - it takes the
    // run's last result as its E and has the same shape - or ends the run.
    while (site_at(next_launched(run.back().sb), &cur) && cur.idE == run.back().idOut && cur.M == first.M && cur.D == first.D &&
           cur.Pd == first.Pd && cur.ldWl == first.ldWl && cur.ldWp == first.ldWp && cur.ldX == first.ldX && cur.ldA == run.back().ldC &&
           cur.tr == first.tr)                      // (a core stored the other way round ends the run)
      run.push_back(cur);
    for (const SweepSite& m : run) used[m.sa] = used[m.sb] = 1;
    if (run.size() > best.size()) best = run;
  }
  if (best.size() < 2) return false;
  const SweepSite &first = best.front(), &last = best.back();
  {
    // the run's result must not land on its own input: blocks of rows start and finish at different times (a launch of
    // more than one round of workgroups), so a block's result rows may only cover ITS OWN input rows - the same region
    // with the same row stride - or nothing of the input at all
    const bool in_ws = first.idE >= P.n_inputs, out_ws = last.idOut < P.n_inputs + P.n_steps - 1;
    if (in_ws && out_ws) {
      const int64_t es = P.elem_size();
      const int64_t a0 = P.tensors[first.idE].ws_offset, a1 = a0 + ((first.M - 1) * first.ldA + first.D) * es;
      const int64_t b0 = P.tensors[last.idOut].ws_offset, b1 = b0 + ((first.M - 1) * last.ldC + first.D) * es;
      const bool overlap = a0 < b1 && b0 < a1;
      if (overlap && !(a0 == b0 && first.ldA == last.ldC)) return false;
    }
  }
  SweepDesc r;
  r.on = true; r.f64 = P.dtype == CTN_F64; r.small = small; r.two = two; r.tr = first.tr; r.idIn = first.idE; r.idOut = last.idOut;
  for (const SweepSite& m : best) {
    r.steps.push_back(m.sa);
    if (two) r.steps.push_back(m.sb);
    r.ids.push_back(m.idW); r.ids.push_back(m.idX);
  }
  r.ldIn = first.ldA; r.ldOut = last.ldC; r.ldWl = first.ldWl; r.ldWp = first.ldWp; r.ldX = first.ldX;
  r.J = (int)((first.M + kFormSWR - 1) / kFormSWR); r.M = (int)first.M; r.D = first.D; r.Pd = first.Pd;
  *d = r;
  return true;
}

// Is k_sweep_small<float> taken without CTN_SWEEP_SMALL=1 wherever sweep_small_match takes a run?  Decided by measurement
// (DESIGN sections 10 and 11): tools/sweep_small_timing.py has to show the one launch ahead of the per-site launches by
// more than the larger spread at every one of its shapes, and the small-bond GPU suite has to be green with CTN_SWEEP_SMALL=1.
static constexpr bool kSweepSmallDefault = false;
// Is k_sweep_small<double> taken without CTN_SWEEP_SMALL64=1 wherever sweep_small_match takes a run?  Decided by measurement
// (DESIGN sections 10 and 11, item 3c): tools/sweep_small_timing.py --dtype f64 has to show the one launch ahead of the
// per-site launches by more than the larger spread at every one of its shapes, and the float64 small-bond GPU suite has to
// be green with CTN_SWEEP_SMALL64=1.
static constexpr bool kSweepSmallF64Default = false;

// A batched MPS of bond 8 ... 64 (kernels_sweep_small.h).  Float32, in either shape the planner gives its sites: the longest
// run of two-step sites or of epilogue-summed steps, whichever walks more sites.  Float64: the longest run of two-step
// sites - the one shape a float64 plan has.  At most kFormSweepMaxSites sites.
// `tr_ok` false (CTN_SWEEP_SMALL_TR=0): a run of transposed cores is not taken.
inline bool sweep_small_match(const Plan& P, SweepDesc* d, bool tr_ok = true) {
  if (P.dtype != CTN_F32 && P.dtype != CTN_F64) return false;
  SweepDesc two, one;
  const bool m2 = sweep_run(P, &two, true, true) && (tr_ok || !two.tr), m1 = P.dtype == CTN_F32 && sweep_run(P, &one, false, true) && (tr_ok || !one.tr);
  if (!m1 && !m2) return false;
  *d = (m2 && (!m1 || two.sites() >= one.sites())) ? two : one;
  return d->sites() <= kFormSweepMaxSites;
}

// Is the small-bond sweep asked for on this plan?  Only on request while its type's default is off - float32:
// CTN_SWEEP_SMALL=1, kSweepSmallDefault; float64: CTN_SWEEP_SMALL64=1, kSweepSmallF64Default, and not against CTN_SWEEP64=0;
// neither switch reaches the other type - and never against CTN_SWEEP=0.
inline bool sweep_small_asked(const Plan& P, const DevSwitches& sw) {
  if (sw.sweep == 0 || !P.stabilize) return false;
  if (P.dtype == CTN_F32) return sw.sweep_small == 1 || (kSweepSmallDefault && sw.sweep_small != 0);
  return P.dtype == CTN_F64 && sw.sweep64 != 0 && (sw.sweep_small64 == 1 || (kSweepSmallF64Default && sw.sweep_small64 != 0));
}

// Is k_sweep_f64 taken without CTN_SWEEP=1?  Decided by measurement.
static constexpr bool kSweepF64Default = false;

// Which sweep takes the plan, if any: the ONE place that states the forms' precedence.  Never against CTN_SWEEP=0, and only
// while the plan rescales.  First k_sweep_f32, at least half a chip of row blocks, or CTN_SWEEP=1; then k_sweep_f64
// (CTN_SWEEP=1 and not CTN_SWEEP64=0; bond 64 ... 512, MFMA-sized steps: its run is never the small form's); then, only where
// neither took the plan and only on request (sweep_small_asked), the small-bond form of the plan's type.
inline bool sweep_form(const Plan& P, int R, int n_cu, const DevSwitches& sw, SweepDesc* d) {
  if (sw.sweep == 0 || !P.stabilize) return false;
  // (bonds up to 128: the per-site launches are a few microseconds of latency each whatever the batch - always)
  if (sweep_run(P, d, false, false) && d->sites() <= kFormSweepMaxSites &&
      (sw.sweep == 1 || (d->steps.size() >= 4 && (d->D <= 128 || (int64_t)d->J * R * 2 >= n_cu))))
    return true;
  if (P.dtype == CTN_F64 && sw.sweep64 != 0 && (sw.sweep == 1 || kSweepF64Default) && sweep_run(P, d, true, false) &&
      (int)d->steps.size() <= 2 * kFormSweepMaxSites)
    return true;
  if (sweep_small_asked(P, sw) && sweep_small_match(P, d, sw.sweep_small_tr != 0)) return true;
  *d = SweepDesc();
  return false;
}

// A chain plan (Plan::chain: every step small) is walked whole by the chain walker and has no fused form - most
// small-bond classifiers with a batch of a few dozen are such plans.  A small-bond sweep that is asked for and takes the
// plan (sweep_form: on a float64 plan only where k_sweep_f64 does not; no step of a chain plan is epilogue-summed, so
// k_sweep_f32 never does) takes it from the walker: the executor (and forms_check) then works on a copy whose steps are
// launches of their own again, with the slot counts and collapse flags the planner gave them before it marked the plan.
inline bool sweep_small_unchains(const Plan& P, int R, int n_cu, const DevSwitches& sw) {
  SweepDesc d;
  return P.chain && sweep_form(P, R, n_cu, sw, &d) && d.small;
}
inline Plan unchained(const Plan& P) {
  Plan Q = P;
  Q.chain = false;
  for (Step& st : Q.steps) { st.partials = st.partials_step; st.collapse = st.collapse_step; }
  return Q;
}

// Is this split dot step the sum over k = (a, b) of X[a Kb + b] Y[b ldY + a] - one operand contiguous in k, the other
// one its transpose (k_dot_tr)?  Checked on the plan's k tables.
inline bool dot_tr_match(const Plan& P, const Step& st, DotTr* d) {
  if (st.kernel != CTN_KERNEL_DOT || st.K < 32768 || st.K >= (1LL << 31)) return false;
  const int32_t* T = P.tables.data();
  for (int x_is_a = 1; x_is_a >= 0; --x_is_a) {
    const int32_t* kx = T + (x_is_a ? st.t.okA : st.t.okB);
    const int32_t* ky = T + (x_is_a ? st.t.okB : st.t.okA);
    bool contig = true;
    for (int64_t k = 0; k < st.K && contig; ++k) contig = kx[k] == k;
    if (!contig || ky[0] != 0) continue;
    const int64_t ldY = ky[1];
    if (ldY < 32) continue;
    int64_t Kb = 0;
    for (int64_t k = 1; k < st.K; ++k) if (ky[k] == 1) { Kb = k; break; }
    if (Kb < 32 || st.K % Kb != 0) continue;
    const int64_t Ka = st.K / Kb;
    if (Ka % 32 != 0 || Kb % 32 != 0 || ldY < Ka) continue;
    bool ok = true;
    for (int64_t k = 0; k < st.K && ok; ++k) ok = ky[k] == (k % Kb) * ldY + k / Kb;
    if (!ok) continue;
    d->on = true; d->Ka = (int)Ka; d->Kb = (int)Kb; d->x_is_a = x_is_a; d->ldY = ldY;
    return true;
  }
  return false;
}

// Can step s run on k_mfma_f32_ares, and how many 128-column tiles should a workgroup walk?  Checked on the plan's own
// tables (0 = no): M = K = 256, N a multiple of 128, B vector-loadable along n or along k, every
// 128-column tile of C dense, more workgroup partials than slots (the step already goes through k_collapse), and
// enough tiles that workgroups of at least four fill the chip's last round.
inline int ares_match(const Plan& P, int s, int R, int n_cu, const DevSwitches& sw) {
  const Step& st = P.steps[s];
  if (sw.ares == 0 || P.dtype != CTN_F32 || st.kernel != CTN_KERNEL_MFMA_F32 || st.rhs < 0 || st.lhs2 >= 0 || st.epw ||
      st.M != kFormArM || st.K != kFormArK || st.N % kFormArTN != 0 || !st.collapse)
    return 0;
  if (st.modeB != 1 && st.modeB != 2) return 0;
  const int32_t* T = P.tables.data();
  const int32_t *onB = T + st.t.onB, *okB = T + st.t.okB, *onC = T + st.t.onC;
  for (int64_t n = 0; n < st.N; ++n)
    if (onC[n] != onC[n & ~(int64_t)(kFormArTN - 1)] + (n & (kFormArTN - 1))) return 0;
  if (st.modeB == 1) {
    for (int64_t n = 0; n < st.N; n += 4)
      if (onB[n + 1] != onB[n] + 1 || onB[n + 2] != onB[n] + 2 || onB[n + 3] != onB[n] + 3 || onB[n] % 4) return 0;
  } else {
    for (int k = 0; k < kFormArK; k += 4)
      if (okB[k + 1] != okB[k] + 1 || okB[k + 2] != okB[k] + 2 || okB[k + 3] != okB[k] + 3 || okB[k] % 4) return 0;
    for (int64_t n = 0; n < st.N; ++n) if (onB[n] % 4) return 0;
  }
  const int64_t tiles = st.N / kFormArTN;       // per batch entry: a workgroup's tiles are tiles of one matrix
  R *= (int)st.Bt;
  if (sw.ares != 1 && tiles * 2 * R < 2LL * n_cu) return 0;         // (the throughput regime of the large-tile kernel)
  if (sw.ares_ntw > 0) return tiles % sw.ares_ntw == 0 ? sw.ares_ntw : 0;
  // as many tiles per workgroup as still fill the last round of workgroups (a workgroup's load of A costs about a
  // quarter of a tile), at least 4
  for (int ntw : {64, 32, 16, 8, 4}) {
    if (tiles % ntw) continue;
    const int64_t wgs = tiles / ntw * R, rounds = (wgs + n_cu - 1) / n_cu;
    if (wgs * 100 >= rounds * n_cu * 94) return ntw;
  }
  return sw.ares == 1 && tiles % 4 == 0 ? 4 : 0;
}

// ... and can the resident operand be fetched with 16-byte loads along k?
inline bool ares_avec(const Plan& P, int s) {
  const Step& st = P.steps[s];
  if (st.modeA != 2) return false;
  const int32_t* T = P.tables.data();
  const int32_t *omA = T + st.t.omA, *okA = T + st.t.okA, *obA = T + st.t.obA;
  if (obA[0] % 4 || P.tensors[st.lhs].numel % 4) return false;
  for (int k = 0; k < kFormArK; ++k) if (okA[k] != okA[0] + k) return false;
  if (okA[0] % 4) return false;
  for (int m = 0; m < kFormArM; ++m) if (omA[m] % 4) return false;
  return true;
}

// ---------------------------------------------------------------------------
// fused_forms(): everything an executor decides about its fused launches when it is created
// ---------------------------------------------------------------------------

// What is launched at a step's position.  Exclusive: latency pairs exist only in an executor that took no throughput
// pair, and a complex pair never contains a member of a zipper pair.
enum class Role : uint8_t {
  Plain,      // the form step_form gives it (or nothing: CTN_KERNEL_FUSED) - unless ares_ntw / dot_tr / groups say otherwise
  Absorbed,   // nothing: it runs inside a later launch - the first step of a zipper pair in either form (its pair is the
              // next step), or the S step of a complex pair (CplxDesc::sp of its pair)
  Zip,        // the second step of a zipper pair, throughput form: FusedForms::zip[s]
  ZipLat,     // ... latency form: FusedForms::zl[s]
  Cplx        // the GEMM of a complex pair: FusedForms::cplx[s]
};

struct FusedForms {
  std::vector<Role> role;             // per step
  // per step, read under its role alone (each vector is empty where no step has the role)
  std::vector<ZipDesc> zip;
  std::vector<ZipLat> zl;
  std::vector<CplxDesc> cplx;         // (its t* fields are offsets inside cplx_tabs)
  // a sweep and its members: sweep_role[s] = 1 a member that is never launched, 2 the last member, which launches the
  // run.  It holds while the executor rescales lazily; in eager mode the members run by their `role`.
  SweepDesc sweep;
  std::vector<char> sweep_role;       // per step
  // per step, for plain steps: column tiles per workgroup of k_mfma_f32_ares (bit 16: the left operand takes 16-byte
  // loads), 0 = not taken; the transposed dot; len >= 2 at the head of a leaf group, else 0
  std::vector<int> ares_ntw;
  std::vector<DotTr> dot_tr;
  std::vector<LeafGroup> groups;
  // the partial sums: abs-sum partials per replica of every step (what step_form gives, or one per workgroup of the fused
  // launch); step s, replica r at (step_off[s] * R + r * step_partials[s]) doubles; the sum of the steps' slots.  A chain
  // plan has one slot per step whatever its count says.
  std::vector<int> step_partials;
  std::vector<int64_t> step_off;
  int64_t part_slots = 0;
  // buffer sizes, in elements unless they say bytes; 0 = no such buffer
  size_t slab_elems = 0;              // split-K partial tiles: S slabs shaped like the step's output, all replicas
  size_t fold_elems = 0;              // where more than 16 slabs are folded 16 to 1
  int64_t zl_slab_elems = 0;          // each of the two slab buffers of the latency pairs, all replicas
  int64_t scratch_need = 1;           // doubles per replica of the collapse scratch
  int group_args = 0;                 // StepArgs records of all leaf groups
  // the sweep's records: a, s, z, la = ls, e (see Exec::d_sweep_*)
  size_t sweep_a = 0, sweep_s = 0, sweep_z = 0, sweep_l = 0, sweep_e = 0;
  // k_zipqp_f32 only: results that the plan's workspace puts where the pair's own E lies (the planner frees E at the
  // pair's first step, and first fit hands its bytes to E') live in side buffers instead - zqp_side[id] = which one, or -1.
  // A workgroup of k_zipq_f32 stores its rows of E' when every workgroup of the replica has long read E; a workgroup
  // that goes on to the replica's next block of u has not.
  std::vector<int> zqp_side;          // per tensor
  int64_t zqp_side_bytes = 0;         // one replica's part of one side buffer
  int zqp_side_bufs = 0;
  // host vectors to upload
  std::vector<int32_t> cplx_tabs;     // the pair-granular tables of all complex pairs
  std::vector<int32_t> sweep_ids;     // [S][2] tensor ids (W_s, x_s)
  std::vector<int64_t> sweep_offs;    // step_off of the sweep's members
  std::vector<int32_t> sweep_slots;   // step_partials of the sweep's members
};

// The throughput form of the zipper pair (s - 1, s), if it has one for R networks in flight: at least one full round of
// workgroups (each is 134 MFLOP long), or CTN_ZIP=1
inline bool zip_pair_form(const Plan& P, int s, int R, int n_cu, const DevSwitches& sw, ZipDesc* out) {
  ZipDesc z;
  // 128 values of u per workgroup (k_zip_f32) when that fills the chip - or CTN_ZIP=1; else 64 (k_zip64_f32) when THAT
  // does: 64 ... 127 networks of |u| = 256 - or CTN_ZIP=2; fewer networks keep the two-launch / latency forms
  // ... and of the two the one whose workgroups fill their rounds better (one workgroup per CU and round: 96 networks
  // are 192 workgroups of 128 - refused - or 384 of 64 - a round and a half: 26.0 ms against 23.0 on the two-launch
  // forms - while 64 networks are exactly one round of 64: 13.5 ms against 15.9)
  auto fill = [&](int64_t wgs) { return (double)wgs / (double)(((wgs + n_cu - 1) / n_cu) * n_cu); };
  ZipDesc z128, z64;
  if (P.dtype == CTN_F64) {
    // fp64: one form, 64 values of u per workgroup (k_zip_f64), and only on request (CTN_ZIP=1).  kZipF64Default is
    // where the rule of the fp32 forms - at least one round of workgroups, rounds filled to 0.9 - would switch it on
    // unasked; the measurement that has to decide that is in DESIGN section 10.
    if (sw.zip == 2 || !zip_match(P, s, &z, CTN_F64, kFormZDU)) return false;
    const int64_t wgs = (int64_t)(z.U / kFormZDU) * R;
    if (sw.zip != 1 && !(kZipF64Default && wgs >= n_cu && fill(wgs) >= 0.9)) return false;
    if (z.U / kFormZDU > kMaxPartials) return false;
    z.zu = kFormZDU; z.form = CTN_FORM_ZIP_F64;
    *out = z;
    return true;
  }
  const bool m128 = sw.zip != 2 && zip_match(P, s, &z128, CTN_F32) && (sw.zip == 1 || (int64_t)(z128.U / kFormZU) * R >= n_cu);
  const bool m64 = sw.zip != 1 && zip_match(P, s, &z64, CTN_F32, kFormZ6U) && z64.K1 % kFormZ6K == 0 &&
                   (sw.zip == 2 || (int64_t)(z64.U / kFormZ6U) * R >= n_cu);
  const double f128 = m128 ? fill((int64_t)(z128.U / kFormZU) * R) : 0.0, f64 = m64 ? fill((int64_t)(z64.U / kFormZ6U) * R) : 0.0;
  bool ok = false;
  if (m128 && (sw.zip == 1 || f128 >= 0.9 || f128 >= f64)) { ok = true; z = z128; z.zu = kFormZU; z.form = CTN_FORM_ZIP; }
  else if (m64 && (sw.zip == 2 || f64 >= 0.9)) { ok = true; z = z64; z.zu = kFormZ6U; z.form = CTN_FORM_ZIP64; }
  else if (m128) { ok = true; z = z128; z.zu = kFormZU; z.form = CTN_FORM_ZIP; }
  // the 128-u form with two legs per pass (k_zipq_f32): on request wherever the pair matches (CTN_ZIPQ=1, also where
  // the rules above chose otherwise - but not against CTN_ZIP=2), else under k_zip_f32's own default rule
  // ... and its walking form (k_zipqp_f32): on request (CTN_ZIPQ=2) wherever CTN_ZIPQ=1 takes k_zipq_f32, else under
  // kZipQPDefault where that kernel is taken by default and has two rounds of workgroups at least
  if ((sw.zipq == 1 || sw.zipq == 2) && sw.zip != 2 && zip_match(P, s, &z128, CTN_F32) && zipq_fits(z128)) {
    ok = true; z = z128; z.zu = kFormZU; z.zq = true; z.zqp = sw.zipq == 2;
    z.form = z.zqp ? CTN_FORM_ZIPQP : CTN_FORM_ZIPQ;
  } else if (sw.zipq == -1 && kZipQDefault && sw.zip == -1 && ok && z.zu == kFormZU && f128 >= 0.9 && zipq_fits(z)) {
    z.zq = true;
    z.zqp = kZipQPDefault && zipq_items(R, z.U, kFormZU) >= 2 * (int64_t)n_cu;
    z.form = z.zqp ? CTN_FORM_ZIPQP : CTN_FORM_ZIPQ;
  }
  // bond 128 (k_zip128_f32: 128 values of u per workgroup, K1 a multiple of its tile depth and two tiles at least -
  // ZK = Z1K, as zip_match checks), when no bond-256 form matches: only on request (CTN_ZIP=1, and not CTN_ZIP128=0).
  // kZip128Default is where the rule of the other forms - at least one round of workgroups, rounds filled to 0.9 - would switch it on unasked;
  // the measurement that has to decide that is in DESIGN section 10.
  if (!m128 && !m64 && sw.zip128 != 0 && sw.zip != 0 && sw.zip != 2 && zip_match(P, s, &z, CTN_F32, kFormZ1U, kFormZ1M) &&
      z.K1 % kFormZ1K == 0 && z.K1 >= 2 * kFormZ1K && ((z.ldE | z.ldXq | z.ldXk | z.ldYq | z.ldYm | z.ldC) & 3) == 0 &&
      (sw.zip == 1 || (kZip128Default && (int64_t)(z.U / kFormZ1U) * R >= n_cu && fill((int64_t)(z.U / kFormZ1U) * R) >= 0.9))) {
    ok = true; z.zu = kFormZ1U; z.zm = kFormZ1M; z.form = CTN_FORM_ZIP128;
  }
  // bond 64 (k_zipm64_f32: 64 values of u per workgroup, the same tile depth), when neither a bond-256 nor the bond-128
  // form matches: only on request (CTN_ZIP=1, and not CTN_ZIPM64=0).  kZipM64Default as kZip128Default: the
  // measurement that has to decide it is in DESIGN section 10.
  if (!ok && sw.zipm64 != 0 && sw.zip != 0 && sw.zip != 2 && zip_match(P, s, &z, CTN_F32, kFormZ4U, kFormZ4M) &&
      z.K1 % kFormZ4K == 0 && z.K1 >= 2 * kFormZ4K && ((z.ldE | z.ldXq | z.ldXk | z.ldYq | z.ldYm | z.ldC) & 3) == 0 &&
      (sw.zip == 1 || (kZipM64Default && (int64_t)(z.U / kFormZ4U) * R >= n_cu && fill((int64_t)(z.U / kFormZ4U) * R) >= 0.9))) {
    ok = true; z.zu = kFormZ4U; z.zm = kFormZ4M; z.form = CTN_FORM_ZIPM64;
  }
  // bond 512 (k_zip512_f32: 64 values of u per workgroup; its tile depth divides ZK, so zip_match's K1 condition - a
  // multiple of 16 and >= 32 - covers it), when no other form matches: only on request (CTN_ZIP=1, and not
  // CTN_ZIP512=0).  kZip512Default as kZip128Default: the measurement that has to decide it is in DESIGN section 10.
  if (!ok && sw.zip512 != 0 && sw.zip != 0 && sw.zip != 2 && zip_match(P, s, &z, CTN_F32, kFormZ5U, kFormZ5M) &&
      ((z.ldE | z.ldXq | z.ldXk | z.ldYq | z.ldYm | z.ldC) & 3) == 0 &&
      (sw.zip == 1 || (kZip512Default && (int64_t)(z.U / kFormZ5U) * R >= n_cu && fill((int64_t)(z.U / kFormZ5U) * R) >= 0.9))) {
    ok = true; z.zu = kFormZ5U; z.zm = kFormZ5M; z.form = CTN_FORM_ZIP512;
  }
  if (!ok || z.U / z.zu > kMaxPartials) return false;    // (one abs-sum partial per workgroup: the consumers add at most that many)
  *out = z;
  return true;
}

// Is k_zip_lat_f64 taken without CTN_ZIPL64=1 on a float64 plan with a few networks in flight?  Decided by measurement
// (DESIGN sections 10 and 11).
static constexpr bool kZipLatF64Default = false;

// The latency form of the same pair (k_zip_lat; `dtype` CTN_F64: k_zip_lat_f64), if it has one
inline bool zip_lat_form(const Plan& P, int s, int R, int n_cu, const DevSwitches& sw, ZipLat* out, int dtype = CTN_F32) {
  ZipDesc z;
  if (dtype == CTN_F64) {
    // fp64: a workgroup owns 32 of m1, always (64 does not fit its LDS; CTN_ZIPL_MP has no fp64 meaning); every leading
    // dimension even: zip_match's own fp64 condition
    if (!zip_match(P, s, &z, CTN_F64, 16)) return false;
    if (z.K1 != kFormZM || (z.Q != 4 && z.Q != 2)) return false;
    if ((z.U / 16) * (kFormZM / kFormZLD_MP) > kMaxPartials) return false;
    out->on = true; out->d = z; out->mp = kFormZLD_MP;
    return true;
  }
  if (!zip_match(P, s, &z, CTN_F32, 16)) return false;
  if (z.K1 != kFormZM || (z.Q != 4 && z.Q != 2) || z.ldC % 4 || z.ldE % 4 || z.ldXk % 4 || z.ldXq % 4 || z.ldYm % 4 || z.ldYq % 4) return false;
  // the part of m1 a workgroup owns: 32 (8 slabs, 128 workgroups per network at |u| = 256) while that still fits ONE
  // round of workgroups, else 64 (4 slabs, half the workgroups, each with twice the work per byte it loads)
  int mp = 64;
  if (z.Q == 4 && (sw.zipl_mp == 32 || (sw.zipl_mp == 0 && (int64_t)R * (z.U / 16) * 8 <= n_cu))) mp = 32;
  if ((z.U / 16) * (kFormZM / mp) > kMaxPartials) return false;
  out->on = true; out->d = z; out->mp = mp;
  return true;
}

// Every form writes its steps' slot counts first; the offsets are laid out once, when all counts stand.
inline FusedForms fused_forms(const Plan& P, int R, int n_cu, const DevSwitches& sw) {
  FusedForms F;
  const int n = P.n_steps;
  F.role.assign(n, Role::Plain);
  F.sweep_role.assign(n, 0);
  F.ares_ntw.assign(n, 0);
  F.dot_tr.assign(n, DotTr());
  F.groups.assign(n, LeafGroup());
  F.zqp_side.assign((size_t)(P.n_inputs + n + 1), -1);
  F.step_partials.resize(n);
  F.step_off.resize(n);
  // plain steps, as step_form runs them (the launcher asks it too, and these answers do not depend on the caller's
  // buffers): the slabs of a K split over workgroups, the partial counts - the plan's value, one per tile in the latency
  // form, up to 64 for the reduce pass of a K split - and the collapse scratch
  F.scratch_need = std::max<int64_t>(P.max_collapse_blocks, 1);
  for (int s = 0; s < n; ++s) {
    const Step& st = P.steps[s];
    const StepForm f = step_form(P, s, R, n_cu, sw, st.cvec);
    const size_t out_elems = (size_t)P.tensors[st.out].numel * (size_t)R;
    if (f.S) F.slab_elems = std::max(F.slab_elems, (size_t)f.S * out_elems);
    if (f.S > 16) F.fold_elems = std::max(F.fold_elems, (size_t)((f.S + 15) / 16) * out_elems);
    F.step_partials[s] = P.chain ? std::max(st.partials, 1) : f.partials;
    if (!P.chain) F.scratch_need = std::max<int64_t>(F.scratch_need, f.collapse_blocks);
  }
  if (P.chain) {   // the chain walker: one slot per step, whatever the kernel kind - and no fused form
    for (int s = 0; s < n; ++s) F.step_off[s] = F.part_slots++;
    return F;
  }
  // zipper pairs in their throughput form.  One abs-sum partial per workgroup of the fused launch; the absorbed step
  // keeps its (never written, zero) slots
  bool any_zip = false;
  if (sw.zip != 0)
    for (int s = 1; s + 1 < n; ++s) {
      ZipDesc z;
      if (F.role[s - 1] != Role::Plain || !zip_pair_form(P, s, R, n_cu, sw, &z)) continue;
      if (F.zip.empty()) F.zip.assign(n, ZipDesc());
      F.zip[s] = z;
      F.role[s] = Role::Zip; F.role[s - 1] = Role::Absorbed;
      F.step_partials[s] = z.U / z.zu;
      any_zip = true;
    }
  // the same pairs in their latency form: a few networks in flight (or CTN_ZIPL=1), and no throughput-form pair taken;
  // float64 (k_zip_lat_f64): only on request (CTN_ZIPL64=1) while kZipLatF64Default is off
  const bool lat32 = P.dtype == CTN_F32 && sw.zipl != 0 && (sw.zipl == 1 || R <= sw.zipl_max_r);
  const bool lat64 = P.dtype == CTN_F64 && (sw.zipl64 == 1 || (kZipLatF64Default && sw.zipl64 != 0 && R <= sw.zipl_max_r));
  if (!any_zip && (lat32 || lat64)) {
    int64_t slab_elems = 0;
    for (int s = 1; s + 1 < n; ++s) {
      ZipLat L;
      if (F.role[s - 1] != Role::Plain || !zip_lat_form(P, s, R, n_cu, sw, &L, P.dtype)) continue;
      if (F.zl.empty()) F.zl.assign(n, ZipLat());
      F.zl[s] = L;
      F.role[s] = Role::ZipLat; F.role[s - 1] = Role::Absorbed;
      const int S = kFormZM / L.mp;
      slab_elems = std::max<int64_t>(slab_elems, (int64_t)S * L.d.U * kFormZM);
      F.step_partials[s] = (L.d.U / 16) * S;        // one abs-sum partial per workgroup (of its slab piece)
    }
    for (int s = 3; s + 1 < n; ++s) {   // links of the chain: the pair (s - 1, s) takes the result of the pair (s - 3, s - 2)
      if (F.role[s] != Role::ZipLat || F.role[s - 2] != Role::ZipLat || P.steps[s - 1].lhs != P.steps[s - 2].out) continue;
      if (F.zl[s - 2].d.U != kFormZM || F.zl[s - 2].mp != F.zl[s].mp || F.zl[s - 2].d.ldC != F.zl[s].d.ldE) continue;
      F.zl[s].from_prev = true;
      F.zl[s].buf = F.zl[s - 2].buf ^ 1;
      F.zl[s - 2].feeds_next = true;
    }
    F.zl_slab_elems = (int64_t)R * slab_elems;
  }
  // complex x complex step pairs (k_cmfma_f32): only on request (CTN_CPLX=1) while kCplxDefault is off
  if (P.dtype == CTN_F32 && (sw.cplx == 1 || (kCplxDefault && sw.cplx != 0)))
    for (int s = 1; s < n; ++s) {
      // (a zipper pair is two GEMM steps: its members never have an S step behind them - and an S step, a streaming
      // step, is never this GEMM)
      if (F.role[s] != Role::Plain) continue;
      CplxDesc cd;
      if (!cplx_match(P, s, &cd, &F.cplx_tabs)) continue;
      const int64_t tiles = (int64_t)((cd.Mx + CX_TX - 1) / CX_TX) * ((cd.Ny + CX_TY - 1) / CX_TY);
      if (F.cplx.empty()) F.cplx.assign(n, CplxDesc());
      F.cplx[s] = cd;
      F.role[s] = Role::Cplx; F.role[cd.sp] = Role::Absorbed;
      // one abs-sum partial per workgroup of the fused launch (beyond the slots: collapsed to one); the absorbed S step
      // keeps its (never written, zero) slots: its rescale reads 0.0
      F.step_partials[s] = tiles > kMaxPartials ? 1 : (int)tiles;
      F.scratch_need = std::max<int64_t>(F.scratch_need, tiles);
    }
  // every step gets a region of exactly its count of slots per replica
  for (int s = 0; s < n; ++s) { F.step_off[s] = F.part_slots; F.part_slots += F.step_partials[s]; }
  // full dots against a transposed tensor
  if (sw.dot_tr)
    for (int s = 0; s < n; ++s) dot_tr_match(P, P.steps[s], &F.dot_tr[s]);
  // steps with a resident left operand (k_mfma_f32_ares)
  if (sw.ares != 0 && P.dtype == CTN_F32)
    for (int s = 0; s < n; ++s) {
      F.ares_ntw[s] = ares_match(P, s, R, n_cu, sw);
      if (F.ares_ntw[s] && ares_avec(P, s)) F.ares_ntw[s] |= 1 << 16;
    }
  // a sweep, in whichever form takes the plan (sweep_form).  Its records, per replica: an abs-sum per (member entry of a
  // site, row block) and a factor per member step; k_sweep_f32 keeps a scale and two logs per (site, row block) beside them,
  // the other forms an exponent
  if (SweepDesc sd; sweep_form(P, R, n_cu, sw, &sd)) {
    const size_t nrec = (size_t)R * sd.sites() * sd.J;
    F.sweep_a = sd.entries() * nrec; F.sweep_z = (size_t)R * sd.steps.size();
    if (sd.f64 || sd.small) F.sweep_e = nrec;
    else F.sweep_s = F.sweep_l = nrec;
    F.sweep_ids = sd.ids;
    for (int s : sd.steps) {
      F.sweep_role[s] = s == sd.steps.back() ? 2 : 1;
      F.sweep_offs.push_back(F.step_off[s]); F.sweep_slots.push_back(F.step_partials[s]);
    }
    F.sweep = sd;
  }
  // leaf groups: runs of consecutive plain streaming steps on network inputs, same kernel variant (see LeafGroup)
  if (sw.group) {
    auto leaf = [&](int s, int* vw, int* u) {
      const Step& st = P.steps[s];
      if (st.kernel != CTN_KERNEL_ELEMENT || st.kvec || st.collapse || s + 1 >= n || st.rhs < 0 ||
          st.lhs >= P.n_inputs || st.rhs >= P.n_inputs || st.lhs2 >= 0 || stream_splits(st, R, n_cu) ||
          F.role[s] == Role::Absorbed ||    // (a streaming step is absorbed as the S step of a complex pair: never launched)
          F.sweep_role[s])                  // (... or is a member of a sweep: at a few rows the E . W_1 step of a small-bond
                                            // two-step site is a streaming step on two network inputs)
        return false;
      int64_t nq;
      *vw = st.vecw;
      stream_variant(st, R, *vw, u, &nq);
      return true;
    };
    for (int s = 0; s < n;) {
      int vw, u;
      if (!leaf(s, &vw, &u)) { ++s; continue; }
      int e = s + 1, blocks = P.steps[s].blocks, vw2, u2;
      while (e < n && e - s < 1024 && leaf(e, &vw2, &u2) && vw2 == vw && u2 == u) { blocks = std::max(blocks, P.steps[e].blocks); ++e; }
      if (e - s >= 2) {
        LeafGroup& G = F.groups[s];
        G.len = e - s; G.vw = vw; G.u = u; G.blocks = blocks; G.off = F.group_args;
        F.group_args += G.len;
      }
      s = e;
    }
  }
  // k_zipqp_f32: a result that would overwrite the pair's E moves to a side buffer.  A buffer is free again once the
  // step that consumes its tensor has been launched (every intermediate is consumed exactly once): a chain needs two.
  if (any_zip) {
    const int64_t es = P.elem_size();
    std::vector<int> busy_until;                        // per side buffer: the step that reads what it holds
    for (int s = 1; s + 1 < n; ++s) {
      if (F.role[s] != Role::Zip || !F.zip[s].zqp) continue;
      const int idE = P.steps[s - 1].lhs, idC = P.steps[s].out;
      if (idE < P.n_inputs) continue;
      const int64_t e0 = P.tensors[idE].ws_offset, e1 = e0 + P.tensors[idE].numel * es;
      const int64_t c0 = P.tensors[idC].ws_offset, c1 = c0 + P.tensors[idC].numel * es;
      const bool e_in_ws = F.zqp_side[idE] < 0;       // (an E that moved itself is out of the way)
      if (!e_in_ws || c0 >= e1 || e0 >= c1) continue;
      int consumer = n;
      for (int c = s + 1; c < n; ++c)
        if (P.steps[c].lhs == idC || P.steps[c].rhs == idC || P.steps[c].lhs2 == idC) { consumer = c; break; }
      int k = 0;
      while (k < (int)busy_until.size() && busy_until[k] >= s - 1) ++k;      // (E's own buffer is read by step s - 1)
      if (k == (int)busy_until.size()) busy_until.push_back(0);
      busy_until[k] = consumer;
      F.zqp_side[idC] = k;
      F.zqp_side_bytes = std::max<int64_t>(F.zqp_side_bytes, (c1 - c0 + 255) / 256 * 256);
    }
    F.zqp_side_bufs = (int)busy_until.size();
  }
  return F;
}

}  // namespace ctn
