// engine.hip - gfx950 kernels + executor + C ABI of the contraction engine.
//
// Replaces the stabilised pairwise loop of the reference
// (contractn/einsum.py:326-393) and stabilize() (einsum.py:89-107):
//
//   * every pairwise step C[b,m,n] = sum_k A[b,m,k] * B[b,k,n] runs as ONE kernel whose
//     loads/stores go through gather-offset tables (transpose/reshape fused into
//     the load; reference einsum.py:371-377 does tensordot + transpose copies);
//   * a label kept while shared (copy tensor / hyperedge, reference ctn.py:154-165)
//     is a batch index of that kernel - no identity tensor is ever materialised;
//   * stabilize() is fused: the epilogue divides by the producers' rescale
//     factors (applied lazily: (A/sA)(B/sB) == (A B)/sA/sB), stores the
//     un-normalised tile and emits one partial sum of |C| per workgroup.  The
//     consumer (or the finishing pass) reduces <= 64 partials with one wave in a
//     fixed order, so results are bit-reproducible run to run (no float atomics).
//
// What runs where is decided in host-only headers: launch_form.h (step_form(): the kernel of a plain step, asked at
// creation and on every launch) and fused_forms.h (fused_forms(): the fused launches, every step's role in them and the
// layout of the partial sums, decided once in ctn_exec_create, which then only allocates).  The launch_<form> functions
// below read those records and launch.
//
// Written for CDNA4 only: 64-lane waves, v_mfma_f32_32x32x2_f32, 160 KiB LDS/CU.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "plan.h"
#include "chain_pack.h"
#include "cplx_match.h"
#include "fused_forms.h"
#include "grad_tape.h"
#include "launch_form.h"

#include "kernel_args.h"
#include "kernels_mfma.h"
#include "kernels_mfma_g.h"
#include "kernels_mfma_g64.h"
#include "kernels_mfma_h.h"
#include "kernels_mfma_ares.h"
#include "kernels_zip.h"
#include "kernels_zipq.h"
#include "kernels_zipqp.h"
#include "kernels_zip64.h"
#include "kernels_zipm.h"
#include "kernels_zip512.h"
#include "kernels_zip_f64.h"
#include "kernels_zipl.h"
#include "kernels_zipl_f64.h"
#include "kernels_sweep.h"
#include "kernels_sweep_f64.h"
#include "kernels_sweep_small.h"
#include "kernels_mfma_lat.h"
#include "kernels_stream.h"
#include "kernels_chain.h"
#include "kernels_grad.h"
#include "kernels_cplx.h"
#include "kernels_cmfma.h"

namespace ctn {

// ---------------------------------------------------------------------------
// executor
// ---------------------------------------------------------------------------
thread_local std::string g_err;

static_assert(kFormGM == GM && kFormGK == GK && kFormDN == DN && kFormLatMaxK == kLatMaxK,
              "launch_form.h selects kernels by these values of theirs");
static_assert(kFormZM == ZM && kFormZU == ZU && kFormZK == ZK && kFormZDU == ZDU && kFormZDK == ZDK && kFormZLD_MP == ZLD_MP && kFormZ6U == Z6U && kFormZ6K == Z6K &&
                  kFormZ1M == Z1M && kFormZ1U == Z1U && kFormZ1K == Z1K && kFormZ4M == Z4M && kFormZ4U == Z4U && kFormZ4K == Z4K && kFormZ5M == Z5M && kFormZ5U == Z5U && kFormZ5K == Z5K &&
                  kFormSWR == SWR && kFormSweepMaxSites == kSweepMaxSites && kFormArM == AR_M && kFormArK == AR_K && kFormArTN == AR_TN,
              "fused_forms.h matches plans against these values of theirs");

#define HIPCHECK(expr)                                                                  \
  do {                                                                                   \
    hipError_t e_ = (expr);                                                              \
    if (e_ != hipSuccess) {                                                              \
      g_err = std::string(#expr) + ": " + hipGetErrorString(e_);                         \
      return CTN_HIP_ERROR;                                                              \
    }                                                                                    \
  } while (0)

// Entry points select the executor's device and give the caller's current device back on return (a caller
// that works on another GPU - torch.cuda.current_device() - must not find it changed behind its back).
struct DeviceGuard {
  int prev = -1;
  hipError_t err;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) { prev = -1; (void)hipGetLastError(); }
    err = prev == dev ? hipSuccess : hipSetDevice(dev);
    if (prev == dev) prev = -1;   // nothing to restore
  }
  ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

struct Exec {
  const Plan* plan = nullptr;
  Plan own_plan;                       // `plan` points here when a small-bond sweep took a chain plan (fused_forms.h, unchained)
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  int R = 1;
  int n_tensors = 0;
  int n_cu = 256;
  DevSwitches sw;        // environment switches as they were when the executor was created
  // the launch sequence as a hipGraph (CTN_GRAPH, see exec_launch_all): captured on the second enqueue,
  // replayed afterwards; tensors are reached through the device pointer table, so new operands need no update
  int use_graph = 1;
  bool graph_warm = false;          // one eager enqueue has run (code objects loaded, tiles recorded)
  bool graph_aligned = true;        // outs_aligned16 the graph was captured under
  hipGraphExec_t graph_exec = nullptr;
  // Every fused launch the executor takes, each step's role in them, the layout of the partial sums and the sizes of
  // the buffers below: decided by fused_forms() (fused_forms.h) when the executor is created, read ever after.
  FusedForms forms;
  char* d_zqp_side = nullptr;          // k_zipqp_f32: [forms.zqp_side_bufs][R] side buffers of forms.zqp_side_bytes
  void* d_zl_slab[2] = {nullptr, nullptr};    // latency pairs: [R][S][U][ZM] each in the plan's dtype, ping-pong along the chain
  int32_t* d_cplx_tabs = nullptr;      // complex pairs: forms.cplx_tabs
  // the sweep's tables and records
  int32_t* d_sweep_ids = nullptr;      // [S][2] tensor ids (W_s, x_s)
  int64_t* d_sweep_off = nullptr;      // [S] step_off of the members
  int32_t* d_sweep_slots = nullptr;    // [S] step_partials of the members
  double* d_sweep_a = nullptr;         // [R][S][J]
  float* d_sweep_s = nullptr;          // [R][S][J]
  double* d_sweep_z = nullptr;         // [R][S]
  double* d_sweep_la = nullptr;        // [R][S][J] logs of d_sweep_a / d_sweep_s
  double* d_sweep_ls = nullptr;
  int32_t* d_sweep_e = nullptr;        // float64: [R][S][J] exponents of the blocks' scales (d_sweep_a: [R][2 S][J], d_sweep_z: [R][2 S])
  std::vector<int32_t> launched_form;  // per step: ctn_step_form of the last enqueue (ctn_exec_step_form), else 0
  std::vector<int32_t> launched_tile;  // per step: (tile rows << 16 | tile columns) of the last enqueue's MFMA kernel, else 0
  std::vector<int32_t> graph_form, graph_tile;   // what the captured sequence reported (a replay runs no host code) ...
  bool report_is_graphs = false;       // ... and whether launched_form / launched_tile hold exactly that
  char* d_ws = nullptr;
  int32_t* d_tables = nullptr;
  int64_t* d_tables64 = nullptr;    // batch / outer-group offsets (Plan::tables64)
  void** d_ptrs = nullptr;
  std::vector<void*> h_ptrs;
  bool ptrs_valid = false;
  double* d_partials = nullptr;
  double* d_scratch = nullptr;
  void* d_slab = nullptr;           // split-K partial tiles (latency mode), sized at creation
  void* d_slab2 = nullptr;          // 1/16 of it: where more than 16 slabs are folded 16 to 1 (k_splitk_fold)
  int64_t* d_stepOff = nullptr;     // forms.step_off and forms.step_partials
  int32_t* d_stepSlots = nullptr;
  double* d_log = nullptr;
  double* d_resc = nullptr;
  double* d_logs = nullptr;
  ChainStep* d_chain = nullptr;
  int32_t* d_chain_prog = nullptr;  // k_chain_lds: the packed program (chain_pack.h); null = the plan is walked by k_chain
  int chain_len0 = 0;               // ... and the length of its first record
  unsigned long long* d_dbg = nullptr;  // CTN_DEBUG_STAMPS=<file>: stamps of the LAST MFMA launch
  size_t dbg_tiles = 0;
  char* h_pack = nullptr;       // pinned host bounce buffer for many-small-operand staging
  size_t h_pack_bytes = 0;
  bool outs_aligned16 = true;
  void* d_ones = nullptr;
  int32_t* d_stepP = nullptr;
  double* d_stepNumel = nullptr;
  char* d_stage_in = nullptr;
  char* d_stage_out = nullptr;
  // Rescale mode.  false = lazy (default): tile kernels multiply by 1 / (sA sB) in the epilogue, the
  // un-normalised tensor is what is stored.  true = eager: every intermediate is normalised in place right
  // after its step (k_renorm) and consumed with scale 1 - the reference's own order of operations.  An executor
  // switches to eager by itself, and repeats the contraction, when the scale registers of a finished run show
  // that a lazy product left the dtype's range (exec_scales_suspect); it then stays eager.
  bool eager_rescale = false;
  bool eager_forced = false;        // ctn_exec_set_rescale_mode(1): every run eager; otherwise lazy is tried first
  int eager_reruns = 0;
  int eager_streak = 0;             // consecutive runs that had to be repeated eagerly (see exec_new_run)
  std::vector<double> h_resc;       // host copy of the last run's per-step rescale factors [R][n_steps]
  // the leaf groups' arguments (forms.groups, forms.group_args records), built on the first enqueue
  StepArgs* h_group_args = nullptr; // pinned: the one-time upload may fall inside a stream capture
  StepArgs* d_group_args = nullptr;
  bool defer_finish = false;        // ctn_exec_set_finish_mode(1): the final division waits for ctn_exec_finish
  double* d_mult = nullptr;         // [R] factors of ctn_exec_finish
  char* d_merge = nullptr;          // ctn_exec_merge_scales: liveness flags + new registers, grown on demand
  size_t merge_bytes = 0;
  int timing_slots = 0;             // 0 = timing off
  int timing_runs = 0;              // enqueues recorded since timing was enabled
  std::vector<hipEvent_t> events;   // [slot][step][2]

  ~Exec() {
    DeviceGuard dg(device);
    for (void* p : {(void*)d_ws, (void*)d_tables, (void*)d_tables64, (void*)d_ptrs, (void*)d_partials, (void*)d_scratch, (void*)d_slab, (void*)d_slab2,
                    (void*)d_log, (void*)d_resc, (void*)d_logs, (void*)d_chain, d_ones, (void*)d_stepP, (void*)d_stepNumel,
                    (void*)d_stepOff, (void*)d_stepSlots,
                    (void*)d_stage_in, (void*)d_stage_out, (void*)d_group_args, (void*)d_sweep_ids, (void*)d_sweep_off,
                    (void*)d_sweep_slots, (void*)d_sweep_a, (void*)d_sweep_s, (void*)d_sweep_z, (void*)d_sweep_la, (void*)d_sweep_ls, (void*)d_sweep_e,
                    (void*)d_merge, (void*)d_zl_slab[0], (void*)d_zl_slab[1], (void*)d_mult, (void*)d_cplx_tabs, (void*)d_chain_prog, (void*)d_zqp_side})
      if (p) (void)hipFree(p);
    if (h_pack) (void)hipHostFree(h_pack);
    if (h_group_args) (void)hipHostFree(h_group_args);
    for (auto ev : events) (void)hipEventDestroy(ev);
    if (graph_exec) (void)hipGraphExecDestroy(graph_exec);
    if (own_stream && stream) (void)hipStreamDestroy(stream);
  }
};

template <int MA, int BK, int TN, int TM>
static void launch_mfma_b(int mb, dim3 grid, hipStream_t st, const StepArgs& a) {
  switch (mb) {
    case 1: hipLaunchKernelGGL((k_mfma_f32<MA, 1, BK, TN, TM>), grid, dim3(256), 0, st, a); break;
    case 2: hipLaunchKernelGGL((k_mfma_f32<MA, 2, BK, TN, TM>), grid, dim3(256), 0, st, a); break;
    default: hipLaunchKernelGGL((k_mfma_f32<MA, 0, BK, TN, TM>), grid, dim3(256), 0, st, a); break;
  }
}

template <int BK, int TN, int TM>
static void launch_mfma_a(int ma, int mb, dim3 grid, hipStream_t st, const StepArgs& a) {
  switch (ma) {
    case 1: launch_mfma_b<1, BK, TN, TM>(mb, grid, st, a); break;
    case 2: launch_mfma_b<2, BK, TN, TM>(mb, grid, st, a); break;
    case 3: launch_mfma_b<3, BK, TN, TM>(mb, grid, st, a); break;   // A = X (.) Y formed while staging (fused step)
    case 4: launch_mfma_b<4, BK, TN, TM>(mb, grid, st, a); break;   // ... with 16-byte accesses along the rows
    case 5: launch_mfma_b<5, BK, TN, TM>(mb, grid, st, a); break;   // ... along k
    default: launch_mfma_b<0, BK, TN, TM>(mb, grid, st, a); break;
  }
}

// epilogue-summed steps (planner pattern C): BK = 16, a plain A operand
template <int MA, int TN, int TM>
static void launch_mfma_epw_b(int mb, dim3 grid, hipStream_t st, const StepArgs& a) {
  switch (mb) {
    case 1: hipLaunchKernelGGL((k_mfma_f32<MA, 1, 16, TN, TM, true>), grid, dim3(256), 0, st, a); break;
    case 2: hipLaunchKernelGGL((k_mfma_f32<MA, 2, 16, TN, TM, true>), grid, dim3(256), 0, st, a); break;
    default: hipLaunchKernelGGL((k_mfma_f32<MA, 0, 16, TN, TM, true>), grid, dim3(256), 0, st, a); break;
  }
}
template <int TN, int TM>
static void launch_mfma_epw(int ma, int mb, dim3 grid, hipStream_t st, const StepArgs& a) {
  switch (ma) {
    case 1: launch_mfma_epw_b<1, TN, TM>(mb, grid, st, a); break;
    case 2: launch_mfma_epw_b<2, TN, TM>(mb, grid, st, a); break;
    default: launch_mfma_epw_b<0, TN, TM>(mb, grid, st, a); break;
  }
}

// tile_m = 64: skinny rows (M <= 64 against a huge N) - always BK = 16 (these steps have a short K)
static void launch_mfma(int ma, int mb, int tile_m, int tile_n, dim3 grid, hipStream_t st, const StepArgs& a, const DevSwitches& sw) {
  if (a.epw) {
    if (tile_m == 64) {
      if (tile_n == 64) launch_mfma_epw<64, 64>(ma, mb, grid, st, a);
      else launch_mfma_epw<128, 64>(ma, mb, grid, st, a);
    } else {
      if (tile_n == 64) launch_mfma_epw<64, 128>(ma, mb, grid, st, a);
      else launch_mfma_epw<128, 128>(ma, mb, grid, st, a);
    }
    return;
  }
  const bool bk16 = mfma_bk(a.K, sw) == 16;
  if (tile_m == 64) {
    if (tile_n == 64) launch_mfma_a<16, 64, 64>(ma, mb, grid, st, a);
    else launch_mfma_a<16, 128, 64>(ma, mb, grid, st, a);
  } else if (tile_n == 64) {
    if (bk16) launch_mfma_a<16, 64, 128>(ma, mb, grid, st, a);
    else launch_mfma_a<32, 64, 128>(ma, mb, grid, st, a);
  } else {
    if (bk16) launch_mfma_a<16, 128, 128>(ma, mb, grid, st, a);
    else launch_mfma_a<32, 128, 128>(ma, mb, grid, st, a);
  }
}

// the reduce pass of a split-K step: fold 16 to 1 while more than 16 slabs are left (ping-pong between the two
// slab buffers), then the final pass (rescale, C, abs-sum partials)
template <typename T>
static void launch_splitk_reduce(Exec* E, int partials, int R, const StepArgs& a, SplitKArgs sk);

template <typename T>
static void launch_stream_group(int vw, int u, dim3 g, hipStream_t st, const StepArgs* arr) {
  constexpr int VF = 16 / (int)sizeof(T);
  if (vw == VF) {
    if (u == 4) hipLaunchKernelGGL((k_stream_group<T, VF, 4>), g, dim3(256), 0, st, arr);
    else hipLaunchKernelGGL((k_stream_group<T, VF, 1>), g, dim3(256), 0, st, arr);
  } else {
    if (u == 4) hipLaunchKernelGGL((k_stream_group<T, 1, 4>), g, dim3(256), 0, st, arr);
    else hipLaunchKernelGGL((k_stream_group<T, 1, 1>), g, dim3(256), 0, st, arr);
  }
}

template <int MA>
static void launch_sk_b(int mb, dim3 grid, hipStream_t st, const StepArgs& a, const SplitKArgs& sk) {
  switch (mb) {
    case 1: hipLaunchKernelGGL((k_mfma_f32_sk<MA, 1>), grid, dim3(256), 0, st, a, sk); break;
    case 2: hipLaunchKernelGGL((k_mfma_f32_sk<MA, 2>), grid, dim3(256), 0, st, a, sk); break;
    default: hipLaunchKernelGGL((k_mfma_f32_sk<MA, 0>), grid, dim3(256), 0, st, a, sk); break;
  }
}

static void launch_sk(int ma, int mb, dim3 grid, hipStream_t st, const StepArgs& a, const SplitKArgs& sk) {
  switch (ma) {
    case 1: launch_sk_b<1>(mb, grid, st, a, sk); break;
    case 2: launch_sk_b<2>(mb, grid, st, a, sk); break;
    default: launch_sk_b<0>(mb, grid, st, a, sk); break;
  }
}

template <int MA>
static void launch_sk64_b(int mb, dim3 grid, hipStream_t st, const StepArgs& a, const SplitKArgs& sk) {
  switch (mb) {
    case 1: hipLaunchKernelGGL((k_mfma_f64_sk<MA, 1>), grid, dim3(256), 0, st, a, sk); break;
    case 2: hipLaunchKernelGGL((k_mfma_f64_sk<MA, 2>), grid, dim3(256), 0, st, a, sk); break;
    default: hipLaunchKernelGGL((k_mfma_f64_sk<MA, 0>), grid, dim3(256), 0, st, a, sk); break;
  }
}

static void launch_sk64(int ma, int mb, dim3 grid, hipStream_t st, const StepArgs& a, const SplitKArgs& sk) {
  switch (ma) {
    case 1: launch_sk64_b<1>(mb, grid, st, a, sk); break;
    case 2: launch_sk64_b<2>(mb, grid, st, a, sk); break;
    default: launch_sk64_b<0>(mb, grid, st, a, sk); break;
  }
}

template <typename T>
static void launch_splitk_reduce(Exec* E, int partials, int R, const StepArgs& a, SplitKArgs sk) {
  T* bufs[2] = {(T*)E->d_slab, (T*)E->d_slab2};
  int cur = 0;
  while (sk.S > 16 && E->d_slab2) {
    const int S_out = (sk.S + 15) / 16;
    constexpr int V = 16 / sizeof(T);
    const dim3 grid((unsigned)((sk.numelC + 256 * V - 1) / (256 * V)), (unsigned)S_out, (unsigned)R);
    hipLaunchKernelGGL(k_splitk_fold<T>, grid, dim3(256), 0, E->stream, (const T*)bufs[cur], bufs[cur ^ 1],
                       sk.numelC, sk.S, S_out);
    cur ^= 1;
    sk.S = S_out;
  }
  sk.slab = bufs[cur];
  hipLaunchKernelGGL(k_splitk_reduce<T>, dim3(partials, R), dim3(256), 0, E->stream, a, sk);
}

// Is a chain plan walked by k_chain_lds without CTN_CHAIN=2 wherever chain_pack accepts it?  Decided by measurement
// (DESIGN sections 10 and 11): tools/chain_timing.py has to show it ahead of k_chain by more than the larger spread at
// every workload it measures, and the whole suite has to be green with it on.  Results are bit-identical either way.
static constexpr bool kChainLdsDefault = false;

// ---------------------------------------------------------------------------
// the launch path: exec_launch_steps walks the plan and hands every step to the launch_<form> of its form.  Its helpers
// are plain functions and small structs: nothing here allocates host memory.
// ---------------------------------------------------------------------------
static int record_event(Exec* E, size_t i) {
  HIPCHECK(hipEventRecord(E->events[i], E->stream));
  return CTN_OK;
}

// The timing bracket of step s (only the first `timing_slots` enqueues are bracketed): the first event is recorded when
// the bracket is built - check rc -, the second by end().
struct StepTimer {
  Exec* E;
  bool on;
  size_t ev;
  int rc;
  StepTimer(Exec* E_, int s)
      : E(E_), on(E_->timing_runs < E_->timing_slots), ev(on ? ((size_t)E_->timing_runs * E_->plan->n_steps + s) * 2 : 0),
        rc(on ? record_event(E_, ev) : CTN_OK) {}
  int end() const { return on ? record_event(E, ev + 1) : CTN_OK; }
};

// a step that launches nothing: an empty bracket
static int time_nothing(Exec* E, int s) {
  const StepTimer t(E, s);
  return t.rc != CTN_OK ? t.rc : t.end();
}

// ... because it runs inside the next launched step (the first step of a pair, a member of a sweep): the marker tile too
static int mark_absorbed(Exec* E, int s) {
  E->launched_tile[s] = (1 << 16) | 1;
  return time_nothing(E, s);
}

static void report_tile(Exec* E, int s, int tm, int tn) { E->launched_tile[s] = (tm << 16) | tn; }

// step s's region of the partial sums, and its slots per replica
static double* part_region(Exec* E, int s) { return E->d_partials + (size_t)E->forms.step_off[s] * E->R; }

// The partials of tensor `id`'s producer - unless the tensor is a network input (or absent), carries scale 1 (eager
// mode: normalised in place), or was never written (CTN_KERNEL_FUSED)
static void producer_partials(Exec* E, int id, const double** p, int32_t* cnt, int32_t* stride, double* numel) {
  const Plan& P = *E->plan;
  *p = nullptr; *cnt = 0; *stride = 0; *numel = 1;
  if (id >= P.n_inputs && P.stabilize && !E->eager_rescale && P.steps[P.tensors[id].producer].kernel != CTN_KERNEL_FUSED) {
    const int ps = P.tensors[id].producer;
    *p = part_region(E, ps);
    *cnt = *stride = E->forms.step_partials[ps];
    *numel = (double)P.tensors[id].numel;
  }
}

// CTN_DEBUG_STAMPS: the stamp buffer for a launch of `need` workgroups, zeroed, into *dbg (untouched when step s is not stamped)
static int stamp_buffer(Exec* E, int s, size_t need, unsigned long long** dbg) {
  if (!E->sw.stamps || (E->sw.stamp_step >= 0 && E->sw.stamp_step != s)) return CTN_OK;
  if (E->dbg_tiles < need) {
    if (E->d_dbg) (void)hipFree(E->d_dbg);
    HIPCHECK(hipMalloc((void**)&E->d_dbg, need * 64));
    E->dbg_tiles = need;
  }
  *dbg = E->d_dbg;
  HIPCHECK(hipMemsetAsync(E->d_dbg, 0, E->dbg_tiles * 64, E->stream));
  return CTN_OK;
}

static void launch_renorm(Exec* E, int s);

// the arguments every kernel of a plain step takes, as the planner's own launch of the step would have them
static void fill_step_args(Exec* E, int s, StepArgs* args) {
  const Plan& P = *E->plan;
  const Step& st = P.steps[s];
  StepArgs& a = *args;
  const int32_t* T = E->d_tables;
  const int64_t* T8 = E->d_tables64;
  a.obA = T8 + st.t.obA; a.obB = T8 + st.t.obB; a.obC = T8 + st.t.obC;
  a.omA = T + st.t.omA; a.omC = T + st.t.omC;
  a.onB = T + st.t.onB; a.onC = T + st.t.onC;
  a.okA = T + st.t.okA; a.okB = T + st.t.okB;
  a.ptrs = E->d_ptrs;
  producer_partials(E, st.lhs, &a.partA, &a.PA, &a.strideA, &a.numelA);
  producer_partials(E, st.rhs, &a.partB, &a.PB, &a.strideB, &a.numelB);
  producer_partials(E, st.lhs2, &a.partA2, &a.PA2, &a.strideA2, &a.numelA2);
  a.obA2 = T8 + st.t.obA2; a.omA2 = T + st.t.omA2; a.okA2 = T + st.t.okA2;
  a.idA2 = st.lhs2 >= 0 ? st.lhs2 : E->n_tensors - 1;
  a.krX = st.krX; a.krY = st.krY;
  a.epw = st.epw | (st.epw_split ? 0x100 : 0);
  // more workgroup partials than slots: through the scratch buffer and k_collapse
  a.partC = st.collapse ? E->d_scratch : part_region(E, s);
  a.partC_stride = st.collapse ? st.blocks : E->forms.step_partials[s];
  a.min_norm = P.min_norm;
  a.Bt = (int32_t)st.Bt; a.M = (int32_t)st.M; a.N = (int32_t)st.N; a.K = (int32_t)st.K;
  a.idA = st.lhs; a.idB = st.rhs >= 0 ? st.rhs : E->n_tensors - 1; a.idC = st.out;
  a.n_tensors = E->n_tensors;
  const int row_tile = (st.kernel == CTN_KERNEL_MFMA_F32 && st.tileM == 64) ? 64 : kTileM;
  a.tiles_m = (int32_t)((st.M + row_tile - 1) / row_tile);
  a.tiles_n = (int32_t)((st.N + kTileN - 1) / kTileN);
  a.blocks_per_replica = st.blocks;
  a.R = E->R;
  a.c_vec = (st.cvec && (s + 1 < P.n_steps || E->outs_aligned16)) ? 1 : 0;
  a.dbg = nullptr;
  a.ks_slab = nullptr; a.ks_numelC = 0; a.ks_S = 0; a.ks_chunk = 0;
  a.ohA = T8 + st.t.ohA; a.ohB = T8 + st.t.ohB; a.ohC = T8 + st.t.ohC;
  a.olA = T + st.t.olA; a.olB = T + st.t.olB; a.olC = T + st.t.olC;
  a.H = (int32_t)st.H; a.L = (int32_t)st.L; a.Nv = (int32_t)st.Nv;
  a.sAn = (int32_t)st.sAn; a.sBn = (int32_t)st.sBn;
  a.dNq = make_fastdiv((st.Nv + st.vecw - 1) / st.vecw);
  a.dL = make_fastdiv(st.L);
  a.dNv = make_fastdiv(st.Nv);
}

// a chain plan: the whole walk is one launch, timed as "step 0"
static int launch_chain(Exec* E) {
  const Plan& P = *E->plan;
  const int R = E->R;
  const StepTimer t(E, 0);
  if (t.rc != CTN_OK) return t.rc;
  if (E->d_chain_prog && P.dtype == CTN_F32)
    hipLaunchKernelGGL(k_chain_lds<float>, dim3(R), dim3(256), 0, E->stream, (const int32_t*)E->d_chain_prog, E->chain_len0, P.n_steps,
                       (void* const*)E->d_ptrs, E->n_tensors, E->d_partials, R, P.min_norm, P.stabilize ? 1 : 0);
  else if (E->d_chain_prog)
    hipLaunchKernelGGL(k_chain_lds<double>, dim3(R), dim3(256), 0, E->stream, (const int32_t*)E->d_chain_prog, E->chain_len0, P.n_steps,
                       (void* const*)E->d_ptrs, E->n_tensors, E->d_partials, R, P.min_norm, P.stabilize ? 1 : 0);
  else if (P.dtype == CTN_F32)
    hipLaunchKernelGGL(k_chain<float>, dim3(R), dim3(256), 0, E->stream, (const ChainStep*)E->d_chain, P.n_steps,
                       (void* const*)E->d_ptrs, E->n_tensors, E->d_partials, R, P.min_norm, P.stabilize ? 1 : 0);
  else
    hipLaunchKernelGGL(k_chain<double>, dim3(R), dim3(256), 0, E->stream, (const ChainStep*)E->d_chain, P.n_steps,
                       (void* const*)E->d_ptrs, E->n_tensors, E->d_partials, R, P.min_norm, P.stabilize ? 1 : 0);
  return t.end();
}

// a group of leaf steps whose arguments are in device memory
static void launch_group(Exec* E, const LeafGroup& G) {
  const dim3 g(G.blocks, E->R, G.len);
  if (E->plan->dtype == CTN_F32) launch_stream_group<float>(G.vw, G.u, g, E->stream, E->d_group_args + G.off);
  else launch_stream_group<double>(G.vw, G.u, g, E->stream, E->d_group_args + G.off);
}

// the scale bookkeeping behind a sweep kernel that leaves the records of k_sweep_f64 (rec_a, rec_e): the members' rescale
// factors, then the result's rows at their common scale.  <T, TWO>: the rows' element type; two member steps per site or one
template <typename T, bool TWO>
static void launch_sweep64_finish(Exec* E) {
  const Plan& P = *E->plan;
  const int R = E->R;
  const SweepDesc& sd = E->forms.sweep;
  const int S = sd.sites();
  const double numelE = (double)P.tensors[sd.idOut].numel, numelC = numelE * sd.Pd;
  hipLaunchKernelGGL(k_sweep64_z<TWO>, dim3((unsigned)sd.steps.size(), (unsigned)R), dim3(256), 0, E->stream, (const double*)E->d_sweep_a,
                     (const int32_t*)E->d_sweep_e, S, sd.J, numelC, numelE, E->d_sweep_z);
  Sweep64Finish f{};
  f.ptrs = E->d_ptrs; f.n_tensors = E->n_tensors; f.idOut = sd.idOut; f.S = S; f.J = sd.J; f.R = R; f.D = sd.D; f.M = sd.M;
  f.ldOut = sd.ldOut; f.Z = E->d_sweep_z; f.rec_e = E->d_sweep_e; f.part_off = E->d_sweep_off;
  f.part_slots = E->d_sweep_slots; f.partials = E->d_partials; f.numelC = numelC; f.numelE = numelE;
  f.min_norm = P.stabilize ? P.min_norm : INFINITY;
  hipLaunchKernelGGL((k_sweep64_finish<T, TWO>), dim3((unsigned)sd.J, (unsigned)R), dim3(256), 0, E->stream, f);
}

// What the argument structs of the three sweep kernels share (SweepArgs, Sweep64Args, SweepSmallArgs: the same field
// names), filled from the descriptor alone - and the tile the run reports at its last member s: 16 rows x all columns of
// C (1024 at bond 256, d = 4) per workgroup, every site
template <typename Args>
static Args sweep_args(Exec* E, int s) {
  const SweepDesc& sd = E->forms.sweep;
  Args w{};
  w.ptrs = E->d_ptrs; w.n_tensors = E->n_tensors; w.site_ids = E->d_sweep_ids;
  w.idIn = sd.idIn; w.idOut = sd.idOut; w.S = sd.sites(); w.J = sd.J; w.M = sd.M;
  w.ldIn = sd.ldIn; w.ldOut = sd.ldOut; w.ldWl = sd.ldWl; w.ldWp = sd.ldWp; w.ldX = sd.ldX;
  producer_partials(E, sd.idIn, &w.partIn, &w.PIn, &w.strideIn, &w.numelIn);
  w.min_norm = E->plan->min_norm;
  w.rec_a = E->d_sweep_a;
  report_tile(E, s, SWR, sd.D * sd.Pd);
  return w;
}

// The ONE ladder behind the sweep kernels' instantiations: f(I, P) with the run-time bond index i = 0 .. 3 and physical
// dimension 2 or 4 as std::integral_constant arguments
template <typename F>
static void sweep_pick(int i, int Pd, F f) {
  auto bond = [&](auto P) {
    if (i == 0) f(std::integral_constant<int, 0>(), P);
    else if (i == 1) f(std::integral_constant<int, 1>(), P);
    else if (i == 2) f(std::integral_constant<int, 2>(), P);
    else f(std::integral_constant<int, 3>(), P);
  };
  if (Pd == 4) bond(std::integral_constant<int, 4>());
  else bond(std::integral_constant<int, 2>());
}

// the last member of a sweep: the whole chain in one launch, then its scale bookkeeping
static int launch_sweep_run(Exec* E, int s) {
  const int R = E->R;
  const SweepDesc& sd = E->forms.sweep;
  const dim3 gs((unsigned)sd.J, (unsigned)R);
  if (sd.small) {
    // small bonds (float: CTN_SWEEP_SMALL=1, double: CTN_SWEEP_SMALL64=1): 16 values of the bond per index step, one wave per
    // workgroup; `tr`: the cores are stored with the contracted bond unit-stride
    SweepSmallArgs w = sweep_args<SweepSmallArgs>(E, s);
    w.D = sd.D; w.rec_e = E->d_sweep_e;
    E->launched_form[s] = sd.f64 ? CTN_FORM_SWEEP_SMALL_F64 : CTN_FORM_SWEEP_SMALL;
    // <T, TWO>: S sites of two member steps each (double always) or of one
    auto run = [&](auto t, auto two) {
      using T = decltype(t);
      sweep_pick((sd.D + 15) / 16 - 1, sd.Pd, [&](auto I, auto P) {
        if (sd.tr) hipLaunchKernelGGL((k_sweep_small<T, I() + 1, P(), two(), true>), gs, dim3(64), 0, E->stream, w);
        else hipLaunchKernelGGL((k_sweep_small<T, I() + 1, P(), two()>), gs, dim3(64), 0, E->stream, w);
      });
      launch_sweep64_finish<T, two()>(E);
    };
    if (sd.f64) run(double(), std::true_type());
    else if (sd.two) run(float(), std::true_type());
    else run(float(), std::false_type());
    return CTN_OK;
  }
  const int ib = sd.D == 64 ? 0 : sd.D == 128 ? 1 : sd.D == 256 ? 2 : 3;       // bond 64 << ib
  if (sd.f64) {
    // float64: 2 S member steps, S sites
    Sweep64Args w = sweep_args<Sweep64Args>(E, s);
    w.rec_e = E->d_sweep_e;
    sweep_pick(ib, sd.Pd, [&](auto I, auto P) {
      hipLaunchKernelGGL((k_sweep_f64<(64 << I()), P()>), gs, dim3(Sweep64Shape<(64 << I())>::NT), 0, E->stream, w);
    });
    launch_sweep64_finish<double, true>(E);
    return CTN_OK;
  }
  const Plan& P = *E->plan;
  const int S = sd.sites();
  SweepArgs w = sweep_args<SweepArgs>(E, s);
  w.rec_s = E->d_sweep_s; w.dbg = nullptr;
  const int rc = stamp_buffer(E, s, (size_t)sd.J * R, &w.dbg);
  if (rc != CTN_OK) return rc;
  sweep_pick(ib, sd.Pd, [&](auto I, auto Pd) {
    hipLaunchKernelGGL((k_sweep_f32<(64 << I()), Pd()>), gs, dim3(I() == 0 ? 256 : 512), 0, E->stream, w);
  });
  const double numel = (double)P.tensors[sd.idOut].numel;
  hipLaunchKernelGGL(k_sweep_logs, dim3((unsigned)S, (unsigned)R), dim3(256), 0, E->stream, (const double*)E->d_sweep_a,
                     (const float*)E->d_sweep_s, S, sd.J, E->d_sweep_la, E->d_sweep_ls);
  hipLaunchKernelGGL(k_sweep_z, dim3((unsigned)S, (unsigned)R), dim3(256), 0, E->stream, (const double*)E->d_sweep_la,
                     (const double*)E->d_sweep_ls, S, sd.J, numel, E->d_sweep_z);
  SweepFinish f{};
  f.ptrs = E->d_ptrs; f.n_tensors = E->n_tensors; f.idOut = sd.idOut; f.S = S; f.J = sd.J; f.R = R; f.D = sd.D; f.M = sd.M;
  f.ldOut = sd.ldOut; f.Z = E->d_sweep_z; f.ls = E->d_sweep_ls; f.part_off = E->d_sweep_off;
  f.part_slots = E->d_sweep_slots; f.partials = E->d_partials; f.numel = numel;
  f.min_norm = P.stabilize ? P.min_norm : INFINITY;
  hipLaunchKernelGGL(k_sweep_finish, dim3((unsigned)sd.J, (unsigned)R), dim3(256), 0, E->stream, f);
  return CTN_OK;
}

// a step of a sweep: the members before the last launch nothing, the last one launches the run
static int launch_sweep_member(Exec* E, int s) {
  if (E->forms.sweep_role[s] == 1) return mark_absorbed(E, s);
  const StepTimer t(E, s);
  if (t.rc != CTN_OK) return t.rc;
  const int rc = launch_sweep_run(E, s);
  return rc != CTN_OK ? rc : t.end();
}

// a float64 zipper pair in its latency form (k_zip_lat_f64, CTN_ZIPL64=1): the same launch on the same descriptors
static int launch_zip_lat_f64(Exec* E, int s) {
  const Plan& P = *E->plan;
  const Step& st = P.steps[s];
  const int R = E->R;
  const ZipLat& L = E->forms.zl[s];
  const ZipDesc& zd = L.d;
  const Step& s1 = P.steps[s - 1];
  const int S = ZLD_S, nub = zd.U / 16;
  const bool eager = E->eager_rescale;
  ZipLat64Args z{};
  z.ptrs = E->d_ptrs; z.n_tensors = E->n_tensors;
  z.idE = s1.lhs; z.idX = s1.rhs; z.idY = st.rhs;
  z.slabs_in = (L.from_prev && !eager) ? (const double*)E->d_zl_slab[L.buf ^ 1] : nullptr;
  z.slabs_out = (double*)E->d_zl_slab[L.buf];
  z.ldE = zd.ldE; z.ldXq = zd.ldXq; z.ldXk = zd.ldXk; z.ldYq = zd.ldYq; z.ldYm = zd.ldYm;
  z.U = zd.U; z.R = R;
  producer_partials(E, s1.lhs, &z.partE, &z.PE, &z.strideE, &z.numelE);
  z.min_norm = P.min_norm;
  z.partC = part_region(E, s);
  z.partC_stride = E->forms.step_partials[s];
  const StepTimer t(E, s);
  if (t.rc != CTN_OK) return t.rc;
  E->launched_form[s] = CTN_FORM_ZIPL_F64;
  report_tile(E, s, L.mp, ZM);      // (m1 part, all n2) per workgroup, 16 values of u: no plain fp64 form reports it
  const dim3 gz((unsigned)((int64_t)R * nub * S));
  if (zd.Q == 4 && z.slabs_in) hipLaunchKernelGGL((k_zip_lat_f64<4, true>), gz, dim3(512), 0, E->stream, z);
  else if (zd.Q == 4) hipLaunchKernelGGL((k_zip_lat_f64<4, false>), gz, dim3(512), 0, E->stream, z);
  else if (z.slabs_in) hipLaunchKernelGGL((k_zip_lat_f64<2, true>), gz, dim3(512), 0, E->stream, z);
  else hipLaunchKernelGGL((k_zip_lat_f64<2, false>), gz, dim3(512), 0, E->stream, z);
  if (!L.feeds_next || eager) {                 // nobody adds these slabs up while loading them: do it here
    hipLaunchKernelGGL(k_zip_slab_sum_f64, dim3((unsigned)E->forms.step_partials[s], (unsigned)R), dim3(256), 0, E->stream,
                       (const double*)z.slabs_out, S, zd.U, (void* const*)E->d_ptrs, E->n_tensors, st.out, zd.ldC, z.partC,
                       z.partC_stride);
    launch_renorm(E, s);
  }
  return t.end();
}

// a zipper pair in its latency form (k_zip_lat): steps (s - 1, s) as one launch, the result leaving as slabs
static int launch_zip_lat(Exec* E, int s) {
  const Plan& P = *E->plan;
  if (P.dtype == CTN_F64) return launch_zip_lat_f64(E, s);
  const Step& st = P.steps[s];
  const int R = E->R;
  const ZipLat& L = E->forms.zl[s];
  const ZipDesc& zd = L.d;
  const Step& s1 = P.steps[s - 1];
  const int S = ZM / L.mp, nub = zd.U / 16;
  const bool eager = E->eager_rescale;
  ZipLatArgs z{};
  z.ptrs = E->d_ptrs; z.n_tensors = E->n_tensors;
  z.idE = s1.lhs; z.idX = s1.rhs; z.idY = st.rhs;
  z.slabs_in = (L.from_prev && !eager) ? (const float*)E->d_zl_slab[L.buf ^ 1] : nullptr;
  z.slabs_out = (float*)E->d_zl_slab[L.buf];
  z.ldE = zd.ldE; z.ldXq = zd.ldXq; z.ldXk = zd.ldXk; z.ldYq = zd.ldYq; z.ldYm = zd.ldYm;
  z.U = zd.U; z.R = R;
  producer_partials(E, s1.lhs, &z.partE, &z.PE, &z.strideE, &z.numelE);
  z.min_norm = P.min_norm;
  z.partC = part_region(E, s);
  z.partC_stride = E->forms.step_partials[s];
  const StepTimer t(E, s);
  if (t.rc != CTN_OK) return t.rc;
  report_tile(E, s, L.mp, ZM);      // (m1 part, all n2) per workgroup, 16 values of u
  const dim3 gz((unsigned)((int64_t)R * nub * S));
  z.dbg = nullptr;
  const int rc = stamp_buffer(E, s, (size_t)gz.x, &z.dbg);
  if (rc != CTN_OK) return rc;
  if (zd.Q == 4 && L.mp == 32) hipLaunchKernelGGL((k_zip_lat<4, 32>), gz, dim3(512), 0, E->stream, z);
  else if (zd.Q == 4) hipLaunchKernelGGL((k_zip_lat<4, 64>), gz, dim3(512), 0, E->stream, z);
  else hipLaunchKernelGGL((k_zip_lat<2, 64>), gz, dim3(512), 0, E->stream, z);
  if (!L.feeds_next || eager) {                 // nobody adds these slabs up while loading them: do it here
    hipLaunchKernelGGL(k_zip_slab_sum, dim3((unsigned)E->forms.step_partials[s], (unsigned)R), dim3(256), 0, E->stream,
                       (const float*)z.slabs_out, S, zd.U, (void* const*)E->d_ptrs, E->n_tensors, st.out, zd.ldC, z.partC,
                       z.partC_stride);
    launch_renorm(E, s);
  }
  return t.end();
}

// Eager mode: normalise step s's result in place by the scale its partials give (the final tensor is normalised by k_finalize)
static void launch_renorm(Exec* E, int s) {
  const Plan& P = *E->plan;
  if (!E->eager_rescale || !P.stabilize || s + 1 >= P.n_steps) return;
  const int out = P.steps[s].out;
  const int64_t numel = P.tensors[out].numel;
  const int V = P.dtype == CTN_F64 ? 2 : 4;
  const dim3 g((unsigned)std::max<int64_t>(1, std::min<int64_t>((numel / V + 255) / 256, 2048)), E->R);
  if (P.dtype == CTN_F32)
    hipLaunchKernelGGL(k_renorm<float>, g, dim3(256), 0, E->stream, (void* const*)E->d_ptrs, E->n_tensors, out, numel,
                       (const double*)part_region(E, s), E->forms.step_partials[s], E->forms.step_partials[s], P.min_norm);
  else
    hipLaunchKernelGGL(k_renorm<double>, g, dim3(256), 0, E->stream, (void* const*)E->d_ptrs, E->n_tensors, out, numel,
                       (const double*)part_region(E, s), E->forms.step_partials[s], E->forms.step_partials[s], P.min_norm);
}

// The zipper-pair kernels by ctn_step_form: threads per workgroup, the tile ctn_exec_step_tile reports, and whether a
// workgroup walks the launch's work items (grid from zipq_grid; else one workgroup per `zu` values of u and replica).
// The tile is 128 (or 64) values of u x all 256 n2 per workgroup; k_zip_f64 (64 values of u) reports (512, 256): an fp64
// step with 128 tile columns reads as k_mfma_f64_g.  The two instantiations of k_zipm_f32 (kernels_zipm.h): k_zip128_f32
// (bond 128) reports (512, 64): the 64 values of m1 a wave sums; k_zipm64_f32 (bond 64) likewise (256, 32): its 256
// threads, 32 values of m1 per wave - a tile no plain form reports (theirs are 16 x 16 or have 64 columns at least).  k_zip512_f32 (bond 512) reports (512, 512): its 512
// threads and all 512 n2 - plain tiles have at most 256 rows, and no other pair kernel has 512 columns.  (Index 8,
// CTN_FORM_ZIPL_F64, is the float64 latency form: it has a launcher of its own and no row here.)
struct ZipKernel { void (*kernel)(ZipArgs); int threads, tm, tn; bool walks; };
static const ZipKernel kZipKernels[] = {
    {nullptr, 0, 0, 0, false},                // CTN_FORM_NONE
    {k_zip_f32, 512, 512, 256, false},        // CTN_FORM_ZIP
    {k_zipq_f32, 256, 512, 256, false},       // CTN_FORM_ZIPQ
    {k_zip64_f32, 512, 512, 128, false},      // CTN_FORM_ZIP64
    {k_zip128_f32, 512, 512, 64, false},      // CTN_FORM_ZIP128
    {k_zipm64_f32, 256, 256, 32, false},      // CTN_FORM_ZIPM64
    {k_zip_f64, 512, 512, 256, false},        // CTN_FORM_ZIP_F64
    {k_zipqp_f32, 256, 512, 256, true},       // CTN_FORM_ZIPQP
    {nullptr, 0, 0, 0, false},                // CTN_FORM_ZIPL_F64: launch_zip_lat's
    {k_zip512_f32, 512, 512, 512, false},     // CTN_FORM_ZIP512
};
static_assert(CTN_FORM_ZIP == 1 && CTN_FORM_ZIPQ == 2 && CTN_FORM_ZIP64 == 3 && CTN_FORM_ZIP128 == 4 && CTN_FORM_ZIPM64 == 5 &&
              CTN_FORM_ZIP_F64 == 6 && CTN_FORM_ZIPQP == 7 && CTN_FORM_ZIPL_F64 == 8 && CTN_FORM_ZIP512 == 9 &&
                  sizeof(kZipKernels) / sizeof(kZipKernels[0]) == 10,
              "kZipKernels is indexed by ctn_step_form");

// a zipper pair: steps (s - 1, s) as one launch
static int launch_zip(Exec* E, int s) {
  const Plan& P = *E->plan;
  const Step& st = P.steps[s];
  const int R = E->R;
  const ZipDesc& zd = E->forms.zip[s];
  const ZipKernel& zk = kZipKernels[zd.form];
  const Step& s1 = P.steps[s - 1];
  ZipArgs z{};
  z.ptrs = E->d_ptrs; z.n_tensors = E->n_tensors;
  z.idE = s1.lhs; z.idX = s1.rhs; z.idY = st.rhs; z.idC = st.out;
  z.ldE = zd.ldE; z.ldXq = zd.ldXq; z.ldXk = zd.ldXk; z.ldYq = zd.ldYq; z.ldYm = zd.ldYm; z.ldC = zd.ldC;
  z.K1 = zd.K1; z.Q = zd.Q; z.U = zd.U;
  producer_partials(E, s1.lhs, &z.partE, &z.PE, &z.strideE, &z.numelE);
  z.min_norm = P.min_norm;
  z.partC = part_region(E, s);
  z.partC_stride = E->forms.step_partials[s];
  z.R = R; z.dbg = nullptr;
  z.n_items = (int32_t)zipq_items(R, zd.U, zd.zu);
  const StepTimer t(E, s);
  if (t.rc != CTN_OK) return t.rc;
  E->launched_form[s] = zd.form;
  report_tile(E, s, zk.tm, zk.tn);
  const int per = zd.U / zd.zu;
  const int rc = stamp_buffer(E, s, (size_t)per * R, &z.dbg);
  if (rc != CTN_OK) return rc;
  const int64_t wgs = zk.walks ? zipq_grid(z.n_items, E->n_cu, E->sw.zipq_wgs) : (int64_t)per * R;
  hipLaunchKernelGGL(zk.kernel, dim3((unsigned)wgs), dim3(zk.threads), 0, E->stream, z);
  launch_renorm(E, s);
  return t.end();
}

// what the launch of a plain step leaves for its tail: partials in the scratch buffer that k_collapse folds
struct Collapse { bool on; int blocks; };

// A complex x complex step: the S step before it and this GEMM as one launch (k_cmfma_f32), reading `small`
// and `big` as arrays of pairs; the scales are those of `small` (not of the never-written mid) and of `big`
static int launch_cplx(Exec* E, int s, Collapse* col) {
  const Plan& P = *E->plan;
  const int R = E->R;
  const CplxDesc& cd = E->forms.cplx[s];
  const int32_t* CT = E->d_cplx_tabs;
  CplxArgs c{};
  c.txr = CT + cd.txr; c.txk = CT + cd.txk; c.tyn = CT + cd.tyn; c.tyk = CT + cd.tyk; c.tcx = CT + cd.tcx; c.tcy = CT + cd.tcy;
  c.ptrs = E->d_ptrs;
  producer_partials(E, cd.small, &c.partX, &c.PX, &c.strideX, &c.numelX);
  producer_partials(E, cd.big, &c.partY, &c.PY, &c.strideY, &c.numelY);
  c.min_norm = P.min_norm;
  c.Mx = cd.Mx; c.Ny = cd.Ny; c.Kc = cd.Kc;
  c.idX = cd.small; c.idY = cd.big; c.idS = cd.sid; c.idC = P.steps[s].out; c.n_tensors = E->n_tensors;
  c.tiles_x = (cd.Mx + CX_TX - 1) / CX_TX; c.tiles_y = (cd.Ny + CX_TY - 1) / CX_TY;
  c.blocks_per_replica = c.tiles_x * c.tiles_y; c.R = R;
  c.sa = cd.sa; c.sb = cd.sb; c.so = cd.so; c.sO = cd.sO; c.legx = cd.legx; c.legy = cd.legy;
  c.c_vec2 = (cd.cvec2 && (s + 1 < P.n_steps || E->outs_aligned16)) ? 1 : 0;
  col->on = c.blocks_per_replica > kMaxPartials;       // more workgroups than slots: through the collapse pass
  col->blocks = c.blocks_per_replica;
  c.partC = col->on ? E->d_scratch : part_region(E, s);
  c.partC_stride = col->on ? col->blocks : E->forms.step_partials[s];
  report_tile(E, s, CX_TX, 2 * CX_TY);   // 64 pairs of `small` x (128 entries of `big` x 2 components): no plain form reports it
  const dim3 gc((unsigned)((int64_t)c.blocks_per_replica * R));
  if (cd.kfx && cd.kfy) hipLaunchKernelGGL((k_cmfma_f32<true, true>), gc, dim3(256), 0, E->stream, c);
  else if (cd.kfx) hipLaunchKernelGGL((k_cmfma_f32<true, false>), gc, dim3(256), 0, E->stream, c);
  else if (cd.kfy) hipLaunchKernelGGL((k_cmfma_f32<false, true>), gc, dim3(256), 0, E->stream, c);
  else hipLaunchKernelGGL((k_cmfma_f32<false, false>), gc, dim3(256), 0, E->stream, c);
  return CTN_OK;
}

// The left operand resident in registers, `ntw` column tiles per workgroup (k_mfma_f32_ares); one partial per
// workgroup through the collapse pass the step has anyway
static int launch_ares(Exec* E, int s, StepArgs& a, int ntw_av, Collapse* col) {
  const Step& st = E->plan->steps[s];
  const int ntw = ntw_av & 0xffff, avec = ntw_av >> 16;
  const int wgs = (int)(st.Bt * (st.N / AR_TN / ntw));
  a.partC = E->d_scratch; a.partC_stride = wgs;
  col->on = true; col->blocks = wgs;
  report_tile(E, s, 256, std::min(AR_TN * ntw, 32768));
  const dim3 ga((unsigned)((int64_t)wgs * E->R));
  if (st.modeB == 2) {
    if (avec) hipLaunchKernelGGL((k_mfma_f32_ares<2, 1>), ga, dim3(512), 0, E->stream, a, ntw);
    else hipLaunchKernelGGL((k_mfma_f32_ares<2, 0>), ga, dim3(512), 0, E->stream, a, ntw);
  } else {
    if (avec) hipLaunchKernelGGL((k_mfma_f32_ares<1, 1>), ga, dim3(512), 0, E->stream, a, ntw);
    else hipLaunchKernelGGL((k_mfma_f32_ares<1, 0>), ga, dim3(512), 0, E->stream, a, ntw);
  }
  return CTN_OK;
}

// ---- the kinds of launch_form.h.  Each takes the step's arguments as fill_step_args left them and the form. ----

// the slabs of a K split over workgroups, as the form laid them out
static SplitKArgs slab_args(Exec* E, int s, const StepForm& f) {
  const Plan& P = *E->plan;
  SplitKArgs sk{};
  sk.slab = E->d_slab;
  sk.numelC = P.tensors[P.steps[s].out].numel;
  sk.kchunk = f.kchunk;
  sk.S = form_splits(P.steps[s], f);           // (empty trailing splits dropped)
  return sk;
}

// k_mfma_f32_g on 256 x 128 tiles: hand-scheduled blocks for whole k-tiles, the C++ loop (which masks a ragged last
// k-tile) otherwise
static void launch_g_tiles(Exec* E, const Step& st, const StepArgs& a, bool use_asm) {
  const dim3 gg((unsigned)((int64_t)a.blocks_per_replica * E->R));
#define CTN_G_LAUNCH(AA, BB)                                                                             \
  do {                                                                                                   \
    if (use_asm) hipLaunchKernelGGL((k_mfma_f32_g<4, 2, true, AA, BB>), gg, dim3(256), 0, E->stream, a); \
    else hipLaunchKernelGGL((k_mfma_f32_g<4, 2, false, AA, BB>), gg, dim3(256), 0, E->stream, a);        \
  } while (0)
  if (st.modeA == 2 && st.modeB == 1) CTN_G_LAUNCH(2, 1);
  else if (st.modeA == 1 && st.modeB == 2) CTN_G_LAUNCH(1, 2);
  else if (st.modeA == 2 || st.modeB == 2) CTN_G_LAUNCH(2, 2);
  else CTN_G_LAUNCH(1, 1);
#undef CTN_G_LAUNCH
}

static int launch_gsplitk(Exec* E, int s, StepArgs& a, const StepForm& f) {
  const Step& st = E->plan->steps[s];
  const SplitKArgs sk = slab_args(E, s, f);
  a.ks_slab = sk.slab; a.ks_numelC = sk.numelC; a.ks_S = sk.S; a.ks_chunk = sk.kchunk;
  launch_g_tiles(E, st, a, !E->sw.g_no_asm);           // (every split is whole k-tiles)
  a.ks_slab = nullptr; a.ks_S = 0;
  launch_splitk_reduce<float>(E, E->forms.step_partials[s], E->R, a, sk);
  return CTN_OK;
}

// one partial per tile, written directly
static int launch_lat(Exec* E, int s, StepArgs& a, const StepForm& f) {
  const dim3 g((unsigned)(f.blocks * E->R));
  if (f.T == 16) hipLaunchKernelGGL((k_mfma_lat<16, float>), g, dim3(512), 0, E->stream, a, f.kchunk);
  else if (f.T == 32) hipLaunchKernelGGL((k_mfma_lat<32, float>), g, dim3(512), 0, E->stream, a, f.kchunk);
  else hipLaunchKernelGGL((k_mfma_lat<64, float>), g, dim3(512), 0, E->stream, a, f.kchunk);
  return CTN_OK;
}

// one partial per tile (<= kMaxPartials)
static int launch_h(Exec* E, int s, StepArgs& a, const StepForm& f) {
  const Step& st = E->plan->steps[s];
  const int rc = stamp_buffer(E, s, (size_t)f.blocks * E->R, &a.dbg);
  if (rc != CTN_OK) return rc;
  const dim3 gh((unsigned)(f.blocks * E->R));
#define CTN_H_LAUNCH(AA, BB)                                                                        \
  do {                                                                                              \
    if (st.epw == 4) hipLaunchKernelGGL((k_mfma_f32_h<AA, BB, 4>), gh, dim3(512), 0, E->stream, a);      \
    else if (st.epw == 2) hipLaunchKernelGGL((k_mfma_f32_h<AA, BB, 2>), gh, dim3(512), 0, E->stream, a); \
    else hipLaunchKernelGGL((k_mfma_f32_h<AA, BB, 0>), gh, dim3(512), 0, E->stream, a);                  \
  } while (0)
  if (st.modeA == 2 && st.modeB == 2) CTN_H_LAUNCH(2, 2);
  else if (st.modeA == 2) CTN_H_LAUNCH(2, 1);
  else if (st.modeB == 2) CTN_H_LAUNCH(1, 2);
  else CTN_H_LAUNCH(1, 1);
#undef CTN_H_LAUNCH
  return CTN_OK;
}

// the three throughput forms of an fp32 GEMM step: 256 x 256 and 256 x 128 tiles fed by LDS-DMA, register-staged tiles
static int launch_tiles(Exec* E, int s, StepArgs& a, const StepForm& f) {
  const Step& st = E->plan->steps[s];
  static_assert(GM == 256 && GN == kTileN && GK == 16 && 2 * GK == 32, "planner eligibility rule (plan.cpp) assumes these");
  const int rc = stamp_buffer(E, s, (size_t)st.blocks * E->R, &a.dbg);
  if (rc != CTN_OK) return rc;
  if (f.kind == Kind::G256)
    hipLaunchKernelGGL((k_mfma_f32_g<8, 2, true>), dim3((unsigned)(f.blocks * E->R)), dim3(512), 0, E->stream, a);
  else if (f.kind == Kind::G128)
    launch_g_tiles(E, st, a, st.K % GK == 0 && !E->sw.g_no_asm);
  else   // (halved tiles beyond the slots collapse; else the region has one slot per tile: step_form sized it by this form)
    launch_mfma(st.modeA, st.modeB, f.tm, f.tn, dim3((unsigned)(f.blocks * E->R)), E->stream, a, E->sw);
  return CTN_OK;
}

static int launch_lat64(Exec* E, int s, StepArgs& a, const StepForm& f) {
  hipLaunchKernelGGL((k_mfma_lat<16, double>), dim3((unsigned)(f.blocks * E->R)), dim3(512), 0, E->stream, a, f.kchunk);
  return CTN_OK;
}

// the reduce pass of a K split over workgroups, in the plan's precision
static void launch_reduce(Exec* E, int s, StepArgs& a, const SplitKArgs& sk) {
  if (E->plan->dtype == CTN_F32) launch_splitk_reduce<float>(E, E->forms.step_partials[s], E->R, a, sk);
  else launch_splitk_reduce<double>(E, E->forms.step_partials[s], E->R, a, sk);
}

// the latency mode of either precision: 64 x 64 tiles, K split over workgroups
static int launch_splitk(Exec* E, int s, StepArgs& a, const StepForm& f) {
  const Step& st = E->plan->steps[s];
  SplitKArgs sk = slab_args(E, s, f);
  sk.tiles_m = (int32_t)((st.M + 63) / 64);
  sk.tiles_n = (int32_t)((st.N + 63) / 64);
  sk.tiles_per_replica = (int32_t)(st.Bt * sk.tiles_m * sk.tiles_n);
  const dim3 g((unsigned)(f.blocks * E->R));
  if (f.kind == Kind::SplitK) launch_sk(st.modeA, st.modeB, g, E->stream, a, sk);
  else launch_sk64(st.modeA, st.modeB, g, E->stream, a, sk);
  launch_reduce(E, s, a, sk);
  return CTN_OK;
}

// fp64 GEMM tiles: 128 x 128 fed by LDS-DMA (k_mfma_f64_g), or the planner's own 128 x 64
static int launch_tiles64(Exec* E, int s, StepArgs& a, const StepForm& f) {
  const Step& st = E->plan->steps[s];
  const dim3 g((unsigned)(f.blocks * E->R)), b(256);
  if (f.kind == Kind::G64) {
    if (st.modeA == 2 && st.modeB == 2) hipLaunchKernelGGL((k_mfma_f64_g<2, 2>), g, b, 0, E->stream, a);
    else if (st.modeA == 2) hipLaunchKernelGGL((k_mfma_f64_g<2, 1>), g, b, 0, E->stream, a);
    else if (st.modeB == 2) hipLaunchKernelGGL((k_mfma_f64_g<1, 2>), g, b, 0, E->stream, a);
    else hipLaunchKernelGGL((k_mfma_f64_g<1, 1>), g, b, 0, E->stream, a);
    return CTN_OK;
  }
#define CTN_F64(AA, BB) hipLaunchKernelGGL((k_mfma_f64<AA, BB>), g, b, 0, E->stream, a)
  switch (st.modeA * 3 + st.modeB) {
    case 0: CTN_F64(0, 0); break; case 1: CTN_F64(0, 1); break; case 2: CTN_F64(0, 2); break;
    case 3: CTN_F64(1, 0); break; case 4: CTN_F64(1, 1); break; case 5: CTN_F64(1, 2); break;
    case 6: CTN_F64(2, 0); break; case 7: CTN_F64(2, 1); break; default: CTN_F64(2, 2); break;
  }
#undef CTN_F64
  return CTN_OK;
}

static int launch_dot(Exec* E, int s, StepArgs& a, const StepForm& f) {
  const Plan& P = *E->plan;
  const Step& st = P.steps[s];
  const int R = E->R;
  if (f.kind == Kind::DotSplit) {
    const SplitKArgs sk = slab_args(E, s, f);
    const dim3 g((unsigned)f.blocks, R);
    const DotTr& dt = E->forms.dot_tr[s];
    if (P.dtype == CTN_F32) {
      if (dt.on) hipLaunchKernelGGL(k_dot_tr<float>, g, dim3(256), 0, E->stream, a, (float*)sk.slab, sk.numelC, sk.S, dt.Ka, dt.Kb, dt.ldY, dt.x_is_a);
      else hipLaunchKernelGGL(k_dot_split<float>, g, dim3(256), 0, E->stream, a, (float*)sk.slab, sk.numelC, sk.S, sk.kchunk);
    } else {
      if (dt.on) hipLaunchKernelGGL(k_dot_tr<double>, g, dim3(256), 0, E->stream, a, (double*)sk.slab, sk.numelC, sk.S, dt.Ka, dt.Kb, dt.ldY, dt.x_is_a);
      else hipLaunchKernelGGL(k_dot_split<double>, g, dim3(256), 0, E->stream, a, (double*)sk.slab, sk.numelC, sk.S, sk.kchunk);
    }
    launch_reduce(E, s, a, sk);
    return CTN_OK;
  }
  if (P.dtype == CTN_F32) hipLaunchKernelGGL(k_dot<float>, dim3(st.blocks, R), dim3(256), 0, E->stream, a);
  else hipLaunchKernelGGL(k_dot<double>, dim3(st.blocks, R), dim3(256), 0, E->stream, a);
  return CTN_OK;
}

// A streaming or row-dot step with its K split over workgroups (f.S > 0): the kernel writes slabs ...
static SplitKArgs split_stream_args(Exec* E, int s, StepArgs& a, const StepForm& f) {
  SplitKArgs sk{};
  if (f.S) {
    sk = slab_args(E, s, f);
    a.ks_slab = sk.slab; a.ks_numelC = sk.numelC; a.ks_S = sk.S; a.ks_chunk = sk.kchunk;
  }
  return sk;
}

// ... and the reduce pass writes the step's region itself
static void reduce_split_stream(Exec* E, int s, StepArgs& a, const StepForm& f, const SplitKArgs& sk) {
  if (!f.S) return;
  a.partC = part_region(E, s); a.partC_stride = E->forms.step_partials[s];
  launch_reduce(E, s, a, sk);
}

static int launch_rowdot(Exec* E, int s, StepArgs& a, const StepForm& f) {
  const SplitKArgs sk = split_stream_args(E, s, a, f);
  const dim3 g(E->plan->steps[s].blocks, E->R, f.S ? sk.S : 1);
  if (E->plan->dtype == CTN_F32) hipLaunchKernelGGL(k_rowdot<float>, g, dim3(256), 0, E->stream, a);
  else hipLaunchKernelGGL(k_rowdot<double>, g, dim3(256), 0, E->stream, a);
  reduce_split_stream(E, s, a, f, sk);
  return CTN_OK;
}

static int launch_stream_kvec(Exec* E, int s, StepArgs& a) {
  const dim3 g(E->plan->steps[s].blocks, E->R);
  if (E->plan->dtype == CTN_F32) hipLaunchKernelGGL(k_stream_kvec<float>, g, dim3(256), 0, E->stream, a);
  else hipLaunchKernelGGL(k_stream_kvec<double>, g, dim3(256), 0, E->stream, a);
  return CTN_OK;
}

// the first enqueue of a leaf group: its steps' arguments are kept, the last one uploads and launches the group
struct GroupCollect { int left = 0, head = -1; };

static int launch_stream(Exec* E, int s, StepArgs& a, const StepForm& f, GroupCollect* gc) {
  const Plan& P = *E->plan;
  const Step& st = P.steps[s];
  // vector stores need a 16-byte aligned destination: the caller's final buffer may not be
  const int vw = (s + 1 == P.n_steps && !E->outs_aligned16) ? 1 : st.vecw;
  int u;
  int64_t nq;
  stream_variant(st, E->R, vw, &u, &nq);
  a.dNq = make_fastdiv(nq / u);
  if (gc->left > 0) {
    LeafGroup& G = E->forms.groups[gc->head];
    E->h_group_args[G.off + (s - gc->head)] = a;
    if (--gc->left == 0) {
      HIPCHECK(hipMemcpyAsync(E->d_group_args + G.off, E->h_group_args + G.off, sizeof(StepArgs) * G.len,
                              hipMemcpyHostToDevice, E->stream));
      G.ready = true;
      launch_group(E, G);
    }
    return CTN_OK;
  }
  const SplitKArgs sk = split_stream_args(E, s, a, f);
  const dim3 g(st.blocks, E->R, f.S ? sk.S : 1), b(256);
#define CTN_STREAM(TT, VV, UU) hipLaunchKernelGGL((k_stream<TT, VV, UU>), g, b, 0, E->stream, a)
  if (P.dtype == CTN_F32) {
    if (vw == 4) { if (u == 4) CTN_STREAM(float, 4, 4); else CTN_STREAM(float, 4, 1); }
    else { if (u == 4) CTN_STREAM(float, 1, 4); else CTN_STREAM(float, 1, 1); }
  } else {
    if (vw == 2) { if (u == 4) CTN_STREAM(double, 2, 4); else CTN_STREAM(double, 2, 1); }
    else { if (u == 4) CTN_STREAM(double, 1, 4); else CTN_STREAM(double, 1, 1); }
  }
#undef CTN_STREAM
  reduce_split_stream(E, s, a, f, sk);
  return CTN_OK;
}

// A plain step: a pair or the resident-operand kernel where the executor found one, else the form step_form gives it
// for this enqueue (the last step's depends on the caller's buffer); then the collapse pass and the eager rescale
static int launch_step(Exec* E, int s, GroupCollect* gc) {
  const Plan& P = *E->plan;
  const Step& st = P.steps[s];
  StepArgs a;
  fill_step_args(E, s, &a);
  const StepTimer t(E, s);
  if (t.rc != CTN_OK) return t.rc;
  const bool f32 = st.kernel == CTN_KERNEL_MFMA_F32;
  if ((f32 || st.kernel == CTN_KERNEL_MFMA_F64) && (int64_t)st.blocks * E->R >= (1LL << 31)) { g_err = "grid too large"; return CTN_UNSUPPORTED; }
  Collapse col{st.collapse, st.blocks};
  int rc = CTN_OK;
  if (f32 && E->forms.role[s] == Role::Cplx) {
    rc = launch_cplx(E, s, &col);
  } else if (const int ntw_av = f32 ? E->forms.ares_ntw[s] : 0) {
    rc = launch_ares(E, s, a, ntw_av, &col);
  } else {
    const StepForm f = step_form(P, s, E->R, E->n_cu, E->sw, a.c_vec != 0);
    col.on = f.collapse; col.blocks = (int)f.collapse_blocks;
    if (f.tm) {   // an MFMA kind: the tile it reports; its tiling and where its partials go follow from the form
      report_tile(E, s, f.tm, f.tn);
      if (f.kind != Kind::SplitK && f.kind != Kind::SplitK64) {   // (those tile their slabs through SplitKArgs)
        a.tiles_m = (int32_t)((st.M + f.tm - 1) / f.tm);
        a.tiles_n = (int32_t)((st.N + f.tn - 1) / f.tn);
        a.blocks_per_replica = (int32_t)f.blocks;
      }
      a.partC = f.collapse ? E->d_scratch : part_region(E, s);
      a.partC_stride = f.collapse ? (int32_t)f.collapse_blocks : E->forms.step_partials[s];
    }
    switch (f.kind) {
      case Kind::None: break;                                              // (CTN_KERNEL_FUSED never gets here)
      case Kind::GSplitK: rc = launch_gsplitk(E, s, a, f); break;
      case Kind::Lat: rc = launch_lat(E, s, a, f); break;
      case Kind::SplitK: case Kind::SplitK64: rc = launch_splitk(E, s, a, f); break;
      case Kind::H: rc = launch_h(E, s, a, f); break;
      case Kind::G256: case Kind::G128: case Kind::Plain: rc = launch_tiles(E, s, a, f); break;
      case Kind::Lat64: rc = launch_lat64(E, s, a, f); break;
      case Kind::G64: case Kind::Plain64: rc = launch_tiles64(E, s, a, f); break;
      case Kind::Dot: case Kind::DotSplit: rc = launch_dot(E, s, a, f); break;
      case Kind::RowDot: rc = launch_rowdot(E, s, a, f); break;
      case Kind::StreamKvec: rc = launch_stream_kvec(E, s, a); break;
      case Kind::Stream: rc = launch_stream(E, s, a, f, gc); break;
    }
  }
  if (rc != CTN_OK) return rc;
  if (col.on)
    hipLaunchKernelGGL(k_collapse, dim3(E->R), dim3(256), 0, E->stream, (const double*)E->d_scratch, col.blocks, part_region(E, s));
  launch_renorm(E, s);
  return t.end();
}

// What a closing run adds to its finish (ctn_exec_enqueue_closed, a closing RUN record of a backward tape): the register
// block and the indices k_tape_regs takes.
struct RunClose { double* regs; int r_log, r_dst, k0, k1; };

// An executor may close its run - k_run_close in place of k_scales, k_finalize and the register launches - only when the
// launch has one step's partials to read, one replica's result to divide, and does divide it.
static bool exec_may_close(const Exec* E) { return E->plan->n_steps == 1 && E->R == 1 && !E->defer_finish; }

// the scales of every step, then the final division; `close`: both and the run's register work as one launch
static int launch_finish(Exec* E, const RunClose* close = nullptr) {
  const Plan& P = *E->plan;
  const int R = E->R;
  FinalArgs f;
  f.ptrs = E->d_ptrs; f.partials = E->d_partials; f.stepOff = E->d_stepOff; f.stepSlots = E->d_stepSlots;
  f.stepP = E->d_stepP; f.stepNumel = E->d_stepNumel; f.log_scale = E->d_log; f.rescales = E->d_resc;
  f.min_norm = P.min_norm; f.out_numel = P.output().numel;
  f.n_steps = P.n_steps; f.R = R; f.id_out = P.n_inputs + P.n_steps - 1; f.n_tensors = E->n_tensors;
  f.stabilize = P.stabilize ? 1 : 0;
  f.defer = E->defer_finish ? 1 : 0;
  f.vec = E->outs_aligned16 ? 1 : 0;
  int fb = (int)std::min<int64_t>((P.output().numel / (f.vec ? (P.dtype == CTN_F64 ? 2 : 4) : 1) + 255) / 256, 4096);
  if (fb < 1) fb = 1;
  const dim3 sg((P.n_steps + 3) / 4, R);
  if (close) {
    if (!exec_may_close(E)) { g_err = "this executor may not close its run (one step, one replica, no deferred finish)"; return CTN_UNSUPPORTED; }
    if (P.dtype == CTN_F32)
      hipLaunchKernelGGL(k_run_close<float>, dim3(fb, 1), dim3(256), 0, E->stream, f, E->d_logs, close->regs, close->r_log,
                         close->r_dst, close->k0, close->k1);
    else
      hipLaunchKernelGGL(k_run_close<double>, dim3(fb, 1), dim3(256), 0, E->stream, f, E->d_logs, close->regs, close->r_log,
                         close->r_dst, close->k0, close->k1);
  } else if (P.dtype == CTN_F32) {
    hipLaunchKernelGGL(k_scales<float>, sg, dim3(256), 0, E->stream, f, E->d_logs);
    hipLaunchKernelGGL(k_finalize<float>, dim3(fb, R), dim3(256), 0, E->stream, f, (const double*)E->d_logs);
  } else {
    hipLaunchKernelGGL(k_scales<double>, sg, dim3(256), 0, E->stream, f, E->d_logs);
    hipLaunchKernelGGL(k_finalize<double>, dim3(fb, R), dim3(256), 0, E->stream, f, (const double*)E->d_logs);
  }
  HIPCHECK(hipGetLastError());
  return CTN_OK;
}

static int exec_launch_steps(Exec* E, const RunClose* close = nullptr) {
  const Plan& P = *E->plan;
  int rc = CTN_OK;
  // the report is of THIS enqueue: a step that reports nothing now (a streaming step, a member that stepped aside for the
  // eager mode) must not keep the mark of an earlier one
  std::fill(E->launched_tile.begin(), E->launched_tile.end(), 0);
  std::fill(E->launched_form.begin(), E->launched_form.end(), 0);
  E->report_is_graphs = false;
  if (P.chain && E->d_chain != nullptr) {
    rc = launch_chain(E);
  } else {
    int group_skip = 0;
    GroupCollect gc;
    for (int s = 0; s < P.n_steps && rc == CTN_OK; ++s) {
      if (group_skip > 0) { --group_skip; continue; }   // went out with the head of its group
      if (gc.left == 0 && E->forms.groups[s].len >= 2 && E->sw.group && !E->eager_rescale &&
          !(E->timing_runs < E->timing_slots)) {
        const LeafGroup& G = E->forms.groups[s];
        if (G.ready) {
          launch_group(E, G);
          group_skip = G.len - 1;
          continue;
        }
        gc.left = G.len; gc.head = s;   // first time: the steps' arguments are built by launch_stream, not launched
      }
      if (E->forms.sweep_role[s] && !E->eager_rescale) { rc = launch_sweep_member(E, s); continue; }
      switch (E->forms.role[s]) {
        case Role::ZipLat: rc = launch_zip_lat(E, s); break;
        case Role::Zip: rc = launch_zip(E, s); break;
        case Role::Absorbed: rc = mark_absorbed(E, s); break;   // first step of a zipper pair, S step of a complex pair
        case Role::Cplx: case Role::Plain:                      // (launch_step reads the role again)
          if (P.steps[s].kernel == CTN_KERNEL_FUSED) rc = time_nothing(E, s);   // formed on the fly inside its consumer
          else rc = launch_step(E, s, &gc);
          break;
      }
    }
  }
  if (rc != CTN_OK) return rc;
  rc = launch_finish(E, close);
  if (rc != CTN_OK) return rc;
  if (E->timing_runs < E->timing_slots) E->timing_runs++;
  return CTN_OK;
}

// One enqueue of the whole path.  A path is hundreds of launches whose arguments never change (operands are
// reached through the device pointer table), and with one small or mid-size network in flight the host's
// launch rate, not the device, bounds the walk (100-site MPS, D = 32 ... 256: 1.3 - 2.3 ms of enqueue for
// 1.6 - 2.6 ms of wall time): from the third enqueue on the sequence is replayed as ONE hipGraph launch.
// Event-timed enqueues, the single-launch chain walk, debug stamping and streams that are themselves being
// captured stay eager.  CTN_GRAPH=0 disables.
static int exec_launch_all(Exec* E, const RunClose* close = nullptr) {
  const Plan& P = *E->plan;
  if (close) return exec_launch_steps(E, close);   // a closing run has one step: never a graph of its own
  const bool timed = E->timing_runs < E->timing_slots;
  const bool chain = P.chain && E->d_chain != nullptr;
  if (!E->use_graph || timed || chain || P.n_steps < 4 || E->eager_rescale || E->sw.stamps) return exec_launch_steps(E);
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(E->stream, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) {
    (void)hipGetLastError();
    return exec_launch_steps(E);
  }
  if (E->graph_exec && E->graph_aligned != E->outs_aligned16) {   // vector width of the last step changed
    (void)hipGraphExecDestroy(E->graph_exec);
    E->graph_exec = nullptr;
  }
  if (!E->graph_exec) {
    if (!E->graph_warm) { E->graph_warm = true; return exec_launch_steps(E); }
    hipGraph_t g = nullptr;
    if (hipStreamBeginCapture(E->stream, hipStreamCaptureModeThreadLocal) != hipSuccess) {
      (void)hipGetLastError();
      E->use_graph = 0;
      return exec_launch_steps(E);
    }
    const int rc = exec_launch_steps(E);
    const hipError_t ec = hipStreamEndCapture(E->stream, &g);
    if (rc != CTN_OK || ec != hipSuccess || !g ||
        hipGraphInstantiate(&E->graph_exec, g, nullptr, nullptr, 0) != hipSuccess) {
      (void)hipGetLastError();
      if (g) (void)hipGraphDestroy(g);
      E->graph_exec = nullptr;
      E->use_graph = 0;                      // fall back to eager launches for good
      return rc != CTN_OK ? rc : exec_launch_steps(E);
    }
    (void)hipGraphDestroy(g);
    E->graph_aligned = E->outs_aligned16;
    E->graph_form = E->launched_form; E->graph_tile = E->launched_tile;
    E->report_is_graphs = true;
  }
  if (!E->report_is_graphs) {                  // an eager repeat (exec_fetch_checked) reported its own launches in between
    E->launched_form = E->graph_form; E->launched_tile = E->graph_tile;
    E->report_is_graphs = true;
  }
  HIPCHECK(hipGraphLaunch(E->graph_exec, E->stream));
  return CTN_OK;
}

static int exec_set_pointers(Exec* E, const void* const* dev_inputs, void* const* dev_outs) {
  const Plan& P = *E->plan;
  const int nt = E->n_tensors;
  bool changed = !E->ptrs_valid;
  for (int r = 0; r < E->R; ++r) {
    void** row = E->h_ptrs.data() + (size_t)r * nt;
    for (int i = 0; i < P.n_inputs; ++i) {
      void* p = const_cast<void*>(dev_inputs[(size_t)r * P.n_inputs + i]);
      if (!p) { g_err = "null operand pointer"; return CTN_INVALID_ARG; }
      if ((uintptr_t)p % 16) { g_err = "operand pointers must be 16-byte aligned"; return CTN_INVALID_ARG; }
      if (row[i] != p) { row[i] = p; changed = true; }
    }
    void* o = dev_outs[r];
    if (!o) { g_err = "null output pointer"; return CTN_INVALID_ARG; }
    if ((uintptr_t)o % P.elem_size()) { g_err = "output pointers must be element aligned"; return CTN_INVALID_ARG; }
    if (r == 0) E->outs_aligned16 = true;
    if ((uintptr_t)o % 16) E->outs_aligned16 = false;
    const int id_out = P.n_inputs + P.n_steps - 1;
    if (row[id_out] != o) { row[id_out] = o; changed = true; }
  }
  if (changed) {
    HIPCHECK(hipMemcpyAsync(E->d_ptrs, E->h_ptrs.data(), E->h_ptrs.size() * sizeof(void*),
                            hipMemcpyHostToDevice, E->stream));
    E->ptrs_valid = true;
  }
  return CTN_OK;
}

// A new set of operands starts in the caller's mode: an executor that switched itself to eager rescaling for one
// extreme input (exec_fetch_checked) tries the lazy form - hipGraph replay, grouped leaf steps, no k_renorm passes -
// again on the next one, and after kEagerSticky such switches in a row it stays eager (a caller who keeps sending
// extreme operands should not pay two contractions each time).
constexpr int kEagerSticky = 3;
static void exec_new_run(Exec* E) {
  if (E->eager_forced) { E->eager_rescale = true; return; }
  if (E->eager_rescale && E->eager_streak < kEagerSticky) E->eager_rescale = false;
}

}  // namespace ctn

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
using namespace ctn;

struct ctn_plan { Plan p; };
struct ctn_exec { Exec e; };

extern "C" {

int ctn_version(void) { return CTN_ABI_VERSION; }

const char* ctn_last_error(void) { return g_err.c_str(); }

int ctn_device_count(int* count) {
  if (!count) { g_err = "count is NULL"; return CTN_INVALID_ARG; }
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) {
    *count = 0;
    g_err = std::string("no HIP device available: ") + hipGetErrorString(e);
    (void)hipGetLastError();
    return CTN_NO_DEVICE;
  }
  *count = n;
  return CTN_OK;
}

int ctn_plan_create(const ctn_plan_desc* desc, ctn_plan** out) {
  if (!desc || !out) { g_err = "NULL argument"; return CTN_INVALID_ARG; }
  *out = nullptr;
  ctn_plan* p = new (std::nothrow) ctn_plan();
  if (!p) { g_err = "out of host memory"; return CTN_OOM; }
  std::string err;
  int rc = CTN_OK;
  try {
    rc = build_plan(*desc, p->p, err);
  } catch (const std::bad_alloc&) {
    rc = CTN_OOM; err = "out of host memory while building the plan";
  } catch (const std::exception& ex) {
    rc = CTN_INVALID_ARG; err = ex.what();
  }
  if (rc != CTN_OK) { g_err = err; delete p; return rc; }
  *out = p;
  return CTN_OK;
}

void ctn_plan_destroy(ctn_plan* plan) { delete plan; }
int ctn_plan_dtype(const ctn_plan* plan) { return plan ? plan->p.dtype : CTN_INVALID_ARG; }
int ctn_plan_n_inputs(const ctn_plan* plan) { return plan ? plan->p.n_inputs : CTN_INVALID_ARG; }
int ctn_plan_n_steps(const ctn_plan* plan) { return plan ? plan->p.n_steps : CTN_INVALID_ARG; }
double ctn_plan_flops(const ctn_plan* plan) { return plan ? plan->p.flops : 0.0; }
int64_t ctn_plan_bytes_min(const ctn_plan* plan) { return plan ? plan->p.bytes_min : 0; }
int ctn_plan_out_ndim(const ctn_plan* plan) { return plan ? (int)plan->p.output().dims.size() : CTN_INVALID_ARG; }
int ctn_plan_out_dims(const ctn_plan* plan, int64_t* dims) {
  if (!plan || !dims) { g_err = "NULL argument"; return CTN_INVALID_ARG; }
  const auto& d = plan->p.output().dims;
  for (size_t i = 0; i < d.size(); ++i) dims[i] = d[i];
  return CTN_OK;
}
int ctn_plan_out_labels(const ctn_plan* plan, int32_t* labels) {
  if (!plan || !labels) { g_err = "NULL argument"; return CTN_INVALID_ARG; }
  const auto& l = plan->p.output().labels;
  for (size_t i = 0; i < l.size(); ++i) labels[i] = l[i];
  return CTN_OK;
}
int64_t ctn_plan_out_numel(const ctn_plan* plan) { return plan ? plan->p.output().numel : 0; }
int64_t ctn_plan_out_bytes(const ctn_plan* plan) {
  return plan ? plan->p.output().numel * (int64_t)plan->p.elem_size() : 0;
}

static int64_t exec_fixed_bytes(const Plan& P, int R) {
  const int nt = P.n_inputs + P.n_steps + 1;
  int64_t slots = 0;
  for (const Step& st : P.steps) slots += std::max(std::max(st.partials, st.partials_step), kWaveOutputs);   // (a launcher may retile: upper bound)
  return (int64_t)P.tables.size() * 4 + (int64_t)P.tables64.size() * 8 + (int64_t)R * nt * 8 + slots * R * 8 +
         (int64_t)R * std::max<int64_t>(P.max_collapse_blocks, 1) * 8 + (int64_t)R * 8 +
         (int64_t)R * P.n_steps * 8 + 256 + (int64_t)P.n_steps * 12;
}

int64_t ctn_plan_workspace_bytes(const ctn_plan* plan, int replicas) {
  if (!plan || replicas < 1) return 0;
  return plan->p.ws_bytes_per_replica * replicas + exec_fixed_bytes(plan->p, replicas);
}

int ctn_plan_step_info(const ctn_plan* plan, int step, ctn_step_info* info) {
  if (!plan || !info || step < 0 || step >= plan->p.n_steps) { g_err = "invalid step query"; return CTN_INVALID_ARG; }
  const Step& s = plan->p.steps[step];
  info->kernel = s.kernel;
  info->swapped = s.swapped ? 1 : 0;
  info->batch = s.Bt; info->m = s.M; info->n = s.N; info->k = s.K;
  info->mode_a = s.modeA; info->mode_b = s.modeB;
  info->partials = s.partials; info->blocks = s.blocks;
  info->flops = s.flops;
  info->out_numel = plan->p.tensors[s.out].numel;
  info->tile_m = s.kernel == CTN_KERNEL_MFMA_F32 ? s.tileM : (s.kernel == CTN_KERNEL_MFMA_F64 ? kTile64M : 0);
  info->tile_n = (s.kernel == CTN_KERNEL_MFMA_F32 || s.kernel == CTN_KERNEL_MFMA_F64) ? s.tileN : 0;
  info->epilogue_sum = s.epw;
  info->reserved = 0;
  return CTN_OK;
}

int ctn_exec_create(const ctn_plan* plan, int device, void* stream, int replicas, ctn_exec** out) {
  if (!plan || !out || replicas < 1) { g_err = "invalid argument to ctn_exec_create"; return CTN_INVALID_ARG; }
  *out = nullptr;
  int ndev = 0;
  int rc = ctn_device_count(&ndev);
  if (rc != CTN_OK) return rc;
  if (device < 0 || device >= ndev) { g_err = "device index out of range"; return CTN_INVALID_ARG; }
  DeviceGuard dg(device);
  HIPCHECK(dg.err);
  int n_cu = 256;
  (void)hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device);
  ctn_exec* x = new (std::nothrow) ctn_exec();
  if (!x) { g_err = "out of host memory"; return CTN_OOM; }
  Exec& E = x->e;
  E.sw = read_dev_switches();
  // (a small-bond sweep that is asked for takes a chain plan from the chain walker: the executor works on its own copy)
  if (sweep_small_unchains(plan->p, replicas, n_cu > 0 ? n_cu : 256, E.sw)) E.own_plan = unchained(plan->p);
  const Plan& P = E.own_plan.n_steps ? E.own_plan : plan->p;
  E.plan = &P; E.device = device; E.R = replicas; E.n_cu = n_cu > 0 ? n_cu : 256;
  E.use_graph = E.sw.graph;
  E.launched_tile.assign(P.n_steps, 0);
  E.launched_form.assign(P.n_steps, 0);
  E.n_tensors = P.n_inputs + P.n_steps + 1;
  // every decision first (host code, fused_forms.h); what follows allocates and uploads what the record asks for
  E.forms = fused_forms(P, replicas, E.n_cu, E.sw);
  const FusedForms& F = E.forms;
  auto fail = [&](int code) { delete x; return code; };
  // `bytes` of device memory (none: the pointer stays null) ... filled with a host vector
  auto dev_alloc = [](auto** d, size_t bytes) { return bytes ? hipMalloc((void**)d, bytes) : hipSuccess; };
  auto dev_upload = [&](auto** d, const auto& h) {
    const size_t bytes = h.size() * sizeof(h[0]);
    const hipError_t e = dev_alloc(d, bytes);
    return e != hipSuccess || !bytes ? e : hipMemcpy(*d, h.data(), bytes, hipMemcpyHostToDevice);
  };
#define HIPCHECK_X(expr)                                                        \
  do {                                                                          \
    hipError_t e_ = (expr);                                                     \
    if (e_ != hipSuccess) {                                                     \
      g_err = std::string(#expr) + ": " + hipGetErrorString(e_);                \
      return fail(e_ == hipErrorOutOfMemory ? CTN_OOM : CTN_HIP_ERROR);         \
    }                                                                           \
  } while (0)
  if (stream) { E.stream = (hipStream_t)stream; }
  else { HIPCHECK_X(hipStreamCreateWithFlags(&E.stream, hipStreamNonBlocking)); E.own_stream = true; }
  const size_t ws = (size_t)std::max<int64_t>(P.ws_bytes_per_replica, 256) * replicas;
  HIPCHECK_X(hipMalloc((void**)&E.d_ws, ws));
  HIPCHECK_X(hipMalloc((void**)&E.d_tables, std::max<size_t>(P.tables.size(), 4) * 4));
  HIPCHECK_X(hipMemcpy(E.d_tables, P.tables.data(), P.tables.size() * 4, hipMemcpyHostToDevice));
  HIPCHECK_X(hipMalloc((void**)&E.d_tables64, std::max<size_t>(P.tables64.size(), 2) * 8));
  HIPCHECK_X(hipMemcpy(E.d_tables64, P.tables64.data(), P.tables64.size() * 8, hipMemcpyHostToDevice));
  HIPCHECK_X(hipMalloc((void**)&E.d_ptrs, (size_t)replicas * E.n_tensors * sizeof(void*)));
  HIPCHECK_X(dev_alloc(&E.d_slab, F.slab_elems * P.elem_size()));
  HIPCHECK_X(dev_alloc(&E.d_slab2, F.fold_elems * P.elem_size()));
  for (int i = 0; i < 2; ++i) HIPCHECK_X(dev_alloc(&E.d_zl_slab[i], (size_t)F.zl_slab_elems * P.elem_size()));
  HIPCHECK_X(dev_upload(&E.d_cplx_tabs, F.cplx_tabs));
  HIPCHECK_X(dev_upload(&E.d_sweep_ids, F.sweep_ids));
  HIPCHECK_X(dev_upload(&E.d_sweep_off, F.sweep_offs));
  HIPCHECK_X(dev_upload(&E.d_sweep_slots, F.sweep_slots));
  HIPCHECK_X(dev_alloc(&E.d_sweep_a, F.sweep_a * 8));
  HIPCHECK_X(dev_alloc(&E.d_sweep_s, F.sweep_s * 4));
  HIPCHECK_X(dev_alloc(&E.d_sweep_e, F.sweep_e * 4));
  HIPCHECK_X(dev_alloc(&E.d_sweep_z, F.sweep_z * 8));
  HIPCHECK_X(dev_alloc(&E.d_sweep_la, F.sweep_l * 8));
  HIPCHECK_X(dev_alloc(&E.d_sweep_ls, F.sweep_l * 8));
  if (F.group_args) HIPCHECK_X(hipHostMalloc((void**)&E.h_group_args, sizeof(StepArgs) * (size_t)F.group_args, hipHostMallocDefault));
  HIPCHECK_X(dev_alloc(&E.d_group_args, sizeof(StepArgs) * (size_t)F.group_args));
  HIPCHECK_X(hipMalloc((void**)&E.d_scratch, (size_t)replicas * F.scratch_need * 8));
  HIPCHECK_X(hipMalloc((void**)&E.d_partials, (size_t)F.part_slots * replicas * 8));
  HIPCHECK_X(hipMemset(E.d_partials, 0, (size_t)F.part_slots * replicas * 8));
  HIPCHECK_X(dev_upload(&E.d_stepOff, F.step_off));
  HIPCHECK_X(dev_upload(&E.d_stepSlots, F.step_partials));
  HIPCHECK_X(hipMalloc((void**)&E.d_log, (size_t)replicas * 8));
  HIPCHECK_X(hipMalloc((void**)&E.d_resc, (size_t)replicas * P.n_steps * 8));
  HIPCHECK_X(hipMalloc((void**)&E.d_logs, (size_t)replicas * P.n_steps * 8));
  HIPCHECK_X(hipMalloc(&E.d_ones, 256));
  {
    double one64 = 1.0; float one32 = 1.0f;
    if (P.dtype == CTN_F64) HIPCHECK_X(hipMemcpy(E.d_ones, &one64, 8, hipMemcpyHostToDevice));
    else HIPCHECK_X(hipMemcpy(E.d_ones, &one32, 4, hipMemcpyHostToDevice));
  }
  std::vector<int32_t> sp(P.n_steps);
  std::vector<double> sn(P.n_steps);
  for (int s = 0; s < P.n_steps; ++s) {
    sp[s] = P.steps[s].kernel == CTN_KERNEL_FUSED ? 0 : F.step_partials[s];   // no partials: rescale reported as 0.0
    sn[s] = (double)P.tensors[P.steps[s].out].numel;
  }
  HIPCHECK_X(dev_upload(&E.d_stepP, sp));
  HIPCHECK_X(dev_upload(&E.d_stepNumel, sn));
  if (P.chain) {
    std::vector<ChainStep> cs(P.n_steps);
    for (int s = 0; s < P.n_steps; ++s) {
      const Step& st = P.steps[s];
      ChainStep& c = cs[s];
      const int32_t* T = E.d_tables;
      const int64_t* T8 = E.d_tables64;
      c.obA = T8 + st.t.obA; c.obB = T8 + st.t.obB; c.obC = T8 + st.t.obC;
      c.omA = T + st.t.omA; c.omC = T + st.t.omC; c.onB = T + st.t.onB; c.onC = T + st.t.onC;
      c.okA = T + st.t.okA; c.okB = T + st.t.okB;
      c.numelC = (double)P.tensors[st.out].numel;
      c.Bt = (int32_t)st.Bt; c.M = (int32_t)st.M; c.N = (int32_t)st.N; c.K = (int32_t)st.K;
      c.idA = st.lhs; c.idB = st.rhs >= 0 ? st.rhs : E.n_tensors - 1; c.idC = st.out;
      c.prodA = st.lhs >= P.n_inputs ? P.tensors[st.lhs].producer : -1;
      c.prodB = st.rhs >= P.n_inputs ? P.tensors[st.rhs].producer : -1;
    }
    HIPCHECK_X(dev_upload(&E.d_chain, cs));
    // the on-chip walker, where asked for and where the packer takes the plan (a refusal keeps k_chain)
    if (E.sw.chain == 2 || (kChainLdsDefault && E.sw.chain != 1)) {
      ChainProgram cp;
      std::string why;
      if (chain_pack(P, &cp, &why)) {
        HIPCHECK_X(dev_upload(&E.d_chain_prog, cp.words));
        E.chain_len0 = cp.steps[0].len;
      }
    }
  }
  HIPCHECK_X(dev_alloc(&E.d_zqp_side, (size_t)F.zqp_side_bytes * F.zqp_side_bufs * replicas));
  // pointer table: intermediates and the ones-scalar are fixed for the executor's lifetime
  E.h_ptrs.assign((size_t)replicas * E.n_tensors, nullptr);
  for (int r = 0; r < replicas; ++r) {
    void** row = E.h_ptrs.data() + (size_t)r * E.n_tensors;
    for (int id = P.n_inputs; id < P.n_inputs + P.n_steps - 1; ++id)
      row[id] = F.zqp_side[id] < 0 ? E.d_ws + (size_t)r * P.ws_bytes_per_replica + P.tensors[id].ws_offset
                                   : E.d_zqp_side + ((size_t)F.zqp_side[id] * replicas + r) * F.zqp_side_bytes;
    row[E.n_tensors - 1] = E.d_ones;
  }
#undef HIPCHECK_X
  *out = x;
  return CTN_OK;
}

void ctn_exec_destroy(ctn_exec* exec) { delete exec; }

int ctn_exec_enqueue(ctn_exec* exec, const void* const* dev_inputs, void* const* dev_outs) {
  if (!exec || !dev_inputs || !dev_outs) { g_err = "NULL argument"; return CTN_INVALID_ARG; }
  Exec* E = &exec->e;
  DeviceGuard dg(E->device);
  HIPCHECK(dg.err);
  int rc = exec_set_pointers(E, dev_inputs, dev_outs);
  if (rc != CTN_OK) return rc;
  exec_new_run(E);
  return exec_launch_all(E);
}

int ctn_exec_enqueue_closed(ctn_exec* exec, const void* const* dev_inputs, void* const* dev_outs, double* regs, int r_log,
                            int r_dst, int k0, int k1) {
  if (!exec || !dev_inputs || !dev_outs || !regs || r_log < 0 || r_dst < 0) { g_err = "invalid argument to ctn_exec_enqueue_closed"; return CTN_INVALID_ARG; }
  Exec* E = &exec->e;
  if (!exec_may_close(E)) {                        // before anything is touched: the caller issues the plain calls instead
    g_err = "ctn_exec_enqueue_closed: the executor needs a one-step plan, one replica and no deferred finish";
    return CTN_UNSUPPORTED;
  }
  DeviceGuard dg(E->device);
  HIPCHECK(dg.err);
  int rc = exec_set_pointers(E, dev_inputs, dev_outs);
  if (rc != CTN_OK) return rc;
  exec_new_run(E);
  const RunClose close{regs, r_log, r_dst, k0, k1};
  return exec_launch_all(E, &close);
}

int ctn_exec_synchronize(ctn_exec* exec) {
  if (!exec) { g_err = "NULL argument"; return CTN_INVALID_ARG; }
  HIPCHECK(hipStreamSynchronize(exec->e.stream));
  if (const char* path = exec->e.sw.stamps) {  // development only: dump the last MFMA launch's stamps
    Exec* E = &exec->e;
    if (E->d_dbg && E->dbg_tiles) {
      std::vector<unsigned long long> h(E->dbg_tiles * 8);
      HIPCHECK(hipMemcpy(h.data(), E->d_dbg, h.size() * 8, hipMemcpyDeviceToHost));
      if (FILE* f = fopen(path, "wb")) { fwrite(h.data(), 8, h.size(), f); fclose(f); }
    }
  }
  return CTN_OK;
}

// Did a lazy epilogue rescale leave the dtype's range in the run whose scale registers are in E->h_resc?
// A tile kernel accumulates on the STORED operands, A_hat sA and B_hat sB, and multiplies by 1 / (sA sB)
// afterwards, where the reference normalises each intermediate before the next product (einsum.py:387): the
// accumulators therefore carry about s_out sA sB, which can overflow (or sink into the subnormals) although
// every normalised quantity is fine - operands of magnitude ~1e13 do it in fp32.  All three factors are in the
// scale registers the run has just produced, so the test costs nothing on the device: non-finite anywhere, an
// accumulator magnitude beyond 2^+-100 (fp32; 2^+-900 fp64), or an all-zero output behind operand scales that
// could have flushed it.
static bool exec_scales_suspect(const Exec* E, const double* resc = nullptr, int replicas = -1) {
  const Plan& P = *E->plan;
  if (!P.stabilize || (P.chain && E->d_chain)) return false;   // the chain walker divides operands on load
  const double hi = std::ldexp(1.0, P.dtype == CTN_F64 ? 900 : 100), lo = 1.0 / hi;
  const double zhi = std::ldexp(1.0, P.dtype == CTN_F64 ? 500 : 60), zlo = 1.0 / zhi;
  if (!resc) resc = E->h_resc.data();
  if (replicas < 0) replicas = E->R;
  for (int r = 0; r < replicas; ++r) {
    const double* rs = resc + (size_t)r * P.n_steps;
    for (int s = 0; s < P.n_steps; ++s) {
      const Step& st = P.steps[s];
      auto scale_of = [&](int id) {
        if (id < P.n_inputs) return 1.0;
        const double v = rs[P.tensors[id].producer];
        return v == 0.0 ? 1.0 : v;
      };
      if (st.kernel == CTN_KERNEL_FUSED) continue;
      const Role role = E->forms.role[s];
      if (role == Role::Absorbed) continue;                          // runs inside a later step's launch
      // A sweep rescales inside its launch, so its members' factors say nothing about its accumulators - and those are NOT
      // in range by themselves: the state stays un-rescaled and a block's scale goes into the next site's weights, so W_s .
      // state carries one core more than any product of the reference.  The sweep raises its own alarm:
      // a block whose state left the range records a non-finite abs-sum, and the bookkeeping (k_sweep_z / k_sweep64_z,
      // k_sweep_finish / k_sweep64_finish) turns that into a non-finite factor of the step.
      if (E->forms.sweep_role[s] && !E->eager_rescale) {
        if (!std::isfinite(rs[s])) return true;
        continue;
      }
      double sab = scale_of(st.lhs) * (st.rhs >= 0 ? scale_of(st.rhs) : 1.0) * (st.lhs2 >= 0 ? scale_of(st.lhs2) : 1.0);
      if (role == Role::Zip || role == Role::ZipLat)                 // the fused pair accumulates on E, X and Y as stored
        sab = scale_of(P.steps[s - 1].lhs) * scale_of(P.steps[s - 1].rhs) * scale_of(st.rhs);
      if (role == Role::Cplx)                                        // the complex pair accumulates on `small` and `big` as stored
        sab = scale_of(E->forms.cplx[s].small) * scale_of(E->forms.cplx[s].big);
      const double so = rs[s];
      if (!std::isfinite(so) || !std::isfinite(sab)) return true;
      if (so == 0.0) { if (sab > zhi || sab < zlo) return true; continue; }
      const double acc = so * sab;
      if (!(acc < hi) || !(acc > lo)) return true;
    }
  }
  return false;
}

// Wait for the stream, read the scale registers, and - in the default lazy mode - repeat the contraction in
// eager mode when they show that a lazy product left the dtype's range.  The operands are still in place: they
// are borrowed until the fetch.
static int exec_fetch_checked(Exec* E, double* log_scale) {
  const Plan& P = *E->plan;
  E->h_resc.resize((size_t)E->R * P.n_steps);
  for (int attempt = 0; attempt < 2; ++attempt) {
    if (log_scale)
      HIPCHECK(hipMemcpyAsync(log_scale, E->d_log, (size_t)E->R * 8, hipMemcpyDeviceToHost, E->stream));
    HIPCHECK(hipMemcpyAsync(E->h_resc.data(), E->d_resc, E->h_resc.size() * 8, hipMemcpyDeviceToHost, E->stream));
    HIPCHECK(hipStreamSynchronize(E->stream));
    if (E->eager_rescale || !E->ptrs_valid) break;
    if (!exec_scales_suspect(E)) { E->eager_streak = 0; break; }
    E->eager_rescale = true;
    E->eager_reruns++;
    E->eager_streak++;
    const int rc = exec_launch_all(E);
    if (rc != CTN_OK) return rc;
  }
  return CTN_OK;
}

int ctn_exec_fetch(ctn_exec* exec, double* log_scale, double* step_rescales) {
  if (!exec) { g_err = "NULL argument"; return CTN_INVALID_ARG; }
  Exec* E = &exec->e;
  DeviceGuard dg(E->device);
  HIPCHECK(dg.err);
  const int rc = exec_fetch_checked(E, log_scale);
  if (rc != CTN_OK) return rc;
  if (step_rescales) memcpy(step_rescales, E->h_resc.data(), E->h_resc.size() * 8);
  return CTN_OK;
}

int ctn_exec_set_rescale_mode(ctn_exec* exec, int mode) {
  if (!exec || mode < 0 || mode > 1) { g_err = "rescale mode must be 0 (lazy, eager on demand) or 1 (eager)"; return CTN_INVALID_ARG; }
  Exec* E = &exec->e;
  const int prev = E->eager_rescale ? 1 : 0;
  E->eager_forced = mode == 1;
  E->eager_rescale = mode == 1;
  return prev;
}

int ctn_exec_eager_reruns(const ctn_exec* exec) { return exec ? exec->e.eager_reruns : CTN_INVALID_ARG; }

int ctn_exec_set_finish_mode(ctn_exec* exec, int mode) {
  if (!exec || mode < 0 || mode > 1) { g_err = "finish mode must be 0 (normalise at the end of every run) or 1 (deferred to ctn_exec_finish)"; return CTN_INVALID_ARG; }
  Exec* E = &exec->e;
  const int prev = E->defer_finish ? 1 : 0;
  if (prev != mode && E->graph_exec) {             // the captured k_finalize carries the old mode
    DeviceGuard dg(E->device);
    HIPCHECK(dg.err);
    HIPCHECK(hipStreamSynchronize(E->stream));
    (void)hipGraphExecDestroy(E->graph_exec);
    E->graph_exec = nullptr;
  }
  E->defer_finish = mode == 1;
  return prev;
}

int ctn_exec_finish(ctn_exec* exec, const double* mult) {
  if (!exec || !mult) { g_err = "NULL argument"; return CTN_INVALID_ARG; }
  Exec* E = &exec->e;
  const Plan& P = *E->plan;
  if (!E->defer_finish || !E->ptrs_valid) { g_err = "ctn_exec_finish: no deferred run to finish (ctn_exec_set_finish_mode(1), then enqueue)"; return CTN_INVALID_ARG; }
  DeviceGuard dg(E->device);
  HIPCHECK(dg.err);
  if (!E->d_mult) HIPCHECK(hipMalloc((void**)&E->d_mult, (size_t)E->R * 8));
  HIPCHECK(hipMemcpyAsync(E->d_mult, mult, (size_t)E->R * 8, hipMemcpyHostToDevice, E->stream));
  const int vec = E->outs_aligned16 ? 1 : 0;
  const int64_t numel = P.output().numel;
  const int V = vec ? (P.dtype == CTN_F64 ? 2 : 4) : 1;
  const dim3 g((unsigned)std::max<int64_t>(1, std::min<int64_t>((numel / V + 255) / 256, 4096)), (unsigned)E->R);
  const int id_out = P.n_inputs + P.n_steps - 1;
  if (P.dtype == CTN_F32)
    hipLaunchKernelGGL(k_finish<float>, g, dim3(256), 0, E->stream, (void* const*)E->d_ptrs, E->n_tensors, id_out, numel,
                       (const double*)E->d_resc, P.n_steps, P.stabilize ? 1 : 0, (const double*)E->d_mult, vec);
  else
    hipLaunchKernelGGL(k_finish<double>, g, dim3(256), 0, E->stream, (void* const*)E->d_ptrs, E->n_tensors, id_out, numel,
                       (const double*)E->d_resc, P.n_steps, P.stabilize ? 1 : 0, (const double*)E->d_mult, vec);
  HIPCHECK(hipGetLastError());
  return CTN_OK;
}

int ctn_exec_run(ctn_exec* exec, const void* const* inputs, int inputs_space, void* const* outs,
                 int outs_space, double* log_scale, double* step_rescales) {
  if (!exec || !inputs || !outs) { g_err = "NULL argument"; return CTN_INVALID_ARG; }
  Exec* E = &exec->e;
  const Plan& P = *E->plan;
  DeviceGuard dg(E->device);
  HIPCHECK(dg.err);
  const size_t es = P.elem_size();
  const int64_t out_bytes = P.output().numel * (int64_t)es;
  const int64_t out_slot = (out_bytes + kAlign - 1) / kAlign * kAlign;
  std::vector<const void*> din((size_t)E->R * P.n_inputs);
  std::vector<void*> dout(E->R);
  if (inputs_space == CTN_MEM_HOST) {
    if (!E->d_stage_in) {
      hipError_t e_ = hipMalloc((void**)&E->d_stage_in, (size_t)std::max<int64_t>(P.input_bytes_per_replica, 256) * E->R);
      if (e_ != hipSuccess) { g_err = "hipMalloc(input staging) failed"; return e_ == hipErrorOutOfMemory ? CTN_OOM : CTN_HIP_ERROR; }
    }
    // many small operands: pack them on the host and issue ONE copy (1001 tiny copies cost ms)
    const size_t total_in = (size_t)P.input_bytes_per_replica * E->R;
    const bool packed = total_in <= (8u << 20) && (size_t)P.n_inputs * E->R > 8;
    if (packed && E->h_pack_bytes < total_in) {
      if (E->h_pack) (void)hipHostFree(E->h_pack);
      E->h_pack = nullptr; E->h_pack_bytes = 0;
      if (hipHostMalloc((void**)&E->h_pack, total_in, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); }
      else E->h_pack_bytes = total_in;
    }
    const bool use_pack = packed && E->h_pack;
    if (use_pack) HIPCHECK(hipStreamSynchronize(E->stream));  // previous copy out of h_pack has finished
    for (int r = 0; r < E->R; ++r)
      for (int i = 0; i < P.n_inputs; ++i) {
        const void* src = inputs[(size_t)r * P.n_inputs + i];
        if (!src) { g_err = "null operand pointer"; return CTN_INVALID_ARG; }
        const size_t off = (size_t)r * P.input_bytes_per_replica + P.input_offsets[i];
        char* dst = E->d_stage_in + off;
        if (use_pack) memcpy(E->h_pack + off, src, (size_t)P.tensors[i].numel * es);
        else HIPCHECK(hipMemcpyAsync(dst, src, (size_t)P.tensors[i].numel * es, hipMemcpyHostToDevice, E->stream));
        din[(size_t)r * P.n_inputs + i] = dst;
      }
    if (use_pack) HIPCHECK(hipMemcpyAsync(E->d_stage_in, E->h_pack, total_in, hipMemcpyHostToDevice, E->stream));
  } else {
    for (size_t i = 0; i < din.size(); ++i) din[i] = inputs[i];
  }
  if (outs_space == CTN_MEM_HOST) {
    if (!E->d_stage_out) {
      hipError_t e_ = hipMalloc((void**)&E->d_stage_out, (size_t)out_slot * E->R);
      if (e_ != hipSuccess) { g_err = "hipMalloc(output staging) failed"; return e_ == hipErrorOutOfMemory ? CTN_OOM : CTN_HIP_ERROR; }
    }
    for (int r = 0; r < E->R; ++r) dout[r] = E->d_stage_out + (size_t)r * out_slot;
  } else {
    for (int r = 0; r < E->R; ++r) dout[r] = outs[r];
  }
  int rc = exec_set_pointers(E, din.data(), dout.data());
  if (rc != CTN_OK) return rc;
  exec_new_run(E);
  rc = exec_launch_all(E);
  if (rc != CTN_OK) return rc;
  rc = exec_fetch_checked(E, log_scale);      // may repeat the contraction in eager-rescale mode
  if (rc != CTN_OK) return rc;
  if (step_rescales) memcpy(step_rescales, E->h_resc.data(), E->h_resc.size() * 8);
  if (outs_space == CTN_MEM_HOST) {
    for (int r = 0; r < E->R; ++r) {
      if (!outs[r]) { g_err = "null output pointer"; return CTN_INVALID_ARG; }
      HIPCHECK(hipMemcpyAsync(outs[r], dout[r], (size_t)out_bytes, hipMemcpyDeviceToHost, E->stream));
    }
    HIPCHECK(hipStreamSynchronize(E->stream));
  }
  return CTN_OK;
}

int ctn_exec_snapshot_scales(ctn_exec* exec, double* dev_log_dst, int n, double* host_rescales) {
  if (!exec || n < 0 || n > exec->e.R) { g_err = "invalid argument to ctn_exec_snapshot_scales"; return CTN_INVALID_ARG; }
  Exec* E = &exec->e;
  DeviceGuard dg(E->device);
  HIPCHECK(dg.err);
  if (dev_log_dst && n)
    HIPCHECK(hipMemcpyAsync(dev_log_dst, E->d_log, (size_t)n * 8, hipMemcpyDeviceToDevice, E->stream));
  if (host_rescales && n)
    HIPCHECK(hipMemcpyAsync(host_rescales, E->d_resc, (size_t)n * E->plan->n_steps * 8, hipMemcpyDeviceToHost, E->stream));
  return CTN_OK;
}

int ctn_exec_scales_suspect(const ctn_exec* exec, const double* host_rescales, int replicas) {
  if (!exec || !host_rescales || replicas < 0) { g_err = "invalid argument to ctn_exec_scales_suspect"; return CTN_INVALID_ARG; }
  if (exec->e.eager_rescale) return 0;     // an eager run normalises every intermediate: nothing to suspect
  return exec_scales_suspect(&exec->e, host_rescales, replicas) ? 1 : 0;
}

int ctn_exec_report_suspect(ctn_exec* exec, int suspect) {
  if (!exec) { g_err = "NULL argument"; return CTN_INVALID_ARG; }
  Exec* E = &exec->e;
  if (E->eager_forced) return E->eager_streak;
  E->eager_streak = suspect ? E->eager_streak + 1 : (E->eager_streak >= kEagerSticky ? E->eager_streak : 0);
  if (E->eager_streak >= kEagerSticky) E->eager_rescale = true;     // exec_new_run keeps it from now on
  return E->eager_streak;
}

int ctn_exec_combine_split(ctn_exec* exec, int t_dtype, const void* t, int64_t t_stride, const double* c,
                           int64_t c_stride, int n, int64_t numel, double* out_packed) {
  if (!exec || !t || !c || !out_packed || n < 1 || numel < 1) { g_err = "invalid argument to ctn_exec_combine_split"; return CTN_INVALID_ARG; }
  if (n > kCombineMaxParts) { g_err = "ctn_exec_combine_split: more than 4096 parts"; return CTN_UNSUPPORTED; }
  if (t_dtype != CTN_F32 && t_dtype != CTN_F64) { g_err = "ctn_exec_combine_split: dtype must be f32 or f64"; return CTN_UNSUPPORTED; }
  Exec* E = &exec->e;
  DeviceGuard dg(E->device);
  HIPCHECK(dg.err);
  if (t_dtype == CTN_F32)
    hipLaunchKernelGGL(k_combine_split<float>, dim3(1), dim3(256), 0, E->stream, (const float*)t, t_stride, c, c_stride, n,
                       numel, E->plan->min_norm, out_packed);
  else
    hipLaunchKernelGGL(k_combine_split<double>, dim3(1), dim3(256), 0, E->stream, (const double*)t, t_stride, c, c_stride, n,
                       numel, E->plan->min_norm, out_packed);
  HIPCHECK(hipGetLastError());
  return CTN_OK;
}

int ctn_exec_add_scales(ctn_exec* exec, double* dst, const double* own, int n, int n_kids, const double* const* kid_scales,
                        const int64_t* const* kid_index) {
  if (!exec || !dst || !own || n < 0 || n_kids < 0 || (n_kids && (!kid_scales || !kid_index))) {
    g_err = "invalid argument to ctn_exec_add_scales";
    return CTN_INVALID_ARG;
  }
  if (n == 0) return CTN_OK;
  Exec* E = &exec->e;
  DeviceGuard dg(E->device);
  HIPCHECK(dg.err);
  const double* src = own;
  int done = 0;
  do {                                           // (more than 8 stages below one: several launches, dst carried along)
    ScalesAddArgs a{};
    a.dst = dst; a.own = src; a.n = n;
    a.n_kids = std::min(kScalesAddMaxKids, n_kids - done);
    for (int j = 0; j < a.n_kids; ++j) {
      if (!kid_scales[done + j] || !kid_index[done + j]) { g_err = "ctn_exec_add_scales: NULL child array"; return CTN_INVALID_ARG; }
      a.kid[j] = kid_scales[done + j]; a.idx[j] = kid_index[done + j];
    }
    hipLaunchKernelGGL(k_scales_add, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, E->stream, a);
    done += a.n_kids;
    src = dst;
  } while (done < n_kids);
  HIPCHECK(hipGetLastError());
  return CTN_OK;
}

int ctn_exec_merge_scales(ctn_exec* exec, int t_dtype, void* buf, int64_t stride, int64_t numel, double* scales, int n,
                          int ndim, const int32_t* extents, const int32_t* merged) {
  if (!exec || !buf || !scales || n < 1 || numel < 1 || stride < numel || ndim < 1 || ndim > kMergeMaxDims || !extents || !merged) {
    g_err = "invalid argument to ctn_exec_merge_scales";
    return CTN_INVALID_ARG;
  }
  if (t_dtype != CTN_F32 && t_dtype != CTN_F64) { g_err = "ctn_exec_merge_scales: dtype must be f32 or f64"; return CTN_UNSUPPORTED; }
  const int esz = t_dtype == CTN_F32 ? 4 : 8;
  if ((uintptr_t)buf % 16 || (stride * esz) % 16) { g_err = "ctn_exec_merge_scales: evaluations must start on 16-byte boundaries"; return CTN_INVALID_ARG; }
  int64_t cells = 1;
  for (int d = 0; d < ndim; ++d) { if (extents[d] < 1) { g_err = "ctn_exec_merge_scales: empty axis"; return CTN_INVALID_ARG; } cells *= extents[d]; }
  if (cells != n || n > 65535) { g_err = "ctn_exec_merge_scales: the grid of evaluations does not match n (<= 65535)"; return CTN_INVALID_ARG; }
  Exec* E = &exec->e;
  DeviceGuard dg(E->device);
  HIPCHECK(dg.err);
  const size_t need = (size_t)n * 16;
  if (E->merge_bytes < need) {
    if (E->d_merge) { HIPCHECK(hipStreamSynchronize(E->stream)); (void)hipFree(E->d_merge); E->d_merge = nullptr; E->merge_bytes = 0; }
    hipError_t e_ = hipMalloc((void**)&E->d_merge, need);
    if (e_ != hipSuccess) { g_err = "hipMalloc(merge scratch) failed"; return e_ == hipErrorOutOfMemory ? CTN_OOM : CTN_HIP_ERROR; }
    E->merge_bytes = need;
  }
  double* cum_new = (double*)E->d_merge;
  int32_t* flags = (int32_t*)(E->d_merge + (size_t)n * 8);
  HIPCHECK(hipMemsetAsync(flags, 0, (size_t)n * 4, E->stream));
  // an evaluation is cut into chunks of whole 16-byte vectors; enough workgroups to fill the chip, at most 4096 per evaluation
  const int64_t per_wg = 256 * 16;
  int64_t chunks = std::min<int64_t>(4096, std::max<int64_t>(1, (numel + per_wg - 1) / per_wg));
  chunks = std::max<int64_t>(1, std::min<int64_t>(chunks, std::max<int64_t>(1, (8LL * E->n_cu + n - 1) / n)));
  const int64_t chunk = ((numel + chunks - 1) / chunks + 1023) / 1024 * 1024;
  chunks = (numel + chunk - 1) / chunk;
  const dim3 grid((unsigned)chunks, (unsigned)n);
  MergeArgs a{};
  a.buf = buf; a.stride = stride; a.numel = numel; a.chunk = chunk; a.cum = scales; a.cum_new = cum_new; a.flags = flags;
  a.n = n; a.ndim = ndim;
  for (int d = 0; d < ndim; ++d) { a.ext[d] = extents[d]; a.merged[d] = merged[d] ? 1 : 0; }
  if (t_dtype == CTN_F32) {
    hipLaunchKernelGGL(k_merge_live<float>, grid, dim3(256), 0, E->stream, (const float*)buf, stride, numel, chunk, flags);
    hipLaunchKernelGGL(k_merge_scale<float>, grid, dim3(256), 0, E->stream, a);
  } else {
    hipLaunchKernelGGL(k_merge_live<double>, grid, dim3(256), 0, E->stream, (const double*)buf, stride, numel, chunk, flags);
    hipLaunchKernelGGL(k_merge_scale<double>, grid, dim3(256), 0, E->stream, a);
  }
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipMemcpyAsync(scales, cum_new, (size_t)n * 8, hipMemcpyDeviceToDevice, E->stream));
  return CTN_OK;
}

int ctn_exec_set_timing(ctn_exec* exec, int slots) {
  if (!exec || slots < 0) { g_err = "invalid argument"; return CTN_INVALID_ARG; }
  Exec* E = &exec->e;
  DeviceGuard dg(E->device);
  HIPCHECK(dg.err);
  HIPCHECK(hipStreamSynchronize(E->stream));
  const size_t need = (size_t)slots * E->plan->n_steps * 2;
  while (E->events.size() < need) {
    hipEvent_t ev;
    HIPCHECK(hipEventCreate(&ev));
    E->events.push_back(ev);
  }
  E->timing_slots = slots;
  E->timing_runs = 0;
  return CTN_OK;
}

int ctn_exec_step_tile(const ctn_exec* exec, int step, int32_t* tile_m, int32_t* tile_n) {
  if (!exec || !tile_m || !tile_n || step < 0 || step >= exec->e.plan->n_steps) { g_err = "invalid step query"; return CTN_INVALID_ARG; }
  const int32_t v = step < (int)exec->e.launched_tile.size() ? exec->e.launched_tile[step] : 0;
  *tile_m = v >> 16;
  *tile_n = v & 0xFFFF;
  return CTN_OK;
}

int ctn_exec_step_form(const ctn_exec* exec, int step, int32_t* form) {
  if (!exec || !form || step < 0 || step >= exec->e.plan->n_steps) { g_err = "invalid step query"; return CTN_INVALID_ARG; }
  *form = step < (int)exec->e.launched_form.size() ? exec->e.launched_form[step] : 0;
  return CTN_OK;
}

int ctn_exec_walk_form(const ctn_exec* exec, int32_t* form) {
  if (!exec || !form) { g_err = "NULL argument"; return CTN_INVALID_ARG; }
  const Exec& E = exec->e;
  *form = !(E.plan->chain && E.d_chain) ? CTN_WALK_NONE : E.d_chain_prog ? CTN_WALK_CHAIN_LDS : CTN_WALK_CHAIN;
  return CTN_OK;
}

int ctn_exec_step_ms(ctn_exec* exec, float* ms) {
  if (!exec || !ms) { g_err = "NULL argument"; return CTN_INVALID_ARG; }
  Exec* E = &exec->e;
  const int used = std::min(E->timing_runs, E->timing_slots);
  if (used < 1) { g_err = "no timed run recorded: call ctn_exec_set_timing(slots) then enqueue"; return CTN_INVALID_ARG; }
  HIPCHECK(hipStreamSynchronize(E->stream));
  const int ns = E->plan->n_steps;
  const bool chain = E->plan->chain && E->d_chain != nullptr;
  for (int s = 0; s < ns; ++s) {
    double acc = 0;
    if (chain && s > 0) { ms[s] = 0.f; continue; }  // the persistent walker is one launch, timed as step 0
    for (int slot = 0; slot < used; ++slot) {
      float t = 0;
      const size_t ev0 = ((size_t)slot * ns + s) * 2;
      HIPCHECK(hipEventElapsedTime(&t, E->events[ev0], E->events[ev0 + 1]));
      acc += t;
    }
    ms[s] = (float)(acc / used);
  }
  return CTN_OK;
}

int ctn_grad_seed(ctn_exec* exec, int dtype, const void* t_hat, const void* g_hat, const void* g_c, const double* z,
                  const double* g_in, int64_t numel, double min_norm, void* out, double* g_out, double* scratch) {
  if (!exec || !t_hat || !z || !out || !g_out || !scratch || numel < 1) { g_err = "invalid argument to ctn_grad_seed"; return CTN_INVALID_ARG; }
  if (dtype != CTN_F32 && dtype != CTN_F64) { g_err = "ctn_grad_seed: dtype must be f32 or f64"; return CTN_UNSUPPORTED; }
  Exec* E = &exec->e;
  DeviceGuard dg(E->device);
  HIPCHECK(dg.err);
  const int nb = (int)std::min<int64_t>((numel + 255) / 256, kGradSeedBlocks);
  const int dot_parts = g_hat ? nb : 0;
  if (dtype == CTN_F32) {
    if (g_hat) hipLaunchKernelGGL(k_grad_seed_dot<float>, dim3(nb), dim3(256), 0, E->stream, (const float*)g_hat, (const float*)t_hat, numel, scratch);
    hipLaunchKernelGGL(k_grad_seed_apply<float>, dim3(nb), dim3(256), 0, E->stream, (const float*)g_hat, (const float*)t_hat,
                       numel, (const float*)g_c, g_in, dot_parts, scratch, (float*)out);
    hipLaunchKernelGGL(k_grad_seed_norm<float>, dim3(nb), dim3(256), 0, E->stream, (float*)out, numel, z, g_in, nb,
                       (const double*)scratch, min_norm, g_out);
  } else {
    if (g_hat) hipLaunchKernelGGL(k_grad_seed_dot<double>, dim3(nb), dim3(256), 0, E->stream, (const double*)g_hat, (const double*)t_hat, numel, scratch);
    hipLaunchKernelGGL(k_grad_seed_apply<double>, dim3(nb), dim3(256), 0, E->stream, (const double*)g_hat, (const double*)t_hat,
                       numel, (const double*)g_c, g_in, dot_parts, scratch, (double*)out);
    hipLaunchKernelGGL(k_grad_seed_norm<double>, dim3(nb), dim3(256), 0, E->stream, (double*)out, numel, z, g_in, nb,
                       (const double*)scratch, min_norm, g_out);
  }
  HIPCHECK(hipGetLastError());
  return CTN_OK;
}

int ctn_grad_leaf(ctn_exec* exec, int src_dtype, const void* src, const double* g, int ndim, const int64_t* dims,
                  const int64_t* src_strides, const int32_t* first, int dst_dtype, void* dst) {
  if (!exec || !src || !dst || ndim < 0 || (ndim > 0 && (!dims || !src_strides || !first))) {
    g_err = "invalid argument to ctn_grad_leaf";
    return CTN_INVALID_ARG;
  }
  if (ndim > kGradMaxDims) { g_err = "ctn_grad_leaf: more than 64 axes"; return CTN_UNSUPPORTED; }
  if ((src_dtype != CTN_F32 && src_dtype != CTN_F64) || (dst_dtype != CTN_F32 && dst_dtype != CTN_F64)) {
    g_err = "ctn_grad_leaf: dtypes must be f32 or f64";
    return CTN_UNSUPPORTED;
  }
  GradLeafArgs a{};
  a.ndim = ndim;
  int64_t numel = 1;
  for (int d = ndim - 1; d >= 0; --d) {
    if (dims[d] < 0 || src_strides[d] < 0 || first[d] < 0 || first[d] > d || (first[d] != d && dims[first[d]] != dims[d])) {
      g_err = "ctn_grad_leaf: inconsistent axis description";
      return CTN_INVALID_ARG;
    }
    a.dims[d] = dims[d];
    a.dst_stride[d] = numel;
    a.src_stride[d] = first[d] == d ? src_strides[d] : 0;
    a.first[d] = first[d];
    numel *= dims[d];
  }
  a.numel = numel;
  if (numel == 0) return CTN_OK;
  Exec* E = &exec->e;
  DeviceGuard dg(E->device);
  HIPCHECK(dg.err);
  const dim3 grid((unsigned)std::min<int64_t>((numel + 255) / 256, 4096));
  if (src_dtype == CTN_F32 && dst_dtype == CTN_F32)
    hipLaunchKernelGGL((k_grad_leaf<float, float>), grid, dim3(256), 0, E->stream, a, (const float*)src, g, (float*)dst);
  else if (src_dtype == CTN_F32)
    hipLaunchKernelGGL((k_grad_leaf<float, double>), grid, dim3(256), 0, E->stream, a, (const float*)src, g, (double*)dst);
  else if (dst_dtype == CTN_F32)
    hipLaunchKernelGGL((k_grad_leaf<double, float>), grid, dim3(256), 0, E->stream, a, (const double*)src, g, (float*)dst);
  else
    hipLaunchKernelGGL((k_grad_leaf<double, double>), grid, dim3(256), 0, E->stream, a, (const double*)src, g, (double*)dst);
  HIPCHECK(hipGetLastError());
  return CTN_OK;
}

// ---------------------------------------------------------------------------
// Backward tape (include/ctn_abi.h, ctn_grad_tape_*; grad_tape.h holds the host logic).  A reverse pass as a fixed
// sequence over fixed buffers: one executor per RUN record (an executor has ONE pointer table, and a replayed graph reads
// whatever that table holds at replay time), SEED and LEAF through the tape's own table of slot addresses.  Everything
// that depends on the caller's tensors - that table and the pointer tables of the RUN records with an external slot - is
// uploaded in front of the sequence, never inside it.
// ---------------------------------------------------------------------------
struct ctn_grad_tape {
  int device = 0;
  hipStream_t stream = nullptr;
  std::vector<ctn_tape_record> recs;
  std::vector<ctn_tape_slot> slots;
  std::vector<const ctn_plan*> plans;
  std::vector<int64_t> off;
  std::vector<int> slot_align;           // per slot: the largest element size a record reads or writes there
  std::vector<GradLeafArgs> leaf;        // per record (LEAF only)
  std::vector<ctn_exec*> execs;          // per record (RUN only)
  std::vector<int> ext_runs;             // RUN records with an external slot: pointer table refreshed on every run
  int n_ext = 0, n_regs = 0, n_execs = 0;
  int64_t arena_bytes = 0, regs_bytes = 0;
  char* d_arena = nullptr;
  void** d_tab = nullptr;                // [n_slots] slot addresses
  std::vector<void*> h_tab;
  bool tab_valid = false;
  int use_graph = 1;
  bool warm = false;
  hipGraphExec_t graph_exec = nullptr;
  int64_t n_eager = 0, n_captured = 0, n_replayed = 0;
  int64_t graph_nodes = 0;                   // nodes of the captured graph (hipGraphGetNodes at capture time), 0 before
  int64_t device_bytes = 0, create_us = 0;   // what creation took from the device (arena, table, executors) and how long

  ~ctn_grad_tape() {
    DeviceGuard dg(device);
    // hipFree waits for the device: nothing of the last run is in flight when the graph and the executors go (the
    // stream is the caller's and may be gone by now: it is not touched here)
    if (d_arena) (void)hipFree(d_arena);
    if (d_tab) (void)hipFree(d_tab);
    if (graph_exec) (void)hipGraphExecDestroy(graph_exec);
    for (ctn_exec* x : execs)
      if (x) ctn_exec_destroy(x);
  }
  double* reg(int i) const { return i < 0 ? nullptr : (double*)d_arena + i; }
};

static int64_t tape_slot_bytes(const ctn_grad_tape* T, int s) { return T->slots[s].external ? INT64_MAX : T->slots[s].bytes; }

// Sizes: every arena slot a record touches is large enough for what the kernels read and write there.
static const char* tape_check_sizes(const ctn_grad_tape* T, const ctn_tape_desc& d) {
  for (size_t i = 0; i < T->recs.size(); ++i) {
    const ctn_tape_record& r = T->recs[i];
    if (r.kind == CTN_TAPE_RUN) {
      const Plan& P = T->plans[r.plan]->p;
      if (P.n_steps != 1 || P.n_inputs != (r.in[1] >= 0 ? 2 : 1) || r.src_dtype != P.dtype) return "a RUN record needs a one-step plan of its arity and dtype";
      const int64_t es = P.elem_size();
      for (int j = 0; j < P.n_inputs; ++j)
        if (P.tensors[j].numel * es > tape_slot_bytes(T, r.in[j])) return "a RUN record's operand is larger than its slot";
      if (ctn_plan_out_bytes(T->plans[r.plan]) > tape_slot_bytes(T, r.out)) return "a RUN record's result is larger than its slot";
    } else if (r.kind == CTN_TAPE_SEED) {
      const int64_t b = r.numel * (r.src_dtype == CTN_F64 ? 8 : 4);
      if (b > tape_slot_bytes(T, r.in[0]) || (r.in[1] >= 0 && b > tape_slot_bytes(T, r.in[1])) || b > tape_slot_bytes(T, r.out))
        return "a SEED record's tensors are larger than their slots";
    } else {
      int64_t numel = 1, reach = 0;
      for (int a = 0; a < r.ndim; ++a) {
        const int64_t dim = d.leaf_dims[r.axes + a], st = d.leaf_strides[r.axes + a];
        const int32_t f = d.leaf_first[r.axes + a];
        if (dim < 0 || st < 0 || f < 0 || f > a || (f != a && d.leaf_dims[r.axes + f] != dim)) return "a LEAF record's axis description is inconsistent";
        numel *= dim;
        if (f == a && dim > 0) reach += (dim - 1) * st;
      }
      if (numel > 0 && (reach + 1) * (r.src_dtype == CTN_F64 ? 8 : 4) > tape_slot_bytes(T, r.in[0])) return "a LEAF record reads past its source slot";
      if (numel * (r.dst_dtype == CTN_F64 ? 8 : 4) > tape_slot_bytes(T, r.out)) return "a LEAF record writes past its destination slot";
    }
  }
  return nullptr;
}

static int tape_set_run_pointers(ctn_grad_tape* T, int i) {
  const ctn_tape_record& r = T->recs[i];
  const void* ins[2] = {T->h_tab[r.in[0]], r.in[1] >= 0 ? T->h_tab[r.in[1]] : nullptr};
  void* outs[1] = {T->h_tab[r.out]};
  return exec_set_pointers(&T->execs[i]->e, ins, outs);
}

// The whole sequence on the tape's stream: nothing here depends on the caller's pointers, nothing copies from the host.
static int tape_issue(ctn_grad_tape* T) {
  hipStream_t st = T->stream;
  double* regs = (double*)T->d_arena;
  HIPCHECK(hipMemsetAsync(regs, 0, (size_t)T->regs_bytes, st));
  for (size_t i = 0; i < T->recs.size(); ++i) {
    const ctn_tape_record& r = T->recs[i];
    if (r.kind == CTN_TAPE_RUN) {
      Exec* E = &T->execs[i]->e;
      exec_new_run(E);
      if (tape_closes(r)) {                        // the register work rides in the run's own finish (k_run_close)
        const RunClose close{regs, r.reg[0], r.reg[1], r.reg[2], r.reg[3]};
        const int rc = exec_launch_all(E, &close);
        if (rc != CTN_OK) return rc;
        continue;
      }
      const int rc = exec_launch_all(E);
      if (rc != CTN_OK) return rc;
      hipLaunchKernelGGL(k_tape_regs, dim3(1), dim3(64), 0, st, (const double*)E->d_log, regs, r.reg[0], r.reg[1], r.reg[2], r.reg[3]);
    } else if (r.kind == CTN_TAPE_SEED) {
      const int64_t numel = r.numel;
      const int nb = (int)std::min<int64_t>((numel + 255) / 256, kGradSeedBlocks);
      const int dot_parts = r.in[1] >= 0 ? nb : 0;
      double* scratch = (double*)(T->d_arena + T->off[r.aux]);
      void* const* tab = T->d_tab;
      if (r.src_dtype == CTN_F32) {
        if (r.in[1] >= 0) hipLaunchKernelGGL(k_grad_seed_dot_tab<float>, dim3(nb), dim3(256), 0, st, tab, r.in[1], r.in[0], numel, scratch);
        hipLaunchKernelGGL(k_grad_seed_apply_tab<float>, dim3(nb), dim3(256), 0, st, tab, r.in[1], r.in[0], numel, r.in[2],
                           (const double*)T->reg(r.reg[1]), dot_parts, scratch, r.out);
        hipLaunchKernelGGL(k_grad_seed_norm_tab<float>, dim3(nb), dim3(256), 0, st, tab, r.out, numel, (const double*)T->reg(r.reg[0]),
                           (const double*)T->reg(r.reg[1]), nb, (const double*)scratch, r.min_norm, T->reg(r.reg[2]));
      } else {
        if (r.in[1] >= 0) hipLaunchKernelGGL(k_grad_seed_dot_tab<double>, dim3(nb), dim3(256), 0, st, tab, r.in[1], r.in[0], numel, scratch);
        hipLaunchKernelGGL(k_grad_seed_apply_tab<double>, dim3(nb), dim3(256), 0, st, tab, r.in[1], r.in[0], numel, r.in[2],
                           (const double*)T->reg(r.reg[1]), dot_parts, scratch, r.out);
        hipLaunchKernelGGL(k_grad_seed_norm_tab<double>, dim3(nb), dim3(256), 0, st, tab, r.out, numel, (const double*)T->reg(r.reg[0]),
                           (const double*)T->reg(r.reg[1]), nb, (const double*)scratch, r.min_norm, T->reg(r.reg[2]));
      }
    } else {
      const GradLeafArgs& a = T->leaf[i];
      if (a.numel == 0) continue;
      const dim3 grid((unsigned)std::min<int64_t>((a.numel + 255) / 256, 4096));
      const double* g = T->reg(r.reg[0]);
      void* const* tab = T->d_tab;
      if (r.src_dtype == CTN_F32 && r.dst_dtype == CTN_F32)
        hipLaunchKernelGGL((k_grad_leaf_tab<float, float>), grid, dim3(256), 0, st, a, tab, r.in[0], g, r.out);
      else if (r.src_dtype == CTN_F32)
        hipLaunchKernelGGL((k_grad_leaf_tab<float, double>), grid, dim3(256), 0, st, a, tab, r.in[0], g, r.out);
      else if (r.dst_dtype == CTN_F32)
        hipLaunchKernelGGL((k_grad_leaf_tab<double, float>), grid, dim3(256), 0, st, a, tab, r.in[0], g, r.out);
      else
        hipLaunchKernelGGL((k_grad_leaf_tab<double, double>), grid, dim3(256), 0, st, a, tab, r.in[0], g, r.out);
    }
  }
  HIPCHECK(hipGetLastError());
  return CTN_OK;
}

int ctn_grad_tape_create(const ctn_tape_desc* desc, int device, void* stream, ctn_grad_tape** out) {
  if (!desc || !out || !stream) { g_err = "invalid argument to ctn_grad_tape_create"; return CTN_INVALID_ARG; }
  *out = nullptr;
  std::vector<TapeLife> life;
  std::string why = tape_check_records(*desc, &life);
  if (!why.empty()) { g_err = "ctn_grad_tape_create: " + why; return CTN_INVALID_ARG; }
  for (int p = 0; p < desc->n_plans; ++p)
    if (!desc->plans || !desc->plans[p]) { g_err = "ctn_grad_tape_create: NULL plan"; return CTN_INVALID_ARG; }
  ctn_grad_tape* T = new (std::nothrow) ctn_grad_tape();
  if (!T) { g_err = "out of host memory"; return CTN_OOM; }
  // a failed creation leaves no HIP error behind: the caller may walk step by step instead (CTN_UNSUPPORTED, CTN_OOM)
  auto fail = [&](int code) { delete T; (void)hipGetLastError(); return code; };
  const auto t_begin = std::chrono::steady_clock::now();
  T->device = device;
  T->recs.assign(desc->records, desc->records + desc->n_records);
  T->slots.assign(desc->slots, desc->slots + desc->n_slots);
  if (desc->n_plans) T->plans.assign(desc->plans, desc->plans + desc->n_plans);
  T->n_ext = desc->n_ext; T->n_regs = desc->n_regs;
  T->regs_bytes = tape_round_up((int64_t)desc->n_regs * 8);
  T->arena_bytes = tape_layout(*desc, life, &T->off);
  why = tape_check_layout(*desc, life, T->off, T->arena_bytes);
  if (!why.empty()) { g_err = "ctn_grad_tape_create: " + why; return fail(CTN_INVALID_ARG); }
  if (const char* bad = tape_check_sizes(T, *desc)) { g_err = std::string("ctn_grad_tape_create: ") + bad; return fail(CTN_INVALID_ARG); }
  const int64_t cap = desc->max_bytes > 0 ? desc->max_bytes : kTapeDefaultMaxBytes;
  if (T->arena_bytes > cap) {
    g_err = "ctn_grad_tape_create: the arena needs " + std::to_string(T->arena_bytes) + " bytes, more than the cap of " + std::to_string(cap);
    return fail(CTN_UNSUPPORTED);
  }
  T->leaf.resize(T->recs.size());
  T->slot_align.assign(desc->n_slots, 4);
  for (size_t i = 0; i < T->recs.size(); ++i) {
    const ctn_tape_record& r = T->recs[i];
    const int es_in = r.src_dtype == CTN_F64 ? 8 : 4, es_out = r.kind == CTN_TAPE_LEAF ? (r.dst_dtype == CTN_F64 ? 8 : 4) : es_in;
    for (int j = 0; j < 3; ++j)
      if (r.in[j] >= 0) T->slot_align[r.in[j]] = std::max(T->slot_align[r.in[j]], es_in);
    T->slot_align[r.out] = std::max(T->slot_align[r.out], es_out);
    if (r.kind != CTN_TAPE_LEAF) continue;
    GradLeafArgs a{};
    a.ndim = r.ndim;
    int64_t numel = 1;
    for (int d = r.ndim - 1; d >= 0; --d) {
      const int32_t f = desc->leaf_first[r.axes + d];
      a.dims[d] = desc->leaf_dims[r.axes + d];
      a.dst_stride[d] = numel;
      a.src_stride[d] = f == d ? desc->leaf_strides[r.axes + d] : 0;
      a.first[d] = f;
      numel *= a.dims[d];
    }
    a.numel = numel;
    T->leaf[i] = a;
  }
  int ndev = 0;
  int rc = ctn_device_count(&ndev);
  if (rc != CTN_OK) return fail(rc);
  if (device < 0 || device >= ndev) { g_err = "device index out of range"; return fail(CTN_INVALID_ARG); }
  DeviceGuard dg(device);
  if (dg.err != hipSuccess) { g_err = "hipSetDevice failed"; return fail(CTN_HIP_ERROR); }
  T->stream = (hipStream_t)stream;
  T->use_graph = read_dev_switches().graph;
#define HIPCHECK_T(expr)                                                        \
  do {                                                                          \
    hipError_t e_ = (expr);                                                     \
    if (e_ != hipSuccess) {                                                     \
      g_err = std::string(#expr) + ": " + hipGetErrorString(e_);                \
      return fail(e_ == hipErrorOutOfMemory ? CTN_OOM : CTN_HIP_ERROR);         \
    }                                                                           \
  } while (0)
  size_t free_before = 0, free_after = 0, total_mem = 0;
  HIPCHECK_T(hipMemGetInfo(&free_before, &total_mem));
  HIPCHECK_T(hipMalloc((void**)&T->d_arena, (size_t)T->arena_bytes));
  HIPCHECK_T(hipMalloc((void**)&T->d_tab, (size_t)desc->n_slots * sizeof(void*)));
  T->h_tab.assign(desc->n_slots, nullptr);
  for (int s = 0; s < desc->n_slots; ++s)
    if (!T->slots[s].external && T->off[s] >= 0) T->h_tab[s] = T->d_arena + T->off[s];
  T->execs.assign(T->recs.size(), nullptr);
  for (size_t i = 0; i < T->recs.size(); ++i) {
    const ctn_tape_record& r = T->recs[i];
    if (r.kind != CTN_TAPE_RUN) continue;
    rc = ctn_exec_create(T->plans[r.plan], device, stream, 1, &T->execs[i]);
    if (rc != CTN_OK) return fail(rc);
    ++T->n_execs;
    (void)ctn_exec_set_rescale_mode(T->execs[i], 1);       // eager: one-step runs are never "suspect", nothing to fetch
    if (tape_closes(r) && !exec_may_close(&T->execs[i]->e)) {
      g_err = "ctn_grad_tape_create: record " + std::to_string(i) + " closes, but its plan may not (one step, one replica)";
      return fail(CTN_INVALID_ARG);
    }
    const bool ext = T->slots[r.in[0]].external || (r.in[1] >= 0 && T->slots[r.in[1]].external);
    if (ext) { T->ext_runs.push_back((int)i); continue; }
    rc = tape_set_run_pointers(T, (int)i);                  // all in the arena: set once, before any capture
    if (rc != CTN_OK) return fail(rc);
  }
  HIPCHECK_T(hipMemGetInfo(&free_after, &total_mem));
#undef HIPCHECK_T
  T->device_bytes = free_before > free_after ? (int64_t)(free_before - free_after) : 0;
  T->create_us = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t_begin).count();
  *out = T;
  return CTN_OK;
}

int ctn_grad_tape_run(ctn_grad_tape* T, void* const* ext, int n_ext) {
  if (!T || n_ext != T->n_ext || (n_ext > 0 && !ext)) { g_err = "invalid argument to ctn_grad_tape_run"; return CTN_INVALID_ARG; }
  DeviceGuard dg(T->device);
  HIPCHECK(dg.err);
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  const bool foreign_capture = hipStreamIsCapturing(T->stream, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone;
  if (foreign_capture) (void)hipGetLastError();
  // 1. everything that follows the caller's tensors, in front of the sequence
  // every pointer is checked before h_tab is touched: a refused call leaves the tape as it was
  for (size_t s = 0; s < T->slots.size(); ++s) {
    if (!T->slots[s].external) continue;
    void* p = ext[T->slots[s].ext_index];
    if (!p) { g_err = "ctn_grad_tape_run: NULL external pointer"; return CTN_INVALID_ARG; }
    if ((uintptr_t)p % T->slot_align[s]) { g_err = "ctn_grad_tape_run: external pointers must be element aligned"; return CTN_INVALID_ARG; }
  }
  bool changed = !T->tab_valid;
  for (size_t s = 0; s < T->slots.size(); ++s) {
    if (!T->slots[s].external) continue;
    void* p = ext[T->slots[s].ext_index];
    if (T->h_tab[s] != p) { T->h_tab[s] = p; changed = true; }
  }
  if (changed) {
    T->tab_valid = false;                    // until the upload is queued: a failure below uploads again next time
    HIPCHECK(hipMemcpyAsync(T->d_tab, T->h_tab.data(), T->h_tab.size() * sizeof(void*), hipMemcpyHostToDevice, T->stream));
    T->tab_valid = true;
  }
  for (int i : T->ext_runs) {
    const int rc = tape_set_run_pointers(T, i);
    if (rc != CTN_OK) return rc;
  }
  // 2. the sequence: eager, captured, replayed (as exec_launch_all)
  if (!T->use_graph || foreign_capture) { ++T->n_eager; return tape_issue(T); }
  if (!T->graph_exec) {
    if (!T->warm) { T->warm = true; ++T->n_eager; return tape_issue(T); }
    hipGraph_t g = nullptr;
    if (hipStreamBeginCapture(T->stream, hipStreamCaptureModeThreadLocal) != hipSuccess) {
      (void)hipGetLastError();
      T->use_graph = 0;
      ++T->n_eager;
      return tape_issue(T);
    }
    const int rc = tape_issue(T);
    const hipError_t ec = hipStreamEndCapture(T->stream, &g);
    if (rc != CTN_OK || ec != hipSuccess || !g || hipGraphInstantiate(&T->graph_exec, g, nullptr, nullptr, 0) != hipSuccess) {
      (void)hipGetLastError();
      if (g) (void)hipGraphDestroy(g);
      T->graph_exec = nullptr;
      T->use_graph = 0;                      // eager for good
      if (rc != CTN_OK) return rc;
      ++T->n_eager;
      return tape_issue(T);
    }
    size_t n_nodes = 0;
    if (hipGraphGetNodes(g, nullptr, &n_nodes) == hipSuccess) T->graph_nodes = (int64_t)n_nodes;
    else (void)hipGetLastError();
    (void)hipGraphDestroy(g);
    HIPCHECK(hipGraphLaunch(T->graph_exec, T->stream));
    ++T->n_captured;
    return CTN_OK;
  }
  HIPCHECK(hipGraphLaunch(T->graph_exec, T->stream));
  ++T->n_replayed;
  return CTN_OK;
}

int ctn_grad_tape_info(const ctn_grad_tape* T, int64_t* info) {
  if (!T || !info) { g_err = "invalid argument to ctn_grad_tape_info"; return CTN_INVALID_ARG; }
  info[0] = (int64_t)T->recs.size(); info[1] = T->arena_bytes; info[2] = T->n_execs;
  info[3] = T->n_eager; info[4] = T->n_captured; info[5] = T->n_replayed;
  info[6] = T->regs_bytes; info[7] = (int64_t)T->slots.size();
  info[8] = T->device_bytes; info[9] = T->create_us;
  return CTN_OK;
}

int ctn_grad_tape_graph_nodes(const ctn_grad_tape* T, int64_t* nodes) {
  if (!T || !nodes) { g_err = "invalid argument to ctn_grad_tape_graph_nodes"; return CTN_INVALID_ARG; }
  *nodes = T->graph_nodes;
  return CTN_OK;
}

void ctn_grad_tape_destroy(ctn_grad_tape* tape) { delete tape; }

static_assert(kCplxBlocks <= CTN_CPLX_SCRATCH, "one scratch double per workgroup of the complex reductions");
static bool aligned16(const void* p) { return p == nullptr || ((uintptr_t)p & 15) == 0; }

int ctn_cplx_normalize(ctn_exec* exec, int dtype, const void* t_e, const void* c_e, int rescaled, int64_t numel,
                       void* t, void* c, double* rho_out, double* scratch) {
  if (!exec || !t_e || !c_e || !t || !c || !rho_out || (rescaled && !scratch) || numel < 1) {
    g_err = "invalid argument to ctn_cplx_normalize";
    return CTN_INVALID_ARG;
  }
  if (dtype != CTN_F32 && dtype != CTN_F64) { g_err = "ctn_cplx_normalize: dtype must be f32 or f64"; return CTN_UNSUPPORTED; }
  Exec* E = &exec->e;
  DeviceGuard dg(E->device);
  HIPCHECK(dg.err);
  const int vec = aligned16(t_e) && aligned16(t) ? 1 : 0;
  const int64_t items = vec ? (2 * numel * (dtype == CTN_F32 ? 4 : 8) + 15) / 16 : numel;
  const int nb = (int)std::min<int64_t>((items + 255) / 256, kCplxBlocks);
  const int parts = rescaled ? nb : 0;
  const dim3 ga((unsigned)std::max<int64_t>(1, std::min<int64_t>((items + 255) / 256, 4096)));
  if (dtype == CTN_F32) {
    if (rescaled) hipLaunchKernelGGL(k_cplx_abs_sum<float>, dim3(nb), dim3(256), 0, E->stream, (const float*)t_e, numel, vec, scratch);
    hipLaunchKernelGGL(k_cplx_normalize<float>, ga, dim3(256), 0, E->stream, (const float*)t_e, (float*)t, numel, vec,
                       (const double*)scratch, parts, rescaled ? 1 : 0, (const float*)c_e, (float*)c, rho_out);
  } else {
    if (rescaled) hipLaunchKernelGGL(k_cplx_abs_sum<double>, dim3(nb), dim3(256), 0, E->stream, (const double*)t_e, numel, vec, scratch);
    hipLaunchKernelGGL(k_cplx_normalize<double>, ga, dim3(256), 0, E->stream, (const double*)t_e, (double*)t, numel, vec,
                       (const double*)scratch, parts, rescaled ? 1 : 0, (const double*)c_e, (double*)c, rho_out);
  }
  HIPCHECK(hipGetLastError());
  return CTN_OK;
}

int ctn_cplx_normalize_grad(ctn_exec* exec, int dtype, const void* t, const void* g_t, const void* g_c,
                            const double* rho, int64_t numel, void* g_te, double* scratch) {
  if (!exec || !t || !rho || !g_te || !scratch || numel < 1) { g_err = "invalid argument to ctn_cplx_normalize_grad"; return CTN_INVALID_ARG; }
  if (dtype != CTN_F32 && dtype != CTN_F64) { g_err = "ctn_cplx_normalize_grad: dtype must be f32 or f64"; return CTN_UNSUPPORTED; }
  Exec* E = &exec->e;
  DeviceGuard dg(E->device);
  HIPCHECK(dg.err);
  const int vec = aligned16(t) && aligned16(g_t) && aligned16(g_te) ? 1 : 0;
  const int64_t items = vec ? (2 * numel * (dtype == CTN_F32 ? 4 : 8) + 15) / 16 : numel;
  const int nb = (int)std::min<int64_t>((items + 255) / 256, kCplxBlocks);
  const int parts = g_t ? nb : 0;
  const dim3 ga((unsigned)std::max<int64_t>(1, std::min<int64_t>((items + 255) / 256, 4096)));
  if (dtype == CTN_F32) {
    if (g_t) hipLaunchKernelGGL(k_cplx_grad_dot<float>, dim3(nb), dim3(256), 0, E->stream, (const float*)g_t, (const float*)t, numel, vec, scratch);
    hipLaunchKernelGGL(k_cplx_grad_apply<float>, ga, dim3(256), 0, E->stream, (const float*)g_t, (const float*)t, numel, vec,
                       (const double*)scratch, parts, (const float*)g_c, rho, (float*)g_te);
  } else {
    if (g_t) hipLaunchKernelGGL(k_cplx_grad_dot<double>, dim3(nb), dim3(256), 0, E->stream, (const double*)g_t, (const double*)t, numel, vec, scratch);
    hipLaunchKernelGGL(k_cplx_grad_apply<double>, ga, dim3(256), 0, E->stream, (const double*)g_t, (const double*)t, numel, vec,
                       (const double*)scratch, parts, (const double*)g_c, rho, (double*)g_te);
  }
  HIPCHECK(hipGetLastError());
  return CTN_OK;
}

}  // extern "C"
