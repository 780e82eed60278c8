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
// Written for CDNA4 only: 64-lane waves, v_mfma_f32_32x32x2_f32, 160 KiB LDS/CU.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "plan.h"
#include "chain_pack.h"
#include "cplx_match.h"
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
#include "kernels_zip128.h"
#include "kernels_zipm64.h"
#include "kernels_zip_f64.h"
#include "kernels_zipl.h"
#include "kernels_sweep.h"
#include "kernels_sweep_f64.h"
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
  // zipper pairs (kernels_zip.h): zip[s2] describes the fused launch of steps (s2 - 1, s2); zip_skip[s1] = the first
  // step of such a pair is never launched (its result only exists in the fused kernel's registers)
  struct ZipDesc { bool on = false; int64_t ldE = 0, ldXq = 0, ldXk = 0, ldYq = 0, ldYm = 0, ldC = 0; int Q = 0, U = 0, K1 = 0;
                   int zu = 128; bool f64 = false;      // zu: values of u per workgroup (128: k_zip_f32, 64: k_zip64_f32, k_zip_f64)
                   int zm = 256;
                   bool zq = false, zqp = false;        // zq: k_zipq_f32 runs the pair (zu = 128, zm = 256, Q even); zqp: as k_zipqp_f32                     // zm: |m1| = |n2| (256; 128: k_zip128_f32, zu = 128; 64: k_zipm64_f32, zu = 64)
                   int form = CTN_FORM_NONE; };         // the kernel that runs the pair (ctn_step_form), set where it is chosen
  std::vector<ZipDesc> zip;
  std::vector<char> zip_skip;
  // k_zipqp_f32 only: results that the plan's workspace puts where the pair's own E lies (the planner frees E at the
  // pair's first step, and first fit hands its bytes to E') live in side buffers instead - zqp_side[id] = which one, or -1.
  // A workgroup of k_zipq_f32 stores its rows of E' when every workgroup of the replica has long read E; a workgroup
  // that goes on to the replica's next block of u has not.
  char* d_zqp_side = nullptr;
  std::vector<int> zqp_side;
  int64_t zqp_side_bytes = 0;       // one replica's part of one side buffer
  // the same pairs in their latency form (kernels_zipl.h): zl[s2] = the fused launch of steps (s2 - 1, s2), whose result
  // leaves as slabs; from_prev = its E is the slabs of the pair before, feeds_next = the next pair adds its slabs up (else
  // k_zip_slab_sum does); zl_skip[s1] like zip_skip
  struct ZipLat { bool on = false, from_prev = false, feeds_next = false; int buf = 0, mp = 32; ZipDesc d; };
  std::vector<ZipLat> zl;
  std::vector<char> zl_skip;
  float* d_zl_slab[2] = {nullptr, nullptr};   // [R][S][U][ZM] each, ping-pong along the chain
  // complex x complex step pairs (kernels_cmfma.h): cplx[s] describes the fused launch of step s, a GEMM, with the S step
  // that produces its operand; cplx_skip[that step] = the S step is never launched (the widened operand only exists in registers).
  // (CplxDesc: cplx_match.h; its t* fields are offsets of the pair-granular tables inside d_cplx_tabs)
  std::vector<CplxDesc> cplx;
  std::vector<char> cplx_skip;
  int32_t* d_cplx_tabs = nullptr;
  // a sweep (kernels_sweep.h): a run of epilogue-summed GEMM steps, each on the result of the one before, walked by ONE
  // launch at the position of its last member; sweep_role[s] = 1 a member that is never launched, 2 the last member
  struct SweepDesc {
    bool on = false;
    std::vector<int> steps;          // the members' step indices, in chain order
    int64_t ldIn = 0, ldOut = 0, ldWl = 0, ldWp = 0, ldX = 0;
    int J = 0, M = 0, D = 0, Pd = 0;     // row blocks, rows, bond and physical dimension
    // float64 (kernels_sweep_f64.h): the members are the 2 S steps of S sites - (GEMM, streaming sum over p) pairs, both
    // reporting a rescale factor; ids = [S][2] tensor ids (W_s, x_s), idIn the chain's input E
    bool f64 = false;
    int idIn = -1;
    std::vector<int32_t> ids;
  };
  SweepDesc sweep;
  std::vector<char> sweep_role;
  int32_t* d_sweep_ids = nullptr;      // [S][2] tensor ids (W_s, x_s)
  int64_t* d_sweep_off = nullptr;      // [S] step_off of the members
  int32_t* d_sweep_slots = nullptr;    // [S] step_partials of the members
  double* d_sweep_a = nullptr;         // [R][S][J]
  float* d_sweep_s = nullptr;          // [R][S][J]
  double* d_sweep_z = nullptr;         // [R][S]
  double* d_sweep_la = nullptr;        // [R][S][J] logs of d_sweep_a / d_sweep_s
  double* d_sweep_ls = nullptr;
  int32_t* d_sweep_e = nullptr;        // float64: [R][S][J] exponents of the blocks' scales (d_sweep_a: [R][2 S][J], d_sweep_z: [R][2 S])
  // steps with a small resident left operand against a very wide right one (kernels_mfma_ares.h): column tiles per workgroup
  // (bit 16: the left operand takes 16-byte loads), 0 = not taken
  std::vector<int> ares_ntw;
  // full dots of a tensor with a transposed one (k_dot_tr), found on the plan's tables when the executor is created
  struct DotTr { bool on = false; int Ka = 0, Kb = 0, x_is_a = 1; int64_t ldY = 0; };
  std::vector<DotTr> dot_tr;
  std::vector<int32_t> launched_form;  // per step: ctn_step_form of the last enqueue (ctn_exec_step_form), else 0
  std::vector<int32_t> launched_tile;  // per step: (tile rows << 16 | tile columns) of the last enqueue's MFMA kernel, else 0
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
  std::vector<int> step_partials;   // abs-sum partials per replica of every step (plan value unless split-K / latency form)
  std::vector<int64_t> step_off;    // d_partials: step s, replica r at (step_off[s] * R + r * step_partials[s]) doubles
  int64_t part_slots = 0;           // sum of the steps' slots
  int64_t* d_stepOff = nullptr;
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
  // Grouped leaf steps: runs of consecutive streaming steps whose operands are all network inputs (independent of
  // each other and of everything before them) go out as ONE launch of k_stream_group; their arguments never
  // change, so they are built on the first enqueue and kept in device memory.
  struct LeafGroup { int len = 0, vw = 1, u = 1, blocks = 1, off = 0; bool ready = false; };
  std::vector<LeafGroup> groups;    // per step: len >= 2 at the head of a group, else 0
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

// Is k_zip_f64 taken without CTN_ZIP=1 when its launch fills the chip?  Decided by measurement.
static constexpr bool kZipF64Default = false;
// Is k_zip128_f32 taken without CTN_ZIP=1 when its launch fills the chip?  Decided by measurement.
static constexpr bool kZip128Default = false;
// Is k_zipm64_f32 taken without CTN_ZIP=1 when its launch fills the chip?  Decided by measurement.
static constexpr bool kZipM64Default = false;

// Do steps (s2 - 1, s2) form a zipper pair that k_zip_f32 (`dtype` CTN_F32; `zm` = 128: k_zip128_f32, 64: k_zipm64_f32) or k_zip_f64 (CTN_F64)
// can run as one launch?
// Checked on the plan's own offset tables (every operand dense along its innermost index with uniform strides), so
// nothing about the network's labels is assumed: T = E . X with |m1| = zm rows from E, columns (q, u) from X;
// E' = T . Y contracting (m1, q), |n2| = zm.  The element type decides the kernel kind of the two steps, the depth of a
// phase-1 tile and - fp64: 16-byte requests and stores of pairs of doubles - that every leading dimension is even.
static bool zip_match(const Plan& P, int s2, Exec::ZipDesc* z, int dtype, int u_mult = ZU, int zm = ZM) {
  if (s2 < 1 || s2 + 1 >= P.n_steps || P.dtype != dtype || (dtype != CTN_F32 && dtype != CTN_F64)) return false;
  const bool f64 = dtype == CTN_F64;
  const int kt = f64 ? ZDK : ZK;
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
static bool zipq_fits(const Exec::ZipDesc& z) {
  const int64_t lim = (int64_t)1 << 31;
  return z.Q >= 2 && z.Q % 2 == 0 && (int64_t)z.K1 * z.ldE * 4 < lim && ((int64_t)z.Q * z.ldXq + (int64_t)z.K1 * z.ldXk + z.U) * 4 < lim &&
         ((int64_t)z.Q * z.ldYq + (int64_t)ZM * z.ldYm) * 4 < lim;
}

// Is k_cmfma_f32 taken without CTN_CPLX=1 wherever cplx_match takes a pair?  Decided by measurement (DESIGN sections 10
// and 11): tools/cplx_step_timing.py has to show the fused form ahead of the two launches by more than the larger spread
// at every one of its shapes, and the complex GPU suite has to be green with CTN_CPLX=1.
static constexpr bool kCplxDefault = false;

// Is a chain plan walked by k_chain_lds without CTN_CHAIN=2 wherever chain_pack accepts it?  Decided by measurement
// (DESIGN sections 10 and 11): tools/chain_timing.py has to show it ahead of k_chain by more than the larger spread at
// every workload it measures, and the whole suite has to be green with it on.  Results are bit-identical either way.
static constexpr bool kChainLdsDefault = false;

// Is step s an epilogue-summed GEMM step that k_sweep_f32 can take as one site of a sweep?  Checked on the plan's own
// offset tables: E row-major [b][l], W[l][p][r] with r unit-stride, x[b][p] with p unit-stride, result rows [b][r].
struct SweepShape { int64_t ldA = 0, ldC = 0, ldWl = 0, ldWp = 0, ldX = 0, M = 0; int D = 0, Pd = 0; };
static bool sweep_step_shape(const Plan& P, int s, SweepShape* sh) {
  const Step& st = P.steps[s];
  const int D = (int)st.K, Pd = st.epw;
  if (P.dtype != CTN_F32 || st.kernel != CTN_KERNEL_MFMA_F32 || (Pd != 2 && Pd != 4) || st.Bt != 1 ||
      (st.K != 64 && st.K != 128 && st.K != 256 && st.K != 512) || st.N != (int64_t)D * Pd || s + 1 >= P.n_steps)
    return false;
  // (st.collapse - the step's OWN launch would have more workgroups than partial slots and leave one collapsed slot - is
  // no obstacle: a member is never launched, and k_sweep_finish fills however many slots the step has, slot 0 first)
  if (st.rhs < 0 || st.rhs >= P.n_inputs || st.lhs2 < 0 || st.lhs2 >= P.n_inputs) return false;   // W, x: network inputs
  const int32_t* T = P.tables.data();
  const int32_t *omA = T + st.t.omA, *okA = T + st.t.okA, *onB = T + st.t.onB, *okB = T + st.t.okB, *omC = T + st.t.omC,
                *onC = T + st.t.onC, *omX = T + st.t.omA2;
  const int64_t M = st.M;
  const int64_t ldA = M > 1 ? omA[1] : D, ldC = M > 1 ? omC[1] : D, ldX = M > 1 ? omX[1] : Pd, ldWl = okB[1];
  for (int64_t m = 0; m < M; ++m)
    if (omA[m] != m * ldA || omC[m] != m * ldC || omX[m] != m * ldX) return false;
  for (int k = 0; k < D; ++k)
    if (okA[k] != k || okB[k] != (int64_t)k * ldWl) return false;
  int64_t ldWp = INT64_MAX;
  for (int n = 0; n < D * Pd; ++n)
    if (onB[n] >= D) ldWp = std::min<int64_t>(ldWp, onB[n]);
  if (ldWp == INT64_MAX) return false;
  std::vector<char> seen((size_t)D * Pd, 0);
  for (int n = 0; n < D * Pd; ++n) {
    const int64_t off = onB[n], pp = off / ldWp, rr = off % ldWp;
    if (off < 0 || pp >= Pd || rr >= D || onC[n] != rr || seen[(size_t)(pp * D + rr)]) return false;
    seen[(size_t)(pp * D + rr)] = 1;
  }
  if (ldA < D || ldC < D || ldA % 4 || ldC % 4 || ldX % Pd || ldX < Pd || ldWl % 4 || ldWp % 4 || ldWl < D) return false;
  if (((D + 12) * ldWl + 3 * ldWp + D) * 4 >= ((int64_t)1 << 31)) return false;   // a lane's offsets into a core: 32 bits
  sh->ldA = ldA; sh->ldC = ldC; sh->ldWl = ldWl; sh->ldWp = ldWp; sh->ldX = ldX; sh->M = M; sh->D = D; sh->Pd = Pd;
  return true;
}

// The longest run of such steps, each taking the result of the one before as its E.
static bool sweep_match(const Plan& P, Exec::SweepDesc* d) {
  std::vector<int> best;
  SweepShape best_first, best_last;
  std::vector<char> used((size_t)P.n_steps, 0);
  for (int s0 = 0; s0 < P.n_steps; ++s0) {
    SweepShape first, cur, last;
    if (used[s0] || !sweep_step_shape(P, s0, &first)) continue;
    std::vector<int> run{s0};
    last = first;
    for (int s = s0 + 1; s < P.n_steps; ++s) {
      // Only markers of absorbed steps (nothing is launched for them) may lie between two members: the ONE launch of
      // the run sits at its last member's position and reads the first member's input there, which the plan's arena
      // released right after the first member - any launched step in between (the other half of an interleaved
      // left / right chain, say) could have been given that region.  Such a step ends the run.
      if (P.steps[s].kernel == CTN_KERNEL_FUSED) continue;
      if (P.steps[s].lhs != P.steps[run.back()].out && P.steps[s].rhs != P.steps[run.back()].out &&
          P.steps[s].lhs2 != P.steps[run.back()].out)
        break;
      // the consumer of the run's last result: a member if it has the same shape and takes it as its E
      if (P.steps[s].lhs == P.steps[run.back()].out && sweep_step_shape(P, s, &cur) && cur.M == first.M && cur.D == first.D &&
          cur.Pd == first.Pd && cur.ldWl == first.ldWl && cur.ldWp == first.ldWp && cur.ldX == first.ldX && cur.ldA == last.ldC) {
        run.push_back(s);
        last = cur;
        continue;
      }
      break;
    }
    for (int s : run) used[s] = 1;
    if (run.size() > best.size()) { best = run; best_first = first; best_last = last; }
  }
  if (best.size() < 2) return false;
  {
    // the run's result must not land on its own input: blocks of rows start and finish at different times (a launch of
    // more than one round of workgroups), so a block's result rows may only cover ITS OWN input rows - the same region
    // with the same row stride - or nothing of the input at all
    const int idIn = P.steps[best.front()].lhs, idOut = P.steps[best.back()].out;
    const bool in_ws = idIn >= P.n_inputs, out_ws = idOut < P.n_inputs + P.n_steps - 1;
    if (in_ws && out_ws) {
      const int64_t es = P.elem_size();
      const int64_t a0 = P.tensors[idIn].ws_offset, a1 = a0 + ((best_first.M - 1) * best_first.ldA + best_first.D) * es;
      const int64_t b0 = P.tensors[idOut].ws_offset, b1 = b0 + ((best_first.M - 1) * best_last.ldC + best_first.D) * es;
      const bool overlap = a0 < b1 && b0 < a1;
      if (overlap && !(a0 == b0 && best_first.ldA == best_last.ldC)) return false;
    }
  }
  d->on = true; d->steps = best;
  d->ldIn = best_first.ldA; d->ldOut = best_last.ldC; d->ldWl = best_first.ldWl; d->ldWp = best_first.ldWp; d->ldX = best_first.ldX;
  d->J = (int)((best_first.M + SWR - 1) / SWR); d->M = (int)best_first.M; d->D = best_first.D; d->Pd = best_first.Pd;
  return true;
}

// Is k_sweep_f64 taken without CTN_SWEEP=1?  Decided by measurement.
static constexpr bool kSweepF64Default = false;

// The float64 plan keeps a site as TWO steps (plan.cpp fuses them for fp32 only): sa a GEMM of E[b, l] with a network
// input W carrying {l, p, r}, sb the streaming step that sums p against a network input x[b, p].  Can k_sweep_f64 take
// the pair as one site?  Matched on the tensors' labels, dims and strides: E and E' row-major [b][.], r unit-stride in W,
// p unit-stride in x, every stride even (16-byte accesses).  The layout the planner gave C does not matter: C is never
// written.
struct Sweep64Site { int idE = -1, idW = -1, idX = -1, idOut = -1; int64_t ldA = 0, ldC = 0, ldWl = 0, ldWp = 0, ldX = 0, M = 0; int D = 0, Pd = 0; };
static bool sweep64_site_shape(const Plan& P, int sa, int sb, Sweep64Site* sh) {
  if (P.dtype != CTN_F64 || sb + 1 >= P.n_steps) return false;              // a step must follow the last member
  const Step& a = P.steps[sa];
  const Step& b = P.steps[sb];
  if (a.kernel != CTN_KERNEL_MFMA_F64 || b.kernel != CTN_KERNEL_ELEMENT || a.rhs < 0 || b.rhs < 0 || a.lhs2 >= 0 || b.lhs2 >= 0 ||
      a.epw || b.epw)
    return false;
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
  if ((D != 64 && D != 128 && D != 256 && D != 512) || (Pd != 2 && Pd != 4) || tW.dims[axis(tW, lr)] != D || M >= ((int64_t)1 << 31) - SWR)
    return false;
  if (tE.strides[el] != 1 || tW.strides[axis(tW, lr)] != 1 || tX.strides[axis(tX, lp)] != 1 || tO.strides[axis(tO, lr)] != 1) return false;
  const int64_t ldA = tE.strides[1 - el], ldC = tO.strides[axis(tO, lb)], ldX = tX.strides[axis(tX, lb)];
  const int64_t ldWl = tW.strides[axis(tW, ll)], ldWp = tW.strides[axis(tW, lp)];
  if (ldA < D || ldC < D || ldX < Pd || ldWl <= 0 || ldWp <= 0 || ((ldA | ldC | ldX | ldWl | ldWp) & 1)) return false;
  if ((D + 12) * ldWl + 3 * ldWp + D >= ((int64_t)1 << 28)) return false;   // a lane's offsets into a core: 32 bits, in bytes
  sh->idE = idE; sh->idW = idW; sh->idX = idX; sh->idOut = b.out;
  sh->ldA = ldA; sh->ldC = ldC; sh->ldWl = ldWl; sh->ldWp = ldWp; sh->ldX = ldX; sh->M = M; sh->D = (int)D; sh->Pd = (int)Pd;
  return true;
}

// The longest run of such pairs, each taking the result of the one before as its E.  The two safety rules are those of
// sweep_match: nothing that is launched may lie between two members, and the run's result may overlap its input only as
// the same region with the same row stride.
static bool sweep64_match(const Plan& P, Exec::SweepDesc* d) {
  auto next_launched = [&](int s) { do ++s; while (s < P.n_steps && P.steps[s].kernel == CTN_KERNEL_FUSED); return s; };
  std::vector<int> best;
  std::vector<int32_t> best_ids;
  Sweep64Site best_first, best_last;
  std::vector<char> used((size_t)P.n_steps, 0);
  for (int s0 = 0; s0 < P.n_steps; ++s0) {
    Sweep64Site first, cur, last;
    int sb = next_launched(s0);
    if (used[s0] || P.steps[s0].kernel == CTN_KERNEL_FUSED || sb >= P.n_steps || !sweep64_site_shape(P, s0, sb, &first)) continue;
    std::vector<int> run{s0, sb};
    std::vector<int32_t> ids{first.idW, first.idX};
    last = first;
    for (;;) {
      const int na = next_launched(run.back());
      const int nb = na < P.n_steps ? next_launched(na) : na;
      if (nb >= P.n_steps || !sweep64_site_shape(P, na, nb, &cur) || cur.idE != last.idOut || cur.M != first.M || cur.D != first.D ||
          cur.Pd != first.Pd || cur.ldWl != first.ldWl || cur.ldWp != first.ldWp || cur.ldX != first.ldX || cur.ldA != last.ldC)
        break;
      run.push_back(na); run.push_back(nb);
      ids.push_back(cur.idW); ids.push_back(cur.idX);
      last = cur;
    }
    for (int s : run) used[s] = 1;
    if (run.size() > best.size()) { best = run; best_ids = ids; best_first = first; best_last = last; }
  }
  if (best.size() < 4) return false;            // at least 2 sites
  {
    const int idIn = best_first.idE, idOut = best_last.idOut;
    const bool in_ws = idIn >= P.n_inputs, out_ws = idOut < P.n_inputs + P.n_steps - 1;
    if (in_ws && out_ws) {
      const int64_t es = P.elem_size();
      const int64_t a0 = P.tensors[idIn].ws_offset, a1 = a0 + ((best_first.M - 1) * best_first.ldA + best_first.D) * es;
      const int64_t b0 = P.tensors[idOut].ws_offset, b1 = b0 + ((best_first.M - 1) * best_last.ldC + best_first.D) * es;
      const bool overlap = a0 < b1 && b0 < a1;
      if (overlap && !(a0 == b0 && best_first.ldA == best_last.ldC)) return false;
    }
  }
  d->on = true; d->f64 = true; d->steps = best; d->ids = best_ids; d->idIn = best_first.idE;
  d->ldIn = best_first.ldA; d->ldOut = best_last.ldC; d->ldWl = best_first.ldWl; d->ldWp = best_first.ldWp; d->ldX = best_first.ldX;
  d->J = (int)((best_first.M + SWR - 1) / SWR); d->M = (int)best_first.M; d->D = best_first.D; d->Pd = best_first.Pd;
  return true;
}

// Is this split dot step the sum over k = (a, b) of X[a Kb + b] Y[b ldY + a] - one operand contiguous in k, the other
// one its transpose (k_dot_tr)?  Checked on the plan's k tables.
static bool dot_tr_match(const Plan& P, const Step& st, Exec::DotTr* d) {
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
static int ares_match(const Plan& P, int s, int R, int n_cu, const DevSwitches& sw) {
  const Step& st = P.steps[s];
  if (sw.ares == 0 || P.dtype != CTN_F32 || st.kernel != CTN_KERNEL_MFMA_F32 || st.rhs < 0 || st.lhs2 >= 0 || st.epw ||
      st.M != AR_M || st.K != AR_K || st.N % AR_TN != 0 || !st.collapse)
    return 0;
  if (st.modeB != 1 && st.modeB != 2) return 0;
  const int32_t* T = P.tables.data();
  const int32_t *onB = T + st.t.onB, *okB = T + st.t.okB, *onC = T + st.t.onC;
  for (int64_t n = 0; n < st.N; ++n)
    if (onC[n] != onC[n & ~(int64_t)(AR_TN - 1)] + (n & (AR_TN - 1))) return 0;
  if (st.modeB == 1) {
    for (int64_t n = 0; n < st.N; n += 4)
      if (onB[n + 1] != onB[n] + 1 || onB[n + 2] != onB[n] + 2 || onB[n + 3] != onB[n] + 3 || onB[n] % 4) return 0;
  } else {
    for (int k = 0; k < AR_K; k += 4)
      if (okB[k + 1] != okB[k] + 1 || okB[k + 2] != okB[k] + 2 || okB[k + 3] != okB[k] + 3 || okB[k] % 4) return 0;
    for (int64_t n = 0; n < st.N; ++n) if (onB[n] % 4) return 0;
  }
  const int64_t tiles = st.N / AR_TN;       // per batch entry: a workgroup's tiles are tiles of one matrix
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
static bool ares_avec(const Plan& P, int s) {
  const Step& st = P.steps[s];
  if (st.modeA != 2) return false;
  const int32_t* T = P.tables.data();
  const int32_t *omA = T + st.t.omA, *okA = T + st.t.okA, *obA = T + st.t.obA;
  if (obA[0] % 4 || P.tensors[st.lhs].numel % 4) return false;
  for (int k = 0; k < AR_K; ++k) if (okA[k] != okA[0] + k) return false;
  if (okA[0] % 4) return false;
  for (int m = 0; m < AR_M; ++m) if (omA[m] % 4) return false;
  return true;
}

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
static double* part_region(Exec* E, int s) { return E->d_partials + (size_t)E->step_off[s] * E->R; }

// The partials of tensor `id`'s producer - unless the tensor is a network input (or absent), carries scale 1 (eager
// mode: normalised in place), or was never written (CTN_KERNEL_FUSED)
static void producer_partials(Exec* E, int id, const double** p, int32_t* cnt, int32_t* stride, double* numel) {
  const Plan& P = *E->plan;
  *p = nullptr; *cnt = 0; *stride = 0; *numel = 1;
  if (id >= P.n_inputs && P.stabilize && !E->eager_rescale && P.steps[P.tensors[id].producer].kernel != CTN_KERNEL_FUSED) {
    const int ps = P.tensors[id].producer;
    *p = part_region(E, ps);
    *cnt = *stride = E->step_partials[ps];
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
  a.partC_stride = st.collapse ? st.blocks : E->step_partials[s];
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
static void launch_group(Exec* E, const Exec::LeafGroup& G) {
  const dim3 g(G.blocks, E->R, G.len);
  if (E->plan->dtype == CTN_F32) launch_stream_group<float>(G.vw, G.u, g, E->stream, E->d_group_args + G.off);
  else launch_stream_group<double>(G.vw, G.u, g, E->stream, E->d_group_args + G.off);
}

// the last member of a float64 sweep: 2 S member steps, S sites
static int launch_sweep64(Exec* E, int s) {
  const Plan& P = *E->plan;
  const Step& st = P.steps[s];
  const int R = E->R;
  const Exec::SweepDesc& sd = E->sweep;
  const int S = (int)sd.steps.size() / 2;
  Sweep64Args w{};
  w.ptrs = E->d_ptrs; w.n_tensors = E->n_tensors; w.site_ids = E->d_sweep_ids;
  w.idIn = sd.idIn; w.idOut = st.out; w.S = S; w.J = sd.J; w.M = sd.M;
  w.ldIn = sd.ldIn; w.ldOut = sd.ldOut; w.ldWl = sd.ldWl; w.ldWp = sd.ldWp; w.ldX = sd.ldX;
  producer_partials(E, sd.idIn, &w.partIn, &w.PIn, &w.strideIn, &w.numelIn);
  w.min_norm = P.min_norm;
  w.rec_a = E->d_sweep_a; w.rec_e = E->d_sweep_e;
  report_tile(E, s, SWR, sd.D * sd.Pd);   // 16 rows x all columns of C per workgroup, every site
  {
    const dim3 gs((unsigned)sd.J, (unsigned)R);
#define CTN_SWEEP64_LAUNCH(DD)                                                                                        \
    do {                                                                                                              \
      if (sd.Pd == 4) hipLaunchKernelGGL((k_sweep_f64<DD, 4>), gs, dim3(Sweep64Shape<DD>::NT), 0, E->stream, w);      \
      else hipLaunchKernelGGL((k_sweep_f64<DD, 2>), gs, dim3(Sweep64Shape<DD>::NT), 0, E->stream, w);                 \
    } while (0)
    if (sd.D == 64) CTN_SWEEP64_LAUNCH(64);
    else if (sd.D == 128) CTN_SWEEP64_LAUNCH(128);
    else if (sd.D == 256) CTN_SWEEP64_LAUNCH(256);
    else CTN_SWEEP64_LAUNCH(512);
#undef CTN_SWEEP64_LAUNCH
  }
  const double numelE = (double)P.tensors[st.out].numel, numelC = numelE * sd.Pd;
  hipLaunchKernelGGL(k_sweep64_z, dim3((unsigned)(2 * S), (unsigned)R), dim3(256), 0, E->stream, (const double*)E->d_sweep_a,
                     (const int32_t*)E->d_sweep_e, S, sd.J, numelC, numelE, E->d_sweep_z);
  Sweep64Finish f{};
  f.ptrs = E->d_ptrs; f.n_tensors = E->n_tensors; f.idOut = st.out; f.S = S; f.J = sd.J; f.R = R; f.D = sd.D; f.M = sd.M;
  f.ldOut = sd.ldOut; f.Z = E->d_sweep_z; f.rec_e = E->d_sweep_e; f.part_off = E->d_sweep_off;
  f.part_slots = E->d_sweep_slots; f.partials = E->d_partials; f.numelC = numelC; f.numelE = numelE;
  f.min_norm = P.stabilize ? P.min_norm : INFINITY;
  hipLaunchKernelGGL(k_sweep64_finish, dim3((unsigned)sd.J, (unsigned)R), dim3(256), 0, E->stream, f);
  return CTN_OK;
}

// the last member of a sweep: the whole chain, then its scale bookkeeping
static int launch_sweep(Exec* E, int s) {
  const Plan& P = *E->plan;
  const Step& st = P.steps[s];
  const int R = E->R;
  const Exec::SweepDesc& sd = E->sweep;
  const int S = (int)sd.steps.size();
  const Step& f0 = P.steps[sd.steps.front()];
  SweepArgs w{};
  w.ptrs = E->d_ptrs; w.n_tensors = E->n_tensors; w.site_ids = E->d_sweep_ids;
  w.idIn = f0.lhs; w.idOut = st.out; w.S = S; w.J = sd.J; w.M = sd.M;
  w.ldIn = sd.ldIn; w.ldOut = sd.ldOut; w.ldWl = sd.ldWl; w.ldWp = sd.ldWp; w.ldX = sd.ldX;
  producer_partials(E, f0.lhs, &w.partIn, &w.PIn, &w.strideIn, &w.numelIn);
  w.min_norm = P.min_norm;
  w.rec_a = E->d_sweep_a; w.rec_s = E->d_sweep_s; w.dbg = nullptr;
  report_tile(E, s, SWR, sd.D * sd.Pd);   // 16 rows x all columns (1024 at bond 256, d = 4) per workgroup, every site
  const int rc = stamp_buffer(E, s, (size_t)sd.J * R, &w.dbg);
  if (rc != CTN_OK) return rc;
  {
    const dim3 gs((unsigned)sd.J, (unsigned)R);
#define CTN_SWEEP_LAUNCH(DD)                                                                                      \
    do {                                                                                                          \
      if (sd.Pd == 4) hipLaunchKernelGGL((k_sweep_f32<DD, 4>), gs, dim3(DD == 64 ? 256 : 512), 0, E->stream, w);  \
      else hipLaunchKernelGGL((k_sweep_f32<DD, 2>), gs, dim3(DD == 64 ? 256 : 512), 0, E->stream, w);             \
    } while (0)
    if (sd.D == 64) CTN_SWEEP_LAUNCH(64);
    else if (sd.D == 128) CTN_SWEEP_LAUNCH(128);
    else if (sd.D == 256) CTN_SWEEP_LAUNCH(256);
    else CTN_SWEEP_LAUNCH(512);
#undef CTN_SWEEP_LAUNCH
  }
  const double numel = (double)P.tensors[st.out].numel;
  hipLaunchKernelGGL(k_sweep_logs, dim3((unsigned)S, (unsigned)R), dim3(256), 0, E->stream, (const double*)E->d_sweep_a,
                     (const float*)E->d_sweep_s, S, sd.J, E->d_sweep_la, E->d_sweep_ls);
  hipLaunchKernelGGL(k_sweep_z, dim3((unsigned)S, (unsigned)R), dim3(256), 0, E->stream, (const double*)E->d_sweep_la,
                     (const double*)E->d_sweep_ls, S, sd.J, numel, E->d_sweep_z);
  SweepFinish f{};
  f.ptrs = E->d_ptrs; f.n_tensors = E->n_tensors; f.idOut = st.out; f.S = S; f.J = sd.J; f.R = R; f.D = sd.D; f.M = sd.M;
  f.ldOut = sd.ldOut; f.Z = E->d_sweep_z; f.ls = E->d_sweep_ls; f.part_off = E->d_sweep_off;
  f.part_slots = E->d_sweep_slots; f.partials = E->d_partials; f.numel = numel;
  f.min_norm = P.stabilize ? P.min_norm : INFINITY;
  hipLaunchKernelGGL(k_sweep_finish, dim3((unsigned)sd.J, (unsigned)R), dim3(256), 0, E->stream, f);
  return CTN_OK;
}

// a step of a sweep: the members before the last launch nothing, the last one launches the run
static int launch_sweep_member(Exec* E, int s) {
  if (E->sweep_role[s] == 1) return mark_absorbed(E, s);
  const StepTimer t(E, s);
  if (t.rc != CTN_OK) return t.rc;
  const int rc = E->sweep.f64 ? launch_sweep64(E, s) : launch_sweep(E, s);
  return rc != CTN_OK ? rc : t.end();
}

// a zipper pair in its latency form (k_zip_lat): steps (s - 1, s) as one launch, the result leaving as slabs
static int launch_zip_lat(Exec* E, int s) {
  const Plan& P = *E->plan;
  const Step& st = P.steps[s];
  const int R = E->R;
  const Exec::ZipLat& L = E->zl[s];
  const Exec::ZipDesc& zd = L.d;
  const Step& s1 = P.steps[s - 1];
  const int S = ZM / L.mp, nub = zd.U / 16;
  const bool eager = E->eager_rescale;
  ZipLatArgs z{};
  z.ptrs = E->d_ptrs; z.n_tensors = E->n_tensors;
  z.idE = s1.lhs; z.idX = s1.rhs; z.idY = st.rhs;
  z.slabs_in = (L.from_prev && !eager) ? E->d_zl_slab[L.buf ^ 1] : nullptr;
  z.slabs_out = E->d_zl_slab[L.buf];
  z.ldE = zd.ldE; z.ldXq = zd.ldXq; z.ldXk = zd.ldXk; z.ldYq = zd.ldYq; z.ldYm = zd.ldYm;
  z.U = zd.U; z.R = R;
  producer_partials(E, s1.lhs, &z.partE, &z.PE, &z.strideE, &z.numelE);
  z.min_norm = P.min_norm;
  z.partC = part_region(E, s);
  z.partC_stride = E->step_partials[s];
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
    hipLaunchKernelGGL(k_zip_slab_sum, dim3((unsigned)E->step_partials[s], (unsigned)R), dim3(256), 0, E->stream,
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
                       (const double*)part_region(E, s), E->step_partials[s], E->step_partials[s], P.min_norm);
  else
    hipLaunchKernelGGL(k_renorm<double>, g, dim3(256), 0, E->stream, (void* const*)E->d_ptrs, E->n_tensors, out, numel,
                       (const double*)part_region(E, s), E->step_partials[s], E->step_partials[s], P.min_norm);
}

// The zipper-pair kernels by ctn_step_form: threads per workgroup, the tile ctn_exec_step_tile reports, and whether a
// workgroup walks the launch's work items (grid from zipq_grid; else one workgroup per `zu` values of u and replica).
// The tile is 128 (or 64) values of u x all 256 n2 per workgroup; k_zip_f64 (64 values of u) reports (512, 256): an fp64
// step with 128 tile columns reads as k_mfma_f64_g.  k_zip128_f32 (bond 128) reports (512, 64): the 64 values of m1 a
// wave sums; k_zipm64_f32 (bond 64) likewise (256, 32): its 256 threads, 32 values of m1 per wave - a tile no plain
// form reports (theirs are 16 x 16 or have 64 columns at least)
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
};
static_assert(CTN_FORM_ZIP == 1 && CTN_FORM_ZIPQ == 2 && CTN_FORM_ZIP64 == 3 && CTN_FORM_ZIP128 == 4 && CTN_FORM_ZIPM64 == 5 &&
              CTN_FORM_ZIP_F64 == 6 && CTN_FORM_ZIPQP == 7, "kZipKernels is indexed by ctn_step_form");

// a zipper pair: steps (s - 1, s) as one launch
static int launch_zip(Exec* E, int s) {
  const Plan& P = *E->plan;
  const Step& st = P.steps[s];
  const int R = E->R;
  const Exec::ZipDesc& zd = E->zip[s];
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
  z.partC_stride = E->step_partials[s];
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
  const CplxDesc& cd = E->cplx[s];
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
  c.partC_stride = col->on ? col->blocks : E->step_partials[s];
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
  launch_splitk_reduce<float>(E, E->step_partials[s], E->R, a, sk);
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
  if (E->plan->dtype == CTN_F32) launch_splitk_reduce<float>(E, E->step_partials[s], E->R, a, sk);
  else launch_splitk_reduce<double>(E, E->step_partials[s], E->R, a, sk);
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
    const Exec::DotTr dt = (int)E->dot_tr.size() == P.n_steps ? E->dot_tr[s] : Exec::DotTr();
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
  a.partC = part_region(E, s); a.partC_stride = E->step_partials[s];
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
    Exec::LeafGroup& G = E->groups[gc->head];
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
  if (f32 && !E->cplx.empty() && E->cplx[s].on) {
    rc = launch_cplx(E, s, &col);
  } else if (const int ntw_av = f32 && (int)E->ares_ntw.size() == P.n_steps ? E->ares_ntw[s] : 0) {
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
      a.partC_stride = f.collapse ? (int32_t)f.collapse_blocks : E->step_partials[s];
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

// the scales of every step, then the final division
static int launch_finish(Exec* E) {
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
  if (P.dtype == CTN_F32) {
    hipLaunchKernelGGL(k_scales<float>, sg, dim3(256), 0, E->stream, f, E->d_logs);
    hipLaunchKernelGGL(k_finalize<float>, dim3(fb, R), dim3(256), 0, E->stream, f, (const double*)E->d_logs);
  } else {
    hipLaunchKernelGGL(k_scales<double>, sg, dim3(256), 0, E->stream, f, E->d_logs);
    hipLaunchKernelGGL(k_finalize<double>, dim3(fb, R), dim3(256), 0, E->stream, f, (const double*)E->d_logs);
  }
  HIPCHECK(hipGetLastError());
  return CTN_OK;
}

static int exec_launch_steps(Exec* E) {
  const Plan& P = *E->plan;
  int rc = CTN_OK;
  if (P.chain && E->d_chain != nullptr) {
    rc = launch_chain(E);
  } else {
    int group_skip = 0;
    GroupCollect gc;
    for (int s = 0; s < P.n_steps && rc == CTN_OK; ++s) {
      if (group_skip > 0) { --group_skip; continue; }   // went out with the head of its group
      if (gc.left == 0 && !E->groups.empty() && E->groups[s].len >= 2 && E->sw.group && !E->eager_rescale &&
          !(E->timing_runs < E->timing_slots)) {
        const Exec::LeafGroup& G = E->groups[s];
        if (G.ready) {
          launch_group(E, G);
          group_skip = G.len - 1;
          continue;
        }
        gc.left = G.len; gc.head = s;   // first time: the steps' arguments are built by launch_stream, not launched
      }
      if (!E->sweep_role.empty() && E->sweep_role[s] && !E->eager_rescale) rc = launch_sweep_member(E, s);
      else if (!E->zl_skip.empty() && E->zl_skip[s]) rc = mark_absorbed(E, s);   // first step of a pair in its latency form
      else if (!E->zl.empty() && E->zl[s].on) rc = launch_zip_lat(E, s);
      else if (!E->zip_skip.empty() && E->zip_skip[s]) rc = mark_absorbed(E, s); // first step of a zipper pair
      else if (!E->zip.empty() && E->zip[s].on) rc = launch_zip(E, s);
      else if (!E->cplx_skip.empty() && E->cplx_skip[s]) rc = mark_absorbed(E, s);   // the S step of a complex pair
      else if (P.steps[s].kernel == CTN_KERNEL_FUSED) rc = time_nothing(E, s);   // formed on the fly inside its consumer
      else rc = launch_step(E, s, &gc);
    }
  }
  if (rc != CTN_OK) return rc;
  rc = launch_finish(E);
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
static int exec_launch_all(Exec* E) {
  const Plan& P = *E->plan;
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
  for (const Step& st : P.steps) slots += std::max(st.partials, kWaveOutputs);   // (a launcher may retile: upper bound)
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
  const Plan& P = plan->p;
  E.plan = &P; E.device = device; E.R = replicas; E.n_cu = n_cu > 0 ? n_cu : 256;
  E.sw = read_dev_switches();
  E.use_graph = E.sw.graph;
  E.launched_tile.assign(P.n_steps, 0);
  E.launched_form.assign(P.n_steps, 0);
  E.n_tensors = P.n_inputs + P.n_steps + 1;
  auto fail = [&](int code) { delete x; return code; };
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
  {
    size_t slab_elems = 0;   // split-K scratch: S slabs shaped like the step's output, per replica
    // the splits the launcher will take: it asks step_form too, and the answer does not depend on the caller's buffers
    auto splits_of = [&](int s) { return step_form(P, s, replicas, E.n_cu, E.sw, P.steps[s].cvec).S; };
    for (int s = 0; s < P.n_steps; ++s)
      if (const int S = splits_of(s))
        slab_elems = std::max(slab_elems, (size_t)S * (size_t)P.tensors[P.steps[s].out].numel * (size_t)replicas);
    if (slab_elems) HIPCHECK_X(hipMalloc((void**)&E.d_slab, slab_elems * (P.dtype == CTN_F64 ? 8 : 4)));
    size_t fold_elems = 0;   // a step with more than 16 slabs folds them 16 to 1 into this buffer and back
    for (int s = 0; s < P.n_steps; ++s)
      if (const int S = splits_of(s))
        if (S > 16)
          fold_elems = std::max(fold_elems, (size_t)((S + 15) / 16) * (size_t)P.tensors[P.steps[s].out].numel * (size_t)replicas);
    if (fold_elems) HIPCHECK_X(hipMalloc((void**)&E.d_slab2, fold_elems * (P.dtype == CTN_F64 ? 8 : 4)));
  }
  // partial counts: plan value, one per tile in the latency form, and the split-K reduce pass spreads over up to
  // 64 workgroups per replica; every step gets a region of exactly that many slots per replica
  E.step_partials.resize(P.n_steps);
  E.step_off.resize(P.n_steps);
  int64_t scratch_need = std::max<int64_t>(P.max_collapse_blocks, 1);
  for (int s = 0; s < P.n_steps; ++s) {
    const Step& st = P.steps[s];
    E.step_partials[s] = std::max(st.partials, 1);
    if (P.chain) { E.step_off[s] = E.part_slots++; continue; }   // the chain walker: one slot per step, whatever the kernel kind
    // (a step with S > 0 has made d_slab non-null just above, and the launcher drops no split for want of it)
    const StepForm f = step_form(P, s, replicas, E.n_cu, E.sw, st.cvec);
    E.step_partials[s] = f.partials;
    scratch_need = std::max<int64_t>(scratch_need, f.collapse_blocks);
    E.step_off[s] = E.part_slots;
    E.part_slots += E.step_partials[s];
  }
  // zipper pairs: at least one full round of workgroups (each is 134 MFLOP long), or CTN_ZIP=1
  if (!P.chain && E.sw.zip != 0) {
    E.zip.assign(P.n_steps, Exec::ZipDesc());
    E.zip_skip.assign(P.n_steps, 0);
    bool any = false;
    for (int s = 1; s + 1 < P.n_steps; ++s) {
      Exec::ZipDesc z;
      if (E.zip_skip[s - 1] || (s >= 2 && E.zip[s - 1].on)) continue;
      // 128 values of u per workgroup (k_zip_f32) when that fills the chip - or CTN_ZIP=1; else 64 (k_zip64_f32) when THAT
      // does: 64 ... 127 networks of |u| = 256 - or CTN_ZIP=2; fewer networks keep the two-launch / latency forms
      // ... and of the two the one whose workgroups fill their rounds better (one workgroup per CU and round: 96 networks
      // are 192 workgroups of 128 - refused - or 384 of 64 - a round and a half: 26.0 ms against 23.0 on the two-launch
      // forms - while 64 networks are exactly one round of 64: 13.5 ms against 15.9)
      auto fill = [&](int64_t wgs) { return (double)wgs / (double)(((wgs + E.n_cu - 1) / E.n_cu) * E.n_cu); };
      Exec::ZipDesc z128, z64;
      if (P.dtype == CTN_F64) {
        // fp64: one form, 64 values of u per workgroup (k_zip_f64), and only on request (CTN_ZIP=1).  kZipF64Default is
        // where the rule of the fp32 forms - at least one round of workgroups, rounds filled to 0.9 - would switch it on
        // unasked; the measurement that has to decide that is in DESIGN section 10.
        if (E.sw.zip == 2 || !zip_match(P, s, &z, CTN_F64, ZDU)) continue;
        const int64_t wgs = (int64_t)(z.U / ZDU) * replicas;
        if (E.sw.zip != 1 && !(kZipF64Default && wgs >= E.n_cu && fill(wgs) >= 0.9)) continue;
        if (z.U / ZDU > kMaxPartials) continue;
        z.zu = ZDU; z.form = CTN_FORM_ZIP_F64;
        E.zip[s] = z;
        E.zip_skip[s - 1] = 1;
        any = true;
        E.part_slots -= E.step_partials[s];
        E.step_partials[s] = z.U / z.zu;
        E.part_slots += E.step_partials[s];
        continue;
      }
      const bool m128 = E.sw.zip != 2 && zip_match(P, s, &z128, CTN_F32) && (E.sw.zip == 1 || (int64_t)(z128.U / ZU) * replicas >= E.n_cu);
      const bool m64 = E.sw.zip != 1 && zip_match(P, s, &z64, CTN_F32, Z6U) && z64.K1 % Z6K == 0 &&
                       (E.sw.zip == 2 || (int64_t)(z64.U / Z6U) * replicas >= E.n_cu);
      const double f128 = m128 ? fill((int64_t)(z128.U / ZU) * replicas) : 0.0, f64 = m64 ? fill((int64_t)(z64.U / Z6U) * replicas) : 0.0;
      bool ok = false;
      if (m128 && (E.sw.zip == 1 || f128 >= 0.9 || f128 >= f64)) { ok = true; z = z128; z.zu = ZU; z.form = CTN_FORM_ZIP; }
      else if (m64 && (E.sw.zip == 2 || f64 >= 0.9)) { ok = true; z = z64; z.zu = Z6U; z.form = CTN_FORM_ZIP64; }
      else if (m128) { ok = true; z = z128; z.zu = ZU; z.form = CTN_FORM_ZIP; }
      // the 128-u form with two legs per pass (k_zipq_f32): on request wherever the pair matches (CTN_ZIPQ=1, also where
      // the rules above chose otherwise - but not against CTN_ZIP=2), else under k_zip_f32's own default rule
      // ... and its walking form (k_zipqp_f32): on request (CTN_ZIPQ=2) wherever CTN_ZIPQ=1 takes k_zipq_f32, else under
      // kZipQPDefault where that kernel is taken by default and has two rounds of workgroups at least
      if ((E.sw.zipq == 1 || E.sw.zipq == 2) && E.sw.zip != 2 && zip_match(P, s, &z128, CTN_F32) && zipq_fits(z128)) {
        ok = true; z = z128; z.zu = ZU; z.zq = true; z.zqp = E.sw.zipq == 2;
        z.form = z.zqp ? CTN_FORM_ZIPQP : CTN_FORM_ZIPQ;
      } else if (E.sw.zipq == -1 && kZipQDefault && E.sw.zip == -1 && ok && z.zu == ZU && f128 >= 0.9 && zipq_fits(z)) {
        z.zq = true;
        z.zqp = kZipQPDefault && zipq_items(replicas, z.U, ZU) >= 2 * (int64_t)E.n_cu;
        z.form = z.zqp ? CTN_FORM_ZIPQP : CTN_FORM_ZIPQ;
      }
      // bond 128 (k_zip128_f32: 128 values of u per workgroup, K1 a multiple of its tile depth and two tiles at least -
      // ZK = Z1K, as zip_match checks), when no bond-256 form matches: only on request (CTN_ZIP=1, and not CTN_ZIP128=0).
      // kZip128Default is where the rule of the other forms - at least one round of workgroups, rounds filled to 0.9 - would switch it on unasked;
      // the measurement that has to decide that is in DESIGN section 10.
      static_assert(Z1K == ZK, "zip_match checks K1 against ZK; k_zip128_f32's tile depth must be the same");
      if (!m128 && !m64 && E.sw.zip128 != 0 && E.sw.zip != 0 && E.sw.zip != 2 && zip_match(P, s, &z, CTN_F32, Z1U, Z1M) &&
          z.K1 % Z1K == 0 && z.K1 >= 2 * Z1K && ((z.ldE | z.ldXq | z.ldXk | z.ldYq | z.ldYm | z.ldC) & 3) == 0 &&
          (E.sw.zip == 1 || (kZip128Default && (int64_t)(z.U / Z1U) * replicas >= E.n_cu && fill((int64_t)(z.U / Z1U) * replicas) >= 0.9))) {
        ok = true; z.zu = Z1U; z.zm = Z1M; z.form = CTN_FORM_ZIP128;
      }
      // bond 64 (k_zipm64_f32: 64 values of u per workgroup, the same tile depth), when neither a bond-256 nor the bond-128
      // form matches: only on request (CTN_ZIP=1, and not CTN_ZIPM64=0).  kZipM64Default as kZip128Default: the
      // measurement that has to decide it is in DESIGN section 10.
      static_assert(Z4K == ZK, "zip_match checks K1 against ZK; k_zipm64_f32's tile depth must be the same");
      if (!ok && E.sw.zipm64 != 0 && E.sw.zip != 0 && E.sw.zip != 2 && zip_match(P, s, &z, CTN_F32, Z4U, Z4M) &&
          z.K1 % Z4K == 0 && z.K1 >= 2 * Z4K && ((z.ldE | z.ldXq | z.ldXk | z.ldYq | z.ldYm | z.ldC) & 3) == 0 &&
          (E.sw.zip == 1 || (kZipM64Default && (int64_t)(z.U / Z4U) * replicas >= E.n_cu && fill((int64_t)(z.U / Z4U) * replicas) >= 0.9))) {
        ok = true; z.zu = Z4U; z.zm = Z4M; z.form = CTN_FORM_ZIPM64;
      }
      if (!ok || z.U / z.zu > kMaxPartials) continue;    // (one abs-sum partial per workgroup: the consumers add at most that many)
      E.zip[s] = z;
      E.zip_skip[s - 1] = 1;
      any = true;
      // one abs-sum partial per workgroup of the fused launch; the skipped step keeps its (never written, zero) slots
      E.part_slots -= E.step_partials[s];
      E.step_partials[s] = z.U / z.zu;
      E.part_slots += E.step_partials[s];
    }
    if (any) {   // regions moved: lay the offsets out again
      E.part_slots = 0;
      for (int s = 0; s < P.n_steps; ++s) { E.step_off[s] = E.part_slots; E.part_slots += E.step_partials[s]; }
    } else {
      E.zip.clear(); E.zip_skip.clear();
    }
  }
  // the same pairs in their latency form: a few networks in flight (or CTN_ZIPL=1), and no throughput-form pair taken
  if (!P.chain && P.dtype == CTN_F32 && E.zip.empty() && E.sw.zipl != 0 && (E.sw.zipl == 1 || replicas <= E.sw.zipl_max_r)) {
    E.zl.assign(P.n_steps, Exec::ZipLat());
    E.zl_skip.assign(P.n_steps, 0);
    bool any = false;
    int64_t slab_elems = 0;
    for (int s = 1; s + 1 < P.n_steps; ++s) {
      Exec::ZipDesc z;
      if (E.zl_skip[s - 1] || (s >= 2 && E.zl[s - 1].on) || !zip_match(P, s, &z, CTN_F32, 16)) continue;
      if (z.K1 != ZM || (z.Q != 4 && z.Q != 2) || z.ldC % 4 || z.ldE % 4 || z.ldXk % 4 || z.ldXq % 4 || z.ldYm % 4 || z.ldYq % 4) continue;
      // the part of m1 a workgroup owns: 32 (8 slabs, 128 workgroups per network at |u| = 256) while that still fits ONE
      // round of workgroups, else 64 (4 slabs, half the workgroups, each with twice the work per byte it loads)
      int mp = 64;
      if (z.Q == 4 && (E.sw.zipl_mp == 32 || (E.sw.zipl_mp == 0 && (int64_t)replicas * (z.U / 16) * 8 <= E.n_cu))) mp = 32;
      const int S = ZM / mp;
      if ((z.U / 16) * S > kMaxPartials) continue;
      E.zl[s].on = true; E.zl[s].d = z; E.zl[s].mp = mp;
      E.zl_skip[s - 1] = 1;
      any = true;
      slab_elems = std::max<int64_t>(slab_elems, (int64_t)S * z.U * ZM);
      E.step_partials[s] = (z.U / 16) * S;        // one abs-sum partial per workgroup (of its slab piece)
    }
    if (any) {
      for (int s = 3; s + 1 < P.n_steps; ++s) {   // links of the chain: the pair (s - 1, s) takes the result of the pair (s - 3, s - 2)
        if (!E.zl[s].on || !E.zl[s - 2].on || P.steps[s - 1].lhs != P.steps[s - 2].out) continue;
        if (E.zl[s - 2].d.U != ZM || E.zl[s - 2].mp != E.zl[s].mp || E.zl[s - 2].d.ldC != E.zl[s].d.ldE) continue;
        E.zl[s].from_prev = true;
        E.zl[s].buf = E.zl[s - 2].buf ^ 1;
        E.zl[s - 2].feeds_next = true;
      }
      E.part_slots = 0;
      for (int s = 0; s < P.n_steps; ++s) { E.step_off[s] = E.part_slots; E.part_slots += E.step_partials[s]; }
      for (int i = 0; i < 2; ++i) HIPCHECK_X(hipMalloc((void**)&E.d_zl_slab[i], (size_t)replicas * slab_elems * 4));
    } else {
      E.zl.clear(); E.zl_skip.clear();
    }
  }
  // complex x complex step pairs (k_cmfma_f32): only on request (CTN_CPLX=1) while kCplxDefault is off
  if (!P.chain && P.dtype == CTN_F32 && (E.sw.cplx == 1 || (kCplxDefault && E.sw.cplx != 0))) {
    E.cplx.assign(P.n_steps, CplxDesc());
    E.cplx_skip.assign(P.n_steps, 0);
    std::vector<int32_t> tabs;
    bool any = false;
    for (int s = 1; s < P.n_steps; ++s) {
      if ((!E.zip.empty() && (E.zip[s].on || E.zip_skip[s])) || (!E.zl.empty() && (E.zl[s].on || E.zl_skip[s])))
        continue;      // (a zipper pair is two GEMM steps: its members never have an S step behind them)
      CplxDesc cd;
      if (!cplx_match(P, s, &cd, &tabs)) continue;
      const int64_t tiles = (int64_t)((cd.Mx + CX_TX - 1) / CX_TX) * ((cd.Ny + CX_TY - 1) / CX_TY);
      E.cplx[s] = cd;
      E.cplx_skip[cd.sp] = 1;
      any = true;
      // one abs-sum partial per workgroup of the fused launch (beyond the slots: collapsed to one); the skipped S step
      // keeps its (never written, zero) slots: its rescale reads 0.0
      E.step_partials[s] = tiles > kMaxPartials ? 1 : (int)tiles;
      scratch_need = std::max<int64_t>(scratch_need, tiles);
    }
    if (any) {
      E.part_slots = 0;
      for (int s = 0; s < P.n_steps; ++s) { E.step_off[s] = E.part_slots; E.part_slots += E.step_partials[s]; }
      HIPCHECK_X(hipMalloc((void**)&E.d_cplx_tabs, tabs.size() * 4));
      HIPCHECK_X(hipMemcpy(E.d_cplx_tabs, tabs.data(), tabs.size() * 4, hipMemcpyHostToDevice));
    } else {
      E.cplx.clear(); E.cplx_skip.clear();
    }
  }
  // full dots against a transposed tensor
  if (!P.chain && E.sw.dot_tr) {
    E.dot_tr.assign(P.n_steps, Exec::DotTr());
    bool any = false;
    for (int s = 0; s < P.n_steps; ++s) any = dot_tr_match(P, P.steps[s], &E.dot_tr[s]) || any;
    if (!any) E.dot_tr.clear();
  }
  // steps with a resident left operand (k_mfma_f32_ares)
  if (!P.chain && E.sw.ares != 0 && P.dtype == CTN_F32) {
    E.ares_ntw.assign(P.n_steps, 0);
    bool any = false;
    for (int s = 0; s < P.n_steps; ++s) { E.ares_ntw[s] = ares_match(P, s, replicas, E.n_cu, E.sw);
      if (E.ares_ntw[s] && ares_avec(P, s)) E.ares_ntw[s] |= 1 << 16;
      any = any || E.ares_ntw[s];
    }
    if (!any) E.ares_ntw.clear();
  }
  // a sweep: at least half a chip of row blocks, or CTN_SWEEP=1
  if (!P.chain && E.sw.sweep != 0 && P.stabilize) {
    Exec::SweepDesc sd;
    // (bonds up to 128: the per-site launches are a few microseconds of latency each whatever the batch - always)
    if (sweep_match(P, &sd) && (int)sd.steps.size() <= kSweepMaxSites &&
        (E.sw.sweep == 1 || (sd.steps.size() >= 4 && (sd.D <= 128 || (int64_t)sd.J * replicas * 2 >= E.n_cu)))) {
      E.sweep = sd;
      const int S = (int)sd.steps.size();
      E.sweep_role.assign(P.n_steps, 0);
      std::vector<int32_t> ids((size_t)S * 2), slots((size_t)S);
      std::vector<int64_t> offs((size_t)S);
      for (int i = 0; i < S; ++i) {
        const int s = sd.steps[i];
        E.sweep_role[s] = i + 1 == S ? 2 : 1;
        ids[2 * i] = P.steps[s].rhs; ids[2 * i + 1] = P.steps[s].lhs2;
        offs[i] = E.step_off[s]; slots[i] = E.step_partials[s];
      }
      HIPCHECK_X(hipMalloc((void**)&E.d_sweep_ids, ids.size() * 4));
      HIPCHECK_X(hipMemcpy(E.d_sweep_ids, ids.data(), ids.size() * 4, hipMemcpyHostToDevice));
      HIPCHECK_X(hipMalloc((void**)&E.d_sweep_off, offs.size() * 8));
      HIPCHECK_X(hipMemcpy(E.d_sweep_off, offs.data(), offs.size() * 8, hipMemcpyHostToDevice));
      HIPCHECK_X(hipMalloc((void**)&E.d_sweep_slots, slots.size() * 4));
      HIPCHECK_X(hipMemcpy(E.d_sweep_slots, slots.data(), slots.size() * 4, hipMemcpyHostToDevice));
      const size_t nrec = (size_t)replicas * S * sd.J;
      HIPCHECK_X(hipMalloc((void**)&E.d_sweep_a, nrec * 8));
      HIPCHECK_X(hipMalloc((void**)&E.d_sweep_s, nrec * 4));
      HIPCHECK_X(hipMalloc((void**)&E.d_sweep_z, (size_t)replicas * S * 8));
      HIPCHECK_X(hipMalloc((void**)&E.d_sweep_la, nrec * 8));
      HIPCHECK_X(hipMalloc((void**)&E.d_sweep_ls, nrec * 8));
    } else if (P.dtype == CTN_F64 && E.sw.sweep64 != 0 && (E.sw.sweep == 1 || kSweepF64Default) && sweep64_match(P, &sd) &&
               (int)sd.steps.size() <= 2 * kSweepMaxSites) {
      // float64 (k_sweep_f64): the run's 2 S steps are all members - a GEMM and a streaming step per site
      E.sweep = sd;
      const int T = (int)sd.steps.size(), S = T / 2;
      E.sweep_role.assign(P.n_steps, 0);
      std::vector<int32_t> slots((size_t)T);
      std::vector<int64_t> offs((size_t)T);
      for (int i = 0; i < T; ++i) {
        const int s = sd.steps[i];
        E.sweep_role[s] = i + 1 == T ? 2 : 1;
        offs[i] = E.step_off[s]; slots[i] = E.step_partials[s];
      }
      HIPCHECK_X(hipMalloc((void**)&E.d_sweep_ids, sd.ids.size() * 4));
      HIPCHECK_X(hipMemcpy(E.d_sweep_ids, sd.ids.data(), sd.ids.size() * 4, hipMemcpyHostToDevice));
      HIPCHECK_X(hipMalloc((void**)&E.d_sweep_off, offs.size() * 8));
      HIPCHECK_X(hipMemcpy(E.d_sweep_off, offs.data(), offs.size() * 8, hipMemcpyHostToDevice));
      HIPCHECK_X(hipMalloc((void**)&E.d_sweep_slots, slots.size() * 4));
      HIPCHECK_X(hipMemcpy(E.d_sweep_slots, slots.data(), slots.size() * 4, hipMemcpyHostToDevice));
      const size_t nrec = (size_t)replicas * S * sd.J;
      HIPCHECK_X(hipMalloc((void**)&E.d_sweep_a, 2 * nrec * 8));
      HIPCHECK_X(hipMalloc((void**)&E.d_sweep_e, nrec * 4));
      HIPCHECK_X(hipMalloc((void**)&E.d_sweep_z, (size_t)replicas * T * 8));
    }
  }
  // leaf groups: runs of consecutive plain streaming steps on network inputs, same kernel variant (see Exec::LeafGroup)
  if (!P.chain && E.sw.group) {
    E.groups.assign(P.n_steps, Exec::LeafGroup());
    auto leaf = [&](int s, int* vw, int* u) {
      const Step& st = P.steps[s];
      if (st.kernel != CTN_KERNEL_ELEMENT || st.kvec || st.collapse || s + 1 >= P.n_steps || st.rhs < 0 ||
          st.lhs >= P.n_inputs || st.rhs >= P.n_inputs || st.lhs2 >= 0 || stream_splits(st, replicas, E.n_cu) ||
          (!E.cplx_skip.empty() && E.cplx_skip[s]))      // (the S step of a complex pair is never launched)
        return false;
      int64_t nq;
      *vw = st.vecw;
      stream_variant(st, replicas, *vw, u, &nq);
      return true;
    };
    int total = 0;
    for (int s = 0; s < P.n_steps;) {
      int vw, u;
      if (!leaf(s, &vw, &u)) { ++s; continue; }
      int e = s + 1, blocks = P.steps[s].blocks, vw2, u2;
      while (e < P.n_steps && e - s < 1024 && leaf(e, &vw2, &u2) && vw2 == vw && u2 == u) { blocks = std::max(blocks, P.steps[e].blocks); ++e; }
      if (e - s >= 2) {
        Exec::LeafGroup& G = E.groups[s];
        G.len = e - s; G.vw = vw; G.u = u; G.blocks = blocks; G.off = total;
        total += G.len;
      }
      s = e;
    }
    if (total) {
      HIPCHECK_X(hipHostMalloc((void**)&E.h_group_args, sizeof(StepArgs) * (size_t)total, hipHostMallocDefault));
      HIPCHECK_X(hipMalloc((void**)&E.d_group_args, sizeof(StepArgs) * (size_t)total));
    } else {
      E.groups.clear();
    }
  }
  HIPCHECK_X(hipMalloc((void**)&E.d_scratch, (size_t)replicas * scratch_need * 8));
  HIPCHECK_X(hipMalloc((void**)&E.d_partials, (size_t)E.part_slots * replicas * 8));
  HIPCHECK_X(hipMemset(E.d_partials, 0, (size_t)E.part_slots * replicas * 8));
  {
    std::vector<int32_t> slots(E.step_partials.begin(), E.step_partials.end());
    HIPCHECK_X(hipMalloc((void**)&E.d_stepOff, P.n_steps * 8));
    HIPCHECK_X(hipMalloc((void**)&E.d_stepSlots, P.n_steps * 4));
    HIPCHECK_X(hipMemcpy(E.d_stepOff, E.step_off.data(), P.n_steps * 8, hipMemcpyHostToDevice));
    HIPCHECK_X(hipMemcpy(E.d_stepSlots, slots.data(), P.n_steps * 4, hipMemcpyHostToDevice));
  }
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
    sp[s] = P.steps[s].kernel == CTN_KERNEL_FUSED ? 0 : E.step_partials[s];   // no partials: rescale reported as 0.0
    sn[s] = (double)P.tensors[P.steps[s].out].numel;
  }
  HIPCHECK_X(hipMalloc((void**)&E.d_stepP, P.n_steps * 4));
  HIPCHECK_X(hipMalloc((void**)&E.d_stepNumel, P.n_steps * 8));
  HIPCHECK_X(hipMemcpy(E.d_stepP, sp.data(), P.n_steps * 4, hipMemcpyHostToDevice));
  HIPCHECK_X(hipMemcpy(E.d_stepNumel, sn.data(), P.n_steps * 8, hipMemcpyHostToDevice));
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
    HIPCHECK_X(hipMalloc((void**)&E.d_chain, cs.size() * sizeof(ChainStep)));
    HIPCHECK_X(hipMemcpy(E.d_chain, cs.data(), cs.size() * sizeof(ChainStep), hipMemcpyHostToDevice));
    // the on-chip walker, where asked for and where the packer takes the plan (a refusal keeps k_chain)
    if (E.sw.chain == 2 || (kChainLdsDefault && E.sw.chain != 1)) {
      ChainProgram cp;
      std::string why;
      if (chain_pack(P, &cp, &why)) {
        HIPCHECK_X(hipMalloc((void**)&E.d_chain_prog, cp.words.size() * 4));
        HIPCHECK_X(hipMemcpy(E.d_chain_prog, cp.words.data(), cp.words.size() * 4, hipMemcpyHostToDevice));
        E.chain_len0 = cp.steps[0].len;
      }
    }
  }
  // k_zipqp_f32: a result that would overwrite the pair's E moves to a side buffer.  A buffer is free again once the
  // step that consumes its tensor has been launched (every intermediate is consumed exactly once): a chain needs two.
  if (!E.zip.empty()) {
    const int64_t es = P.elem_size();
    std::vector<int> busy_until;                        // per side buffer: the step that reads what it holds
    for (int s = 1; s + 1 < P.n_steps; ++s) {
      if (!E.zip[s].on || !E.zip[s].zqp) continue;
      const int idE = P.steps[s - 1].lhs, idC = P.steps[s].out;
      if (idE < P.n_inputs) continue;
      const int64_t e0 = P.tensors[idE].ws_offset, e1 = e0 + P.tensors[idE].numel * es;
      const int64_t c0 = P.tensors[idC].ws_offset, c1 = c0 + P.tensors[idC].numel * es;
      const bool e_in_ws = E.zqp_side.empty() || E.zqp_side[idE] < 0;       // (an E that moved itself is out of the way)
      if (!e_in_ws || c0 >= e1 || e0 >= c1) continue;
      if (E.zqp_side.empty()) E.zqp_side.assign((size_t)E.n_tensors, -1);
      int consumer = P.n_steps;
      for (int c = s + 1; c < P.n_steps; ++c)
        if (P.steps[c].lhs == idC || P.steps[c].rhs == idC || P.steps[c].lhs2 == idC) { consumer = c; break; }
      int k = 0;
      while (k < (int)busy_until.size() && busy_until[k] >= s - 1) ++k;      // (E's own buffer is read by step s - 1)
      if (k == (int)busy_until.size()) busy_until.push_back(0);
      busy_until[k] = consumer;
      E.zqp_side[idC] = k;
      E.zqp_side_bytes = std::max<int64_t>(E.zqp_side_bytes, (c1 - c0 + 255) / 256 * 256);
    }
    if (!busy_until.empty())
      HIPCHECK_X(hipMalloc((void**)&E.d_zqp_side, (size_t)E.zqp_side_bytes * busy_until.size() * replicas));
  }
  // pointer table: intermediates and the ones-scalar are fixed for the executor's lifetime
  E.h_ptrs.assign((size_t)replicas * E.n_tensors, nullptr);
  for (int r = 0; r < replicas; ++r) {
    void** row = E.h_ptrs.data() + (size_t)r * E.n_tensors;
    for (int id = P.n_inputs; id < P.n_inputs + P.n_steps - 1; ++id)
      row[id] = E.zqp_side.empty() || E.zqp_side[id] < 0
                    ? E.d_ws + (size_t)r * P.ws_bytes_per_replica + P.tensors[id].ws_offset
                    : E.d_zqp_side + ((size_t)E.zqp_side[id] * replicas + r) * E.zqp_side_bytes;
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
      if (!E->zip_skip.empty() && E->zip_skip[s]) continue;          // runs inside the next step's launch
      if (!E->zl_skip.empty() && E->zl_skip[s]) continue;
      if (!E->cplx_skip.empty() && E->cplx_skip[s]) continue;
      if (!E->sweep_role.empty() && E->sweep_role[s] && !E->eager_rescale) {   // a sweep keeps its products in range by itself
        if (!std::isfinite(rs[s])) return true;
        continue;
      }
      double sab = scale_of(st.lhs) * (st.rhs >= 0 ? scale_of(st.rhs) : 1.0) * (st.lhs2 >= 0 ? scale_of(st.lhs2) : 1.0);
      if ((!E->zip.empty() && E->zip[s].on) || (!E->zl.empty() && E->zl[s].on))   // the fused pair accumulates on E, X and Y as stored
        sab = scale_of(P.steps[s - 1].lhs) * scale_of(P.steps[s - 1].rhs) * scale_of(st.rhs);
      if (!E->cplx.empty() && E->cplx[s].on)                         // the complex pair accumulates on `small` and `big` as stored
        sab = scale_of(E->cplx[s].small) * scale_of(E->cplx[s].big);
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
