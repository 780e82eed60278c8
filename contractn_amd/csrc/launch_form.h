// launch_form.h - which kernel a plain step of a plan runs on, for a given number of networks in flight and chip size.
// Pure host code (no HIP, no kernel header): the development switches, the selection functions with the measurements
// behind them, and step_form(), the ONE place that walks them in order.  engine.hip calls step_form() when an executor is
// created (slab buffers, partial-sum regions, collapse scratch) and again on every eager enqueue (the launch itself).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>

#include "ctn_abi.h"
#include "plan.h"

namespace ctn {

// Development switches: every environment variable the library looks at, read in ONE place, once per executor
// (ctn_exec_create) - never on the launch path.  None is needed in production ("Development switches").
struct DevSwitches {
  int mfma_g = 1;        // CTN_MFMA_G: 0 never use the large-tile LDS-DMA kernels, 1 when a launch fills the chip, 2 whenever eligible (tests)
  int graph = 1;         // CTN_GRAPH=0: every enqueue issues its launches one by one
  int mfma_bk = 0;       // CTN_MFMA_BK=16|32: force the k-tile depth of k_mfma_f32
  int group = 1;         // CTN_GROUP=0: never batch independent leaf steps into one launch (k_stream_group)
  int halve = 1;         // CTN_HALVE_TILES=0: never halve the tiles of an under-filled register-staged launch
  int lat_wg_per_cu_x2 = 2;  // CTN_LAT_WG_X2: twice the workgroups per CU up to which the one-launch latency form is taken
  int lat_max_t = 64;    // CTN_LAT_MAX_T=32: no 64 x 64 form of the one-launch latency kernel
  int splitk_fill_long = 2;  // CTN_SPLITK_FILL_LONG: K >= 1024 steps are split until 64 x 64 tiles give this many workgroups per CU
  int lat64_min_k = 512; // CTN_LAT64_MIN_K: least K for the 64 x 64 one-launch latency form when an operand is k-contiguous
  int splitk = -1;       // CTN_SPLITK: 0 disables the latency mode, 1 forces it for every eligible step (tests)
  int splitk_max = 0;    // CTN_SPLITK_MAX: tile-count threshold of the latency mode
  int lat = -1;          // CTN_LAT: 0 never use the one-launch latency form (k_mfma_f32_lat), 1 whenever the shape allows (tests)
  int hform = -1;        // CTN_H: 0 never use the one-tile-per-CU form (k_mfma_f32_h), 1 whenever the shape allows (tests)
  int sweep = -1;        // CTN_SWEEP: 0 never walk a chain of epilogue-summed steps in one launch (k_sweep_f32), 1 whenever one matches (tests)
  int sweep64 = 1;       // CTN_SWEEP64=0: never the float64 sweep (k_sweep_f64), which CTN_SWEEP=1 takes on a float64 plan whose
                         // per-site step pairs (a GEMM and the streaming sum over p) match
  int sweep_small = -1;  // CTN_SWEEP_SMALL: 1 a float32 batched MPS of bond 8 ... 64 is walked in one launch (k_sweep_small<float>) wherever
                         // sweep_small_match takes it, k_sweep_f32 does not and CTN_SWEEP is not 0; 0 or unset: never (kSweepSmallDefault)
  int sweep_small64 = -1;  // CTN_SWEEP_SMALL64: 1 a float64 batched MPS of bond 8 ... 64 is walked in one launch (k_sweep_small<double>)
                         // wherever sweep_small_match takes it, k_sweep_f64 does not and neither CTN_SWEEP nor CTN_SWEEP64 is 0;
                         // 0 or unset: never (kSweepSmallF64Default).  CTN_SWEEP_SMALL does not reach a float64 plan, nor this a float32 one
  int sweep_small_tr = 1;  // CTN_SWEEP_SMALL_TR=0: never a run of TRANSPOSED cores (the bond contracted with the state unit-stride:
                         // k_sweep_small<.., TR = true>), which CTN_SWEEP_SMALL=1 / CTN_SWEEP_SMALL64=1 take as they take the forward ones
  int dot_tr = 1;        // CTN_DOT_TR=0: full dots against a transposed tensor stay on k_dot_split's 4-byte gathers
  int zip = -1;          // CTN_ZIP: 0 never fuse a zipper's two GEMM steps into one launch (k_zip_f32), 1 whenever the pair matches
                         // (tests), 2 likewise with 64 values of u per workgroup (k_zip64_f32).  fp64 plans: 1 the fp64 pair kernel
                         // (k_zip_f64) whenever the pair matches; 2 has no fp64 meaning and keeps the two-launch path
  int zipq = -1;         // CTN_ZIPQ: 0 never the two-legs-per-pass form of the bond-256 pair (k_zipq_f32), 1 whenever the pair matches it
                         // (zip_match and Q even - tests), 2 likewise its form that walks several work items per workgroup
                         // (k_zipqp_f32), unset: kZipQDefault where k_zip_f32 is taken by its own default rule, and of the two
                         // forms k_zipqp_f32 under kZipQPDefault from two rounds of workgroups on
  int zipq_wgs = 0;      // CTN_ZIPQ_WGS=n: at most n workgroups per k_zipqp_f32 launch (1 ... CUs; tests and experiments: a small
                         // launch crosses item seams only under a cap); never part of the default rule
  int zip128 = 1;        // CTN_ZIP128=0: never the bond-128 pair kernel (k_zip128_f32), which CTN_ZIP=1 takes for fp32 pairs with
                         // |m1| = |n2| = 128 that no bond-256 form matches
  int zipm64 = 1;        // CTN_ZIPM64=0: never the bond-64 pair kernel (k_zipm64_f32), which CTN_ZIP=1 takes for fp32 pairs with
                         // |m1| = |n2| = 64 (no bond-256 and no bond-128 form matches those)
  int zip512 = 1;        // CTN_ZIP512=0: never the bond-512 pair kernel (k_zip512_f32), which CTN_ZIP=1 takes for fp32 pairs with
                         // |m1| = |n2| = 512 (no other form matches those)
  int cplx = -1;         // CTN_CPLX: 1 a complex x complex step pair - the S step and the 4-byte-gather GEMM behind it - runs as one launch
                         // (k_cmfma_f32) wherever cplx_match takes it; 0 or unset: never (kCplxDefault)
  int chain = -1;        // CTN_CHAIN: 1 a chain plan is always walked by k_chain, 2 by k_chain_lds (records, inputs and intermediates
                         // on chip) wherever chain_pack accepts the plan; unset: kChainLdsDefault
  int zipl = -1;         // CTN_ZIPL: 0 never run a zipper pair as one latency-form launch (k_zip_lat), 1 whenever the pair matches (tests)
  int zipl_max_r = 8;    // CTN_ZIPL_MAX_R: most networks in flight for which k_zip_lat is taken by default (100-site D = 256
                         // network, ms per pass, k_zip_lat / per-step launches: R = 1 1.40 / 2.05, 2: 1.58 / 3.3, 4: 2.1 / 3.5,
                         // 8: 4.1 / 4.4, 16: 8.5 / 7.0)
  int g_big_min_k = 1024;  // CTN_G_BIG_MIN_K: least K from which full long-K steps of any width take the 256 x 256 tiles
                           // (1536 until round 4; K = 1024, N = 1024: CP r = n = 1024 16.4 -> 15.9 ms, Tucker 15.8 -> 15.7 per mode product)
  int ares = -1;         // CTN_ARES: 0 never the resident-left-operand kernel (k_mfma_f32_ares), 1 whenever the step's shape allows (tests)
  int ares_ntw = 0;      // CTN_ARES_NTW: column tiles per workgroup of that kernel (tests)
  int g_big = 1;         // CTN_G_BIG=0: never the 256 x 256 tiles (experiments)
  int g_splitk = 1;      // CTN_G_SPLITK=0: no K split over workgroups on the large-tile kernel
  int zipl_mp = 0;       // CTN_ZIPL_MP=32|64: force the part of m1 a k_zip_lat workgroup owns (tests)
  int zipl64 = -1;       // CTN_ZIPL64: 1 a float64 zipper pair runs as one latency-form launch (k_zip_lat_f64) wherever the pair
                         // matches and no throughput form (CTN_ZIP=1) took it; 0 or unset: never (kZipLatF64Default)
  bool g_no_asm = false; // CTN_G_NO_ASM: C++ inner loop instead of the hand-scheduled blocks
  const char* stamps = nullptr;  // CTN_DEBUG_STAMPS=<file> (make STAMPS=1 builds): dump in-kernel cycle stamps
  int stamp_step = -1;   // CTN_DEBUG_STAMP_STEP=<s>: stamp only this step
};
inline DevSwitches read_dev_switches() {
  DevSwitches d;
  auto num = [](const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; };
  d.mfma_g = num("CTN_MFMA_G", 1);
  d.graph = num("CTN_GRAPH", 1);
  const int bk = num("CTN_MFMA_BK", 0);
  d.mfma_bk = (bk == 16 || bk == 32) ? bk : 0;
  d.splitk = num("CTN_SPLITK", -1);
  d.splitk_max = num("CTN_SPLITK_MAX", 0);
  d.lat = num("CTN_LAT", -1);
  d.hform = num("CTN_H", -1);
  d.zip = num("CTN_ZIP", -1);
  d.zipq = num("CTN_ZIPQ", -1);
  d.zipq_wgs = num("CTN_ZIPQ_WGS", 0);
  d.zip128 = num("CTN_ZIP128", 1);
  d.zipm64 = num("CTN_ZIPM64", 1);
  d.zip512 = num("CTN_ZIP512", 1);
  d.zipl = num("CTN_ZIPL", -1);
  d.cplx = num("CTN_CPLX", -1);
  d.chain = num("CTN_CHAIN", -1);
  d.zipl_max_r = num("CTN_ZIPL_MAX_R", 8);
  d.zipl_mp = num("CTN_ZIPL_MP", 0);
  d.zipl64 = num("CTN_ZIPL64", -1);
  d.g_splitk = num("CTN_G_SPLITK", 1);
  d.g_big = num("CTN_G_BIG", 1);
  d.ares = num("CTN_ARES", -1);
  d.ares_ntw = num("CTN_ARES_NTW", 0);
  d.g_big_min_k = num("CTN_G_BIG_MIN_K", 1024);
  d.dot_tr = num("CTN_DOT_TR", 1);
  d.sweep = num("CTN_SWEEP", -1);
  d.sweep64 = num("CTN_SWEEP64", 1);
  d.sweep_small = num("CTN_SWEEP_SMALL", -1);
  d.sweep_small64 = num("CTN_SWEEP_SMALL64", -1);
  d.sweep_small_tr = num("CTN_SWEEP_SMALL_TR", 1);
  d.lat64_min_k = num("CTN_LAT64_MIN_K", 512);
  d.splitk_fill_long = num("CTN_SPLITK_FILL_LONG", 2);
  d.lat_max_t = num("CTN_LAT_MAX_T", 64);
  d.lat_wg_per_cu_x2 = num("CTN_LAT_WG_X2", 2);
  d.halve = num("CTN_HALVE_TILES", 1);
  d.group = num("CTN_GROUP", 1);
  d.g_no_asm = getenv("CTN_G_NO_ASM") != nullptr;
  d.stamps = getenv("CTN_DEBUG_STAMPS");
  d.stamp_step = num("CTN_DEBUG_STAMP_STEP", -1);
  return d;
}

// What the rules below know of the kernels (engine.hip asserts that these are the kernels' own values): the large-tile
// fp32 kernel's tile rows and k-tile depth (GM, GK of kernels_mfma_g.h), the fp64 one's tile columns (DN of
// kernels_mfma_g64.h), and the longest K whose two k-offset tables fit the latency kernel's LDS (kLatMaxK of kernels_mfma_lat.h)
constexpr int kFormGM = 256, kFormGK = 16, kFormDN = 128, kFormLatMaxK = 4096;

// k-tile depth.  BK = 16: 32 KiB of LDS + 167 registers => 3 workgroups (12 waves) per CU, which
// hides the per-tile prologue/epilogue best when K is short (MPS shapes: 108-118 TFLOP/s vs
// 103-117 with BK = 32); BK = 32 halves the barriers per flop and wins on long-K GEMMs
// (4096^3: 130 vs 115 TFLOP/s).  CTN_MFMA_BK=16|32 forces one of them (development knob).
inline int mfma_bk(int K, const DevSwitches& sw) {
  if (sw.mfma_bk) return sw.mfma_bk;
  return K >= 2048 ? 32 : 16;
}

// Latency mode (see k_mfma_f32_sk): chosen when the 128-wide tiles of a step cannot occupy half the
// chip.  Returns the number of K splits (0 = use the throughput kernel).  CTN_SPLITK=0 disables,
// CTN_SPLITK=1 forces it for every eligible step (tests).
inline bool h_forced(const Step& st, int dtype, const DevSwitches& sw);
inline int splitk_splits(const Step& st, int R, int n_cu, int dtype, const DevSwitches& sw) {
  if (h_forced(st, dtype, sw)) return 0;
  const int mode = sw.splitk;
  const bool mfma = (dtype == CTN_F32 && st.kernel == CTN_KERNEL_MFMA_F32) || (dtype == CTN_F64 && st.kernel == CTN_KERNEL_MFMA_F64);
  if (mode == 0 || !mfma || st.collapse || st.K < 128 || st.modeA >= 3 || st.epw) return 0;
  const int max_tiles = sw.splitk_max;
  const int64_t limit = max_tiles > 0 ? max_tiles : n_cu / 2;
  if (mode != 1 && (int64_t)st.blocks * R > limit) return 0;
  const int64_t tiles64 = st.Bt * ((st.M + 63) / 64) * ((st.N + 63) / 64) * R;
  // 64 x 64 tiles that already give every CU a workgroup run un-split on the register-staged kernel: two K slabs plus
  // the reduce pass lose to it (7 replicas of 256 x 1024 x 256: 5.3 ms per 100-site network against 4.35 at 8) - a long
  // K (>= 1024) is still worth two slabs up to two workgroups per CU (16 x (256 x 256 x 1024): 7.02 -> 6.20 ms)
  if (tiles64 >= (int64_t)n_cu * (st.K >= 1024 ? sw.splitk_fill_long : 1) && mode != 1) return 0;
  int64_t S = (2 * (int64_t)n_cu + tiles64 - 1) / tiles64;   // aim at ~2 small workgroups per CU
  S = std::max<int64_t>(1, std::min<int64_t>(S, st.K / 64));
  // one split is no split: the register-staged kernel on halved tiles does the same work without slab and reduce pass
  // (8 replicas of a 256 x 1024 x 256 step; CTN_SPLITK=1 keeps it for the tests)
  if (S <= 1 && mode != 1) return 0;
  return (int)S;
}

// One-launch latency form (k_mfma_f32_lat): K split over the eight waves of a workgroup instead of over
// workgroups, no slabs and no reduce launch.  Returns the tile edge T (16, 32 or 64), 0 = not taken.
// Same launch-size condition as split-K (the step's 128-wide tiles cannot occupy half the chip); the largest tile
// that still gives every CU a workgroup (with one network in flight a 256 x 256 x 1024 step runs as 256 tiles of
// 16 x 16: on 64 tiles of 32 x 32 three quarters of the matrix pipes idle and the step takes 14 us instead of ~6);
// at most kLatMaxTiles tiles per replica (one abs-sum partial each), both k-offset tables in LDS.
constexpr int kLatMaxTiles = kMaxPartials;
inline int lat_form(const Step& st, int R, int n_cu, int dtype, const DevSwitches& sw) {
  if (h_forced(st, dtype, sw)) return 0;           // tests of the one-tile-per-CU form (CTN_H=1)
  const bool f64 = dtype == CTN_F64 && st.kernel == CTN_KERNEL_MFMA_F64;
  if (sw.lat == 0 || !(f64 || (dtype == CTN_F32 && st.kernel == CTN_KERNEL_MFMA_F32)) || st.rhs < 0 || st.modeA >= 3 || st.epw) return 0;
  if (st.K > kFormLatMaxK || st.K < 32) return 0;
  if (sw.mfma_g >= 2 && (f64 ? st.tileN == 128 : st.tileM == 256)) return 0;   // tests that force the large-tile kernels
  if (sw.lat != 1 && ((int64_t)st.blocks * R > n_cu / 2 || st.K < 128)) return 0;
  auto tiles = [&](int T) { return st.Bt * ((st.M + T - 1) / T) * ((st.N + T - 1) / T); };
  const int64_t t16 = tiles(16), t32 = tiles(32), t64 = tiles(64);
  // ... and not more than one workgroup per CU (a second round of 512-thread workgroups doubles the step): beyond
  // that split-K / halved register-staged tiles win (100-site D = 256 network, R = 4: 3.49 vs 4.23 ms; R = 5: 5.33 vs
  // 4.61; R = 6: 5.55 vs 4.79; R = 8: 5.83 vs 4.37)
  auto fits = [&](int64_t t) { return t <= kLatMaxTiles && (sw.lat == 1 || t * R <= (int64_t)n_cu * sw.lat_wg_per_cu_x2 / 2); };
  if (f64) return fits(t16) ? 16 : 0;     // fp64: 16 x 16 tiles (v_mfma_f64_16x16x4_f64) only
  // (a k-contiguous operand reaches the fragment registers as 4-byte loads a row stride apart; with a short K split
  // eight ways there is nothing to pipeline them behind: 1024 x 1024 x 256, A k-contiguous, took 27.8 us on 256 tiles
  // of 64 x 64 against 23.7 us for the LDS-staged tiles with two K slabs - while the same tile count with both
  // operands row-contiguous, 4 x (256 x 1024 x 256), is 6 % faster here than there)
  const bool kcontig = st.modeA == 2 || st.modeB == 2;
  // (... and with K = 1024 the plain 64 x 64 tiles win: 16 replicas of 256 x 256 x 1024, 7.53 -> 7.03 ms per network)
  if (sw.lat_max_t >= 64 && t64 * R >= n_cu && fits(t64) && st.K <= 512 && (!kcontig || st.K >= sw.lat64_min_k)) return 64;
  if (t32 * R >= n_cu && fits(t32)) return 32;
  if (fits(t16)) return 16;
  if (fits(t32)) return 32;
  // half the CUs busy with 64 x 64 tiles still beats four K slabs plus a reduce pass (2 / 3 replicas of
  // 256 x 1024 x 256: 3.47 -> 3.28 / 3.62 -> 3.44 ms per 100-site network)
  if (sw.lat_max_t >= 64 && 2 * t64 * R >= n_cu && fits(t64) && st.K <= 256 && !kcontig) return 64;   // (a long K is better off split over workgroups)
  return 0;
}

// CTN_H=1 (tests): a step whose SHAPE admits the one-tile-per-CU form takes it whatever the launch size - the latency
// forms step aside (the remaining conditions - vector-storable C, not the last step - are checked by h_form itself)
inline bool h_forced(const Step& st, int dtype, const DevSwitches& sw) {
  return sw.hform == 1 && dtype == CTN_F32 && st.kernel == CTN_KERNEL_MFMA_F32 && st.rhs >= 0 && !st.collapse &&
         st.modeA >= 1 && st.modeA <= 2 && st.modeB >= 1 && st.modeB <= 2 && st.K % 32 == 0 && st.K >= 64 && st.cvec &&
         (st.epw ? (st.epw_split && (st.epw == 2 || st.epw == 4)) : st.lhs2 < 0) &&
         st.Bt * ((st.M + 127) / 128) * ((st.N + 127) / 128) <= kMaxPartials;
}

// One-tile-per-CU form (k_mfma_f32_h, kernels_mfma_h.h): 128 x 128 tiles, K split over the two halves of an 8-wave
// workgroup.  Taken when the step's 128 x 128 tiles are about one round of one workgroup per CU - between three quarters
// of a chip and a whole one - which is where the register-staged kernel's 128 x 64 tiles run as a single round of two small
// workgroups per CU and the large-tile kernel would leave CUs idle (one MPS site applied to 4096 inputs: 256 tiles).
inline bool h_form(const Plan& P, const Step& st, int R, int n_cu, int dtype, const DevSwitches& sw, bool c_vec) {
  if (sw.hform == 0 || dtype != CTN_F32 || st.kernel != CTN_KERNEL_MFMA_F32 || st.rhs < 0 || st.collapse) return false;
  if (st.modeA < 1 || st.modeA > 2 || st.modeB < 1 || st.modeB > 2) return false;      // LDS-DMA: 16-byte requests only
  if (st.epw ? !(st.epw_split && (st.epw == 2 || st.epw == 4)) : st.lhs2 >= 0) return false;
  if (st.K % 32 != 0 || st.K < 64 || !c_vec) return false;
  if (P.tensors[st.lhs].numel > (1LL << 30) || P.tensors[st.rhs].numel > (1LL << 30)) return false;   // 32-bit byte offsets
  const int64_t t128 = st.Bt * ((st.M + 127) / 128) * ((st.N + 127) / 128);
  if (t128 > kMaxPartials) return false;
  if (sw.hform == 1) return true;
  if (sw.mfma_g >= 2 && st.tileM == 256) return false;     // tests that force the large-tile kernels
  // (from three quarters of a chip of tiles: at half a chip - 8 networks of the headline in flight, 2048 inputs through
  // the batched MPS - the smaller tiles of the other forms keep more CUs busy: 27.1 vs 20.6 us per site at B = 2048)
  return 4 * t128 * R >= 3 * n_cu && t128 * R <= n_cu;
}

// Tile of the register-staged fp32 kernel for this step and replica count: the planner's 128 / 64 choice, halved
// (rows or columns, the larger extent first) while the launch has fewer than two workgroups per CU - one network with
// a batch leg, or a fused step whose output is a quarter of the GEMM it replaced - as long as the tile count still
// fits the step's partial-sum region.  Steps the planner made eligible for the large-tile kernel keep 128-unit
// counting (their fallback must agree with it), and so do steps that already go through the collapse pass.
inline bool g_launch(const Step& st, int R, int n_cu, int use_g) {
  // does a launch of this (planner-eligible) step take the large-tile LDS-DMA kernel?  At least two of the big tiles
  // per CU and K >= 192 (below that the 128-tile kernel's 3-4 workgroups per CU hide the per-tile cost better), or a
  // long K (>= 1024) from 7/8 of a tile per CU; CTN_MFMA_G=2: whenever eligible (tests)
  if (!use_g || st.kernel != CTN_KERNEL_MFMA_F32 || st.tileM != 256) return false;
  const int64_t gtiles = st.Bt * ((st.M + 255) / 256) * ((st.N + st.tileN - 1) / st.tileN) * R;
  if (use_g >= 2 || (gtiles >= 2LL * n_cu && st.K >= 192)) return true;
  // ... below two tiles per CU a long K still pays, provided the tiles divide evenly over the CUs: 320 tiles are two
  // rounds on 64 CUs and one on the rest (100-site network: 160 replicas 42.8 ms against 39.7 on 128-wide tiles; 96
  // replicas = 192 tiles 25.2 against 23.1; 112 = 224 tiles 28.4 against 29.7, 128 = 256 tiles 29.0 against 29.1)
  const int64_t rounds = (gtiles + n_cu - 1) / n_cu;
  return st.K >= 1024 && 4 * gtiles >= 3LL * n_cu && 100 * gtiles >= 85 * rounds * n_cu;
}

// K split over workgroups ON the large-tile LDS-DMA kernel (256 x 128 tiles; k_mfma_f32_g with a.ks_S > 0, then the
// fixed-order reduce pass): a planner-eligible step whose tiles cannot fill the chip by themselves while K is long - the
// root GEMMs of a sliced 2D grid with a rank's few slices in flight (8 x (512 x 512 x 4096): 64 tiles; they ran as 512
// register-staged 64 x 64 tiles), a batch of 256 x 256 x 2^20 products.  Returns the number of splits (0 = not taken): about
// two workgroups per CU, every split at least 256 deep and a whole number of 16-deep k-tiles.
inline int g_splitk(const Step& st, int R, int n_cu, int use_g, const DevSwitches& sw, bool c_vec) {
  if (!use_g || sw.g_splitk == 0 || st.kernel != CTN_KERNEL_MFMA_F32 || st.tileM != 256 || !c_vec || st.collapse || st.rhs < 0) return 0;
  if (st.K < 2048 || st.K % kFormGK != 0) return 0;
  const int64_t gtiles = st.Bt * ((st.M + kFormGM - 1) / kFormGM) * ((st.N + st.tileN - 1) / st.tileN) * R;
  if (gtiles >= n_cu) return 0;
  int64_t S = (2LL * n_cu + gtiles - 1) / gtiles;
  S = std::min<int64_t>(std::min<int64_t>(S, 16), st.K / 256);   // (at most 16 slabs: one reduce pass, no folding)
  while (S > 1 && (st.K % S != 0 || (st.K / S) % kFormGK != 0)) --S;
  return S >= 2 ? (int)S : 0;
}

inline void plain_tiles(const Step& st, int R, int n_cu, int use_g, bool is_last, int* tm, int* tn, int halve = 1) {
  *tm = st.tileM == 64 ? 64 : kTileM;
  *tn = st.tileN;
  if (st.kernel != CTN_KERNEL_MFMA_F32 || st.collapse || !halve) return;
  // a step the planner made eligible for the large-tile kernel keeps 128-unit counting when that kernel will (or,
  // for the caller's possibly unaligned final buffer, may) take it
  if (st.tileM == 256 && (is_last || g_launch(st, R, n_cu, use_g))) return;
  auto tiles = [&](int a, int b) { return st.Bt * ((st.M + a - 1) / a) * ((st.N + b - 1) / b); };
  while (tiles(*tm, *tn) * R < 2LL * n_cu) {
    int a = *tm, b = *tn;
    // columns first: 128 x 64 tiles measured 62 vs 45 TFLOP/s for 64 x 128 on 4096 x 1024 x 256 (one batched-MPS site)
    if (b == 128 && st.N > 64) b = 64;
    else if (a == 128 && st.M > 64) a = 64;
    else break;
    if (tiles(a, b) > 4096) break;
    *tm = a; *tn = b;
  }
}

// A streaming step with few output items and a long K (column sums, `ab,ab->b`: 4 workgroups walked K = 4096 one
// element at a time - 1.7 ms for 67 MB): split K over workgroups, partial sums through the split-K reduce pass
inline int stream_splits(const Step& st, int R, int n_cu) {
  if (st.kernel != CTN_KERNEL_ELEMENT || st.K < 1024 || st.kvec) return 0;
  const int64_t wgs = (int64_t)st.blocks * R;
  if (wgs >= 2LL * n_cu) return 0;
  return (int)std::max<int64_t>(2, std::min<int64_t>(std::min<int64_t>(st.K / 128, 1024), (8LL * n_cu + wgs - 1) / wgs));
}

// k_stream variant of a plain streaming step: vector width along n and vectors per row lookup (4 only where it pays:
// short K - lookup-dominated - and enough rows left to fill the chip; long-K / small steps keep one for parallelism)
inline void stream_variant(const Step& st, int R, int vw, int* u, int64_t* nq) {
  *nq = (st.Nv + vw - 1) / vw;
  const int64_t rows = st.H * st.L * (int64_t)R;
  *u = (*nq % 4 == 0 && st.K <= 16 && rows * (*nq / 4) >= (1 << 20)) ? 4 : 1;
}

// Row-dot steps (one wave per output) with few outputs and a long K: split K over workgroups too
inline int rowdot_splits(const Step& st, int R, int n_cu) {
  if (st.kernel != CTN_KERNEL_ROWDOT || st.K < 4096) return 0;
  const int64_t waves = st.H * st.L * st.Nv * (int64_t)R;
  if (waves >= 16LL * n_cu) return 0;
  return (int)std::max<int64_t>(2, std::min<int64_t>(std::min<int64_t>(st.K / 1024, 1024), (16LL * n_cu + waves - 1) / waves));
}

// Tiny output, huge K (CTN_KERNEL_DOT: at most 64 outputs): split K over workgroups as well, see k_dot_split
inline int dot_splits(const Step& st) {
  if (st.kernel != CTN_KERNEL_DOT || st.K < 32768) return 0;
  return (int)std::min<int64_t>(1024, st.K / 8192);
}

// The launch form of a plain step: the kernel, and every size that follows from the choice.  (Zipper and complex pairs,
// the resident-operand kernel, sweeps and leaf groups are found on the plan's tables by their own matchers when the
// executor is created, and override this; a chain plan is walked whole.)
enum class Kind {
  None,                                                   // CTN_KERNEL_FUSED: formed inside its consumer, nothing to launch
  GSplitK, Lat, SplitK, H, G256, G128, Plain,             // fp32 MFMA: k_mfma_f32_g with a K split, k_mfma_lat, k_mfma_f32_sk, k_mfma_f32_h,
                                                          // k_mfma_f32_g on 256 x 256 / 256 x 128 tiles, k_mfma_f32 (register-staged)
  Lat64, SplitK64, G64, Plain64,                          // fp64 MFMA: k_mfma_lat, k_mfma_f64_sk, k_mfma_f64_g, k_mfma_f64
  Dot, DotSplit, RowDot, StreamKvec, Stream               // k_dot, k_dot_split / k_dot_tr, k_rowdot, k_stream_kvec, k_stream
};
constexpr int kNumKinds = (int)Kind::Stream + 1;

struct StepForm {
  Kind kind = Kind::None;
  int tm = 0, tn = 0;          // the tile ctn_exec_step_tile reports (0: not an MFMA kernel, nothing reported)
  int S = 0;                   // K splits over workgroups as the slab buffers are sized for them, else 0
  int T = 0;                   // latency-form tile edge, else 0
  int kchunk = 0;              // K per split (S > 0: the launch has ceil(K / kchunk) splits, empty trailing ones dropped) or per
                               // wave of the latency form, else 0
  int64_t blocks = 0;          // workgroups per replica of the main launch
  int partials = 1;            // slots per replica of the step's partial-sum region
  bool collapse = false;       // the launch writes collapse_blocks partials per replica to the scratch buffer and k_collapse
                               // folds them into the region's one slot
  int64_t collapse_blocks = 0; // ... and otherwise what the step asks of the scratch buffer's size (0: nothing)
};

inline int form_splits(const Step& st, const StepForm& f) { return (int)((st.K + f.kchunk - 1) / f.kchunk); }

// `c_vec`: may this launch store C as 16-byte vectors - Step::cvec, and for the last step a 16-byte aligned caller
// buffer.  It decides between the large-tile kernel and its register-staged fallback on the last step and nothing else:
// S, partials and collapse_blocks do not depend on it, so an executor sizes its buffers once for both.
inline StepForm step_form(const Plan& P, int s, int R, int n_cu, const DevSwitches& sw, bool c_vec) {
  const Step& st = P.steps[s];
  const bool last = s + 1 == P.n_steps;
  auto tiles = [&](int a, int b) { return st.Bt * ((st.M + a - 1) / a) * ((st.N + b - 1) / b); };
  // the reduce pass of a K split over workgroups spreads over up to kWaveOutputs workgroups, one partial each
  const int reduce_slots = (int)std::max<int64_t>(1, std::min<int64_t>(kWaveOutputs, P.tensors[st.out].numel / 1024));
  StepForm f;
  f.blocks = st.blocks;
  f.partials = std::max(st.partials, 1);
  f.collapse = st.collapse;
  f.collapse_blocks = st.collapse ? st.blocks : 0;
  auto uncollapsed = [&](Kind k, int tm, int tn) { f.kind = k; f.tm = tm; f.tn = tn; f.collapse = false; f.collapse_blocks = 0; };
  switch (st.kernel) {
    case CTN_KERNEL_FUSED:
      f.blocks = 0;
      return f;
    case CTN_KERNEL_MFMA_F32: {
      // the large-tile split-K only on a step with a consumer (the final step goes on to the latency form, whose S can
      // exceed the 16 slabs of the large-tile one; with a consumer, c_vec is Step::cvec)
      if (!last && (f.S = g_splitk(st, R, n_cu, sw.mfma_g, sw, st.cvec))) {
        uncollapsed(Kind::GSplitK, 256, 128);
        f.kchunk = (int)(st.K / f.S);
        f.blocks = tiles(kFormGM, st.tileN) * f.S;
        f.partials = reduce_slots;
        return f;
      }
      if ((f.T = lat_form(st, R, n_cu, P.dtype, sw))) {
        uncollapsed(Kind::Lat, f.T, f.T);
        const int ks = f.T == 64 ? 2 : 8, kp = f.T == 16 ? 4 : 2;
        f.kchunk = (int)(((st.K + ks - 1) / ks + kp - 1) / kp * kp);
        f.blocks = tiles(f.T, f.T);
        f.partials = (int)f.blocks;            // one partial per tile, written directly
        return f;
      }
      if ((f.S = splitk_splits(st, R, n_cu, P.dtype, sw))) {
        uncollapsed(Kind::SplitK, 64, 64);     // (splitk_splits takes no step that collapses)
        f.kchunk = (int)(((st.K + f.S - 1) / f.S + 31) / 32 * 32);
        f.blocks = tiles(64, 64) * form_splits(st, f);
        f.partials = reduce_slots;
        return f;
      }
      const bool g = g_launch(st, R, n_cu, sw.mfma_g);
      if (!g && !last && h_form(P, st, R, n_cu, P.dtype, sw, c_vec)) {
        uncollapsed(Kind::H, 128, 128);
        f.blocks = tiles(128, 128);
        f.partials = (int)f.blocks;            // one partial per tile (<= kMaxPartials)
        return f;
      }
      // register-staged tiles; halved (128 -> 64 rows / columns) while the launch is under-filled - see plain_tiles.
      // They size the region of a step that runs on the large-tile kernel too (128-unit counting, not 256-row tiles).
      int tm, tn;
      plain_tiles(st, R, n_cu, sw.mfma_g, last, &tm, &tn, sw.halve);
      const int64_t plain = tiles(tm, tn);
      if (!st.collapse) {
        f.partials = plain > kMaxPartials ? 1 : (int)plain;   // halved tiles beyond the slots: collapsed at launch
        f.collapse_blocks = plain;
      }
      // large-tile LDS-DMA variant (kernels_mfma_g.h) where the step's shape allows it.
      // CTN_MFMA_G (read when the executor is created): 0 = never, 1 = 256x128 tiles when the launch
      // fills the chip (default), 2 = whenever eligible (tests)
      // ... and the launch has at least two of the big tiles per CU: with fewer, 128-row tiles spread the
      // same work over more CUs (measured: 2048^3 runs at 90 vs 56 TFLOP/s, 4096^3 at 125 vs 135)
      // ... and K >= 192: below that the 128-tile kernel's 3-4 workgroups per CU hide the per-tile cost
      // better (8192 x 8192 x K: K = 64 old +7 %, 128 +2 %, 192 equal, 256 large tiles +5 %)
      // ... and long K (>= 1024) already from 3/4 of a tile per CU: the per-tile cost amortises over the k loop
      // (256 x 256 x 1024 per replica, R = 96 / 128: 86.9 / 106.2 vs 80.3 / 95.8 TFLOP/s; R = 48 / 64 lose)
      if (g && c_vec) {
        const int64_t gtiles = tiles(kFormGM, st.tileN) * R;
        const bool kcontig = st.modeA == 2 || st.modeB == 2;
        // long-K steps on narrow outputs whose tiles are all full also exist as 256 x 256 tiles (8 waves, one
        // workgroup per CU): with N <= 512 each A tile is fetched half as often (256 x 256 x 1024 per replica:
        // 133.9 vs 130.3 TFLOP/s); K = 256 steps (116.0 vs 116.7) and wide outputs (8192 x 8192 x 768: 130.3 vs
        // 132.1) are better off with 256 x 128
        // - and so are very long K on any width (K = 2048 ... 8192: +1.5 ... +3 %)
        const bool big = sw.mfma_g == 1 && sw.g_big && !kcontig && st.M % 256 == 0 && st.N % 256 == 0 && st.K % kFormGK == 0 &&
                         ((st.K >= 512 && st.N <= 512) || st.K >= sw.g_big_min_k) && gtiles / 2 >= (int64_t)n_cu;
        f.kind = big ? Kind::G256 : Kind::G128;
        f.tm = 256; f.tn = big ? 256 : 128;
        f.blocks = big ? st.Bt * ((st.M + kFormGM - 1) / kFormGM) * (st.N / 256) : tiles(kFormGM, st.tileN);
        return f;
      }
      f.kind = Kind::Plain; f.tm = tm; f.tn = tn;
      f.blocks = plain;
      if (plain > kMaxPartials) { f.collapse = true; f.collapse_blocks = plain; }
      return f;
    }
    case CTN_KERNEL_MFMA_F64: {
      if ((f.T = lat_form(st, R, n_cu, P.dtype, sw))) {        // one-launch latency form, 16 x 16 tiles
        uncollapsed(Kind::Lat64, f.T, f.T);
        f.kchunk = (int)(((st.K + 7) / 8 + 3) / 4 * 4);
        f.blocks = tiles(f.T, f.T);
        f.partials = (int)f.blocks;
        return f;
      }
      if ((f.S = splitk_splits(st, R, n_cu, P.dtype, sw))) {   // latency mode, as in fp32
        uncollapsed(Kind::SplitK64, 64, 64);
        f.kchunk = (int)(((st.K + f.S - 1) / f.S + 31) / 32 * 32);
        f.blocks = tiles(64, 64) * form_splits(st, f);
        f.partials = reduce_slots;
        return f;
      }
      // 128 x 128 LDS-DMA kernel, under the same launch-size rule as fp32
      if (sw.mfma_g && st.tileN == kFormDN && (sw.mfma_g >= 2 || tiles(kTile64M, kFormDN) * R >= 2LL * n_cu)) {
        f.kind = Kind::G64; f.tm = 128; f.tn = 128;
        f.blocks = tiles(kTile64M, kFormDN);
        return f;
      }
      f.kind = Kind::Plain64; f.tm = 128; f.tn = 64;
      return f;
    }
    case CTN_KERNEL_DOT:
      if ((f.S = dot_splits(st))) {
        f.kind = Kind::DotSplit;
        f.kchunk = (int)(((st.K + f.S - 1) / f.S + 255) / 256 * 256);
        f.blocks = (int64_t)st.blocks * form_splits(st, f);
        f.partials = reduce_slots;
        return f;
      }
      f.kind = Kind::Dot;
      return f;
    case CTN_KERNEL_ROWDOT:
      f.kind = Kind::RowDot;
      if ((f.S = rowdot_splits(st, R, n_cu))) {
        f.kchunk = (int)(((st.K + f.S - 1) / f.S + 63) / 64 * 64);
        f.blocks = (int64_t)st.blocks * form_splits(st, f);
        f.partials = reduce_slots;
        f.collapse = false; f.collapse_blocks = 0;             // the reduce pass writes the region itself
      }
      return f;
    default:
      // short unit-stride K of the left operand: one output per thread, 16-byte loads along k
      if (st.kvec) { f.kind = Kind::StreamKvec; return f; }
      f.kind = Kind::Stream;
      if ((f.S = stream_splits(st, R, n_cu))) {
        f.kchunk = (int)((st.K + f.S - 1) / f.S);
        f.blocks = (int64_t)st.blocks * form_splits(st, f);
        f.partials = reduce_slots;
        f.collapse = false; f.collapse_blocks = 0;
      }
      return f;
  }
}

}  // namespace ctn
