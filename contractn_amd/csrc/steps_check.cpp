// steps_check.cpp - host-only driver of step_form() (launch_form.h): which kernel a PLAIN step of a plan runs on, by name.
//
//   make -C contractn_amd/csrc steps_check   ->  ../lib/steps_check_asan   (-fsanitize=address,undefined)
//   steps_check_asan R=1,CU=256,LAT=0,SPLITK=1 R=3,H=1,SWEEP=0 ... < plans.txt   (the input format of plan_check.cpp)
//
// Every argument is one setting: the networks in flight (R, default 1), the chip's CUs (CU, default 256) and every
// development switch a plain step's form depends on, by the name of its environment variable without the CTN_ prefix
// (LAT, LAT_MAX_T, LAT_WG_X2, LAT64_MIN_K, SPLITK, SPLITK_MAX, SPLITK_FILL_LONG, H, HALVE_TILES, MFMA_G, MFMA_BK, G_BIG,
// G_BIG_MIN_K, G_SPLITK, ARES, ARES_NTW, DOT_TR) plus the switches of the fused forms that would take a step away from
// step_form() (ZIP, ZIPQ, ZIPL, CPLX, SWEEP, CHAIN, GROUP) - filled into a DevSwitches directly, the environment is not
// read.  For every plan, every setting, each of the chip sizes (the setting's CU, then 64 and 304) and every step one line
// goes to stdout:
//
//   plan <i> set <j> cu <n> step <s> last=<0|1> kernel=<ctn_kernel> modeA=<0..5> modeB=<0..2> tileM=<n> tileN=<n> cvec=<0|1>
//     Bt=<n> M=<n> N=<n> K=<n> swapped=<0|1> pblocks=<n> pcollapse=<0|1>                                   (the planner's Step)
//     kind=<Kind by name> tm=<n> tn=<n> S=<n> T=<n> kchunk=<n> splits=<n> blocks=<n> partials=<n> collapse=<0|1> cblocks=<n> bk=<16|32|0>
//     role=<P|A|Z|L|C> slots=<the region fused_forms() gives the step> ares=<ntw, 0 = not taken> avec=<0|1>
//     H=<n> L=<n> Nv=<n> sAn=<n> sBn=<n> vecw=<1|2|4> kvec=<0|1> u=<1|4, 0 = no k_stream variant> u1=<1|4|0>   (the streaming decomposition)
//     group=<length of the LeafGroup this step heads, else 0> dottr=<0|1> Ka=<n> Kb=<n> chain=<Plan::chain>
//     divA=<0|1> divB=<0|1>                                        (the operand is a step's result: divided by its rescale on load)
//
// `splits` is the number of K slabs the launch really has (empty trailing ones dropped), `bk` the k-tile depth of the
// register-staged fp32 kernel (0 for every other kind), `u` what stream_variant() gives a plain streaming step at the
// plan's own vector width and this R, `u1` the same at vector width 1 (a final step whose caller's buffer is not 16-byte
// aligned).  The form is evaluated with c_vec = Step::cvec: the last step's
// also depends on the alignment of the caller's buffer, which the engine's own staging buffers satisfy.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "fused_forms.h"

using namespace ctn;

struct Setting { int R = 1, cu = 256; DevSwitches sw; };

static bool parse_setting(const char* arg, Setting* out) {
  std::string s(arg);
  for (size_t p = 0; p < s.size();) {
    const size_t e = std::min(s.find(',', p), s.size()), q = s.find('=', p);
    if (q == std::string::npos || q > e) return false;
    const std::string key = s.substr(p, q - p);
    const int v = atoi(s.substr(q + 1, e - q - 1).c_str());
    DevSwitches& d = out->sw;
    if (key == "R") out->R = v;
    else if (key == "CU") out->cu = v;
    else if (key == "LAT") d.lat = v;
    else if (key == "LAT_MAX_T") d.lat_max_t = v;
    else if (key == "LAT_WG_X2") d.lat_wg_per_cu_x2 = v;
    else if (key == "LAT64_MIN_K") d.lat64_min_k = v;
    else if (key == "SPLITK") d.splitk = v;
    else if (key == "SPLITK_MAX") d.splitk_max = v;
    else if (key == "SPLITK_FILL_LONG") d.splitk_fill_long = v;
    else if (key == "H") d.hform = v;
    else if (key == "HALVE_TILES") d.halve = v;
    else if (key == "MFMA_G") d.mfma_g = v;
    else if (key == "MFMA_BK") d.mfma_bk = (v == 16 || v == 32) ? v : 0;
    else if (key == "G_BIG") d.g_big = v;
    else if (key == "G_BIG_MIN_K") d.g_big_min_k = v;
    else if (key == "G_SPLITK") d.g_splitk = v;
    else if (key == "ARES") d.ares = v;
    else if (key == "ARES_NTW") d.ares_ntw = v;
    else if (key == "ZIP") d.zip = v;
    else if (key == "ZIPQ") d.zipq = v;
    else if (key == "ZIPL") d.zipl = v;
    else if (key == "CPLX") d.cplx = v;
    else if (key == "SWEEP") d.sweep = v;
    else if (key == "CHAIN") d.chain = v;
    else if (key == "GROUP") d.group = v;
    else if (key == "DOT_TR") d.dot_tr = v;
    else return false;
    p = e + 1;
  }
  return out->R >= 1 && out->cu >= 1;
}

static const char* kind_name(Kind k) {
  static_assert(kNumKinds == 17 && (int)Kind::None == 0 && (int)Kind::Plain == 7 && (int)Kind::Plain64 == 11 && (int)Kind::Stream == 16,
                "the names below follow the order of enum class Kind (launch_form.h)");
  static const char* names[kNumKinds] = {"None", "GSplitK", "Lat", "SplitK", "H", "G256", "G128", "Plain", "Lat64", "SplitK64",
                                         "G64", "Plain64", "Dot", "DotSplit", "RowDot", "StreamKvec", "Stream"};
  return names[(int)k];
}

static void print_steps(int plan, int set, const Plan& P, const Setting& st_, int cu) {
  const FusedForms F = fused_forms(P, st_.R, cu, st_.sw);
  for (int s = 0; s < P.n_steps; ++s) {
    const Step& st = P.steps[s];
    const StepForm f = step_form(P, s, st_.R, cu, st_.sw, st.cvec);
    const bool slabs = f.S > 0 && f.kchunk > 0;
    const int bk = f.kind == Kind::Plain ? (f.tm == 64 ? 16 : mfma_bk((int)st.K, st_.sw)) : 0;
    int u = 0, u1 = 0;
    int64_t nq = 0;
    if (f.kind == Kind::Stream) { stream_variant(st, st_.R, st.vecw, &u, &nq); stream_variant(st, st_.R, 1, &u1, &nq); }
    const DotTr& dt = F.dot_tr[s];
    printf("plan %d set %d cu %d step %d last=%d kernel=%d modeA=%d modeB=%d tileM=%d tileN=%d cvec=%d Bt=%lld M=%lld N=%lld K=%lld "
           "swapped=%d pblocks=%d pcollapse=%d kind=%s tm=%d tn=%d S=%d T=%d kchunk=%d splits=%d blocks=%lld partials=%d collapse=%d "
           "cblocks=%lld bk=%d role=%c slots=%d ares=%d avec=%d H=%lld L=%lld Nv=%lld sAn=%lld sBn=%lld vecw=%d kvec=%d u=%d u1=%d group=%d "
           "dottr=%d Ka=%d Kb=%d chain=%d divA=%d divB=%d\n",
           plan, set, cu, s, s + 1 == P.n_steps ? 1 : 0, st.kernel, st.modeA, st.modeB, st.tileM, st.tileN, st.cvec ? 1 : 0,
           (long long)st.Bt, (long long)st.M, (long long)st.N, (long long)st.K, st.swapped ? 1 : 0, st.blocks, st.collapse ? 1 : 0,
           kind_name(f.kind), f.tm, f.tn, f.S, f.T, f.kchunk, slabs ? form_splits(st, f) : 0, (long long)f.blocks, f.partials,
           f.collapse ? 1 : 0, (long long)f.collapse_blocks, bk, "PAZLC"[(int)F.role[s]], F.step_partials[s],
           F.ares_ntw[s] & 0xffff, F.ares_ntw[s] >> 16, (long long)st.H, (long long)st.L, (long long)st.Nv, (long long)st.sAn,
           (long long)st.sBn, st.vecw, st.kvec ? 1 : 0, u, u1, F.groups[s].len, dt.on ? 1 : 0, dt.on ? dt.Ka : 0, dt.on ? dt.Kb : 0,
           P.chain ? 1 : 0, st.lhs >= P.n_inputs ? 1 : 0, st.rhs >= P.n_inputs ? 1 : 0);
  }
}

int main(int argc, char** argv) {
  std::vector<Setting> sets;
  for (int i = 1; i < argc; ++i) {
    Setting st;
    if (!parse_setting(argv[i], &st)) { fprintf(stderr, "bad setting '%s'\n", argv[i]); return 2; }
    sets.push_back(st);
  }
  if (sets.empty()) sets.push_back(Setting());
  std::string tok;
  int n_plans = 0, n_fail = 0;
  while (std::cin >> tok) {
    if (tok != "plan") { fprintf(stderr, "expected 'plan', got '%s'\n", tok.c_str()); return 2; }
    ctn_plan_desc d{};
    std::cin >> d.dtype >> d.n_inputs >> d.n_steps;
    std::vector<int32_t> in_ndim, in_labels, lhs, rhs, ond, olab;
    std::vector<int64_t> in_dims;
    for (int i = 0; i < d.n_inputs; ++i) {
      int nd;
      std::cin >> tok >> nd;
      in_ndim.push_back(nd);
      for (int a = 0; a < nd; ++a) { int64_t x; std::cin >> x; in_dims.push_back(x); }
      for (int a = 0; a < nd; ++a) { int32_t x; std::cin >> x; in_labels.push_back(x); }
    }
    for (int s = 0; s < d.n_steps; ++s) {
      int l, r, nd;
      std::cin >> tok >> l >> r >> nd;
      lhs.push_back(l); rhs.push_back(r); ond.push_back(nd);
      for (int a = 0; a < nd; ++a) { int32_t x; std::cin >> x; olab.push_back(x); }
    }
    if (!std::cin) { fprintf(stderr, "truncated plan description\n"); return 2; }
    in_dims.push_back(0); in_labels.push_back(0); olab.push_back(0);   // keep .data() non-null for rank-0 tensors
    d.in_ndim = in_ndim.data(); d.in_dims = in_dims.data(); d.in_labels = in_labels.data(); d.in_strides = nullptr;
    d.step_lhs = lhs.data(); d.step_rhs = rhs.data(); d.step_out_ndim = ond.data(); d.step_out_labels = olab.data();
    d.stabilize = 1; d.min_norm = 1e-7;
    Plan P;
    std::string err;
    const int rc = build_plan(d, P, err);
    ++n_plans;
    if (rc != CTN_OK) { printf("plan %d rc=%d %s\n", n_plans, rc, err.c_str()); ++n_fail; continue; }
    for (size_t j = 0; j < sets.size(); ++j) {
      int cus[3] = {sets[j].cu, 64, 304};
      for (int c = 0; c < 3; ++c)
        if (c == 0 || cus[c] != cus[0]) print_steps(n_plans, (int)j, P, sets[j], cus[c]);
    }
  }
  return n_fail ? 1 : 0;
}
