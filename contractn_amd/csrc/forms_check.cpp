// forms_check.cpp - host-only driver of fused_forms() (fused_forms.h), for sanitizer runs on the CPU.
//
//   make -C contractn_amd/csrc forms_check   ->  ../lib/forms_check_asan   (-fsanitize=address,undefined)
//   forms_check_asan R=512,CU=256 R=1,CU=256,ZIP=1,ZIPQ=2 ... < plans.txt   (the input format of plan_check.cpp)
//
// Every argument is one setting: the networks in flight (R, default 1), the chip's CUs (CU, default 256) and development
// switches by the names of their environment variables without the CTN_ prefix (ZIP, ZIPQ, ZIPL, ZIPL_MP, ZIPL_MAX_R, ZIPL64,
// ZIP128, ZIPM64, ZIP512, CPLX, SWEEP, SWEEP64, SWEEP_SMALL, SWEEP_SMALL64, SWEEP_SMALL_TR, GROUP, ARES, ARES_NTW, DOT_TR) - filled into a DevSwitches directly, the
// environment is not read.  ALIAS_LD=<n> is no switch but a change to the PLAN, for the one rule of the sweep matchers that
// no planner-made layout reaches: the result of the run that sweep_small_match finds is moved onto the run's input in the
// workspace, with rows n elements apart (a two-step run; n = the input's own row stride must stay taken, any other refused).
// On a float64 plan the run is the one the same matcher finds there.  W_LDL=<n> likewise: the l stride of every core of that
// float64 run becomes n (dense network inputs never have an odd one; the cores' own stride must stay taken).
// DESC=1 is no switch either: it appends the `desc=` field below to the line, which is otherwise byte for byte the same.
// For every plan and every setting one line goes to stdout with everything an executor would
// decide when it is created:
//
//   plan <i> set <j> rc=0 roles=<one letter per step: P plain, A absorbed, Z zip, L zip latency form, C complex>
//     forms=[<step>:<ctn_step_form>/zu<zu>/zm<zm>,..] lat=[<step>:mp<mp>/prev<0|1>/next<0|1>/buf<0|1>,..] cplx=[<sp>+<step>,..]
//     partials=<n per step,..> off=<per step,..> slots=<n> scratch=<n>
//     bufs=slab:<n>,fold:<n>,zl:<n>,group:<n>,sweep:<a>/<s>/<z>/<l>/<e>,tabs:<n>
//     sweep=[<member steps,..>]<f32|f64|small2|small1|small2f64|->[/tr: a small run of transposed cores] ares=[<step>:<ntw>,..] dot=[<step>,..] groups=[<head>:<len>,..]
//     side=[<tensor>:<buffer>,..]x<bytes>x<buffers> ok | <the invariant that failed>
//     [DESC=1: desc=in<idIn>/out<idOut>/S<sites>/J<J>/M<M>/D<D>/P<Pd>/ld<In,Out,Wl,Wp,X>/ids<W_1,x_1,..>/offs<..>/slots<..> - what
//      the sweep's launch is given: the descriptor, the id table and the members' partial-sum offsets and slot counts; "desc=-": no sweep]
//
// and these invariants are checked on each: a step's descriptor is on exactly under its role; an absorbed step is
// directly followed by its pair's second member or named by a complex pair's `sp`; step_off is the running sum of
// step_partials (a chain plan: one slot per step); no fused launch has more than kMaxPartials slots; two side buffers of
// k_zipqp_f32 that are live at the same time never share an index; no leaf group holds a sweep member or an absorbed step.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "fused_forms.h"

using namespace ctn;

struct Setting { int R = 1, cu = 256, alias_ld = 0, w_ldl = 0, desc = 0; DevSwitches sw; };

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
    else if (key == "ALIAS_LD") out->alias_ld = v;
    else if (key == "W_LDL") out->w_ldl = v;
    else if (key == "DESC") out->desc = v;
    else if (key == "ZIP") d.zip = v;
    else if (key == "ZIPQ") d.zipq = v;
    else if (key == "ZIPL") d.zipl = v;
    else if (key == "ZIPL_MP") d.zipl_mp = v;
    else if (key == "ZIPL_MAX_R") d.zipl_max_r = v;
    else if (key == "ZIPL64") d.zipl64 = v;
    else if (key == "ZIP128") d.zip128 = v;
    else if (key == "ZIPM64") d.zipm64 = v;
    else if (key == "ZIP512") d.zip512 = v;
    else if (key == "CPLX") d.cplx = v;
    else if (key == "SWEEP") d.sweep = v;
    else if (key == "SWEEP64") d.sweep64 = v;
    else if (key == "SWEEP_SMALL") d.sweep_small = v;
    else if (key == "SWEEP_SMALL64") d.sweep_small64 = v;
    else if (key == "SWEEP_SMALL_TR") d.sweep_small_tr = v;
    else if (key == "GROUP") d.group = v;
    else if (key == "ARES") d.ares = v;
    else if (key == "ARES_NTW") d.ares_ntw = v;
    else if (key == "DOT_TR") d.dot_tr = v;
    else return false;
    p = e + 1;
  }
  return out->R >= 1 && out->cu >= 1;
}

static std::string invariants(const Plan& P, const FusedForms& F) {
  const int n = P.n_steps;
  std::vector<char> named(n, 0);
  for (int s = 0; s < n; ++s)
    if (F.role[s] == Role::Cplx) {
      if (F.cplx[s].sp < 0 || F.cplx[s].sp >= s) return "a complex pair's S step is not before it";
      named[F.cplx[s].sp] = 1;
    }
  int64_t off = 0;
  for (int s = 0; s < n; ++s) {
    const Role r = F.role[s];
    if ((r == Role::Zip) != (!F.zip.empty() && F.zip[s].on) || (r == Role::ZipLat) != (!F.zl.empty() && F.zl[s].on) ||
        (r == Role::Cplx) != (!F.cplx.empty() && F.cplx[s].on))
      return "step " + std::to_string(s) + ": a descriptor is on outside its role";
    if (r == Role::Absorbed) {
      const bool pair = s + 1 < n && (F.role[s + 1] == Role::Zip || F.role[s + 1] == Role::ZipLat);
      if (pair == (bool)named[s]) return "step " + std::to_string(s) + ": absorbed by no launch, or by two";
    } else if (named[s]) {
      return "step " + std::to_string(s) + ": the S step of a complex pair is not absorbed";
    }
    if ((r == Role::Zip || r == Role::ZipLat) && (s < 1 || F.role[s - 1] != Role::Absorbed))
      return "step " + std::to_string(s) + ": a pair without its first step";
    if (r != Role::Plain && r != Role::Absorbed && F.step_partials[s] > kMaxPartials)
      return "step " + std::to_string(s) + ": more slots than kMaxPartials";
    if (F.step_partials[s] < 1 || F.step_off[s] != off) return "step " + std::to_string(s) + ": step_off is not the running sum";
    off += P.chain ? 1 : F.step_partials[s];
  }
  if (off != F.part_slots) return "part_slots is not the sum of the slots";
  if (P.chain)
    for (int s = 0; s < n; ++s)
      if (F.role[s] != Role::Plain || F.sweep_role[s] || F.ares_ntw[s] || F.dot_tr[s].on || F.groups[s].len)
        return "a chain plan with a fused form";
  for (int s = 0; s < n; ++s)
    for (int i = 0; i < F.groups[s].len; ++i)
      if (s + i >= n || F.sweep_role[s + i] || F.role[s + i] == Role::Absorbed)
        return "step " + std::to_string(s + i) + ": in a leaf group and never launched on its own";
  // side buffers: tensor id (the result of pair s, consumed by step c) holds its buffer over steps [s - 1, c]
  struct Live { int k, from, to; };
  std::vector<Live> live;
  for (int s = 1; s < n; ++s) {
    const int id = P.steps[s].out, k = F.zqp_side[id];
    if (k < 0) continue;
    if (F.role[s] != Role::Zip || !F.zip[s].zqp || k >= F.zqp_side_bufs) return "a side buffer outside a k_zipqp_f32 pair";
    if (P.tensors[id].numel * (int64_t)P.elem_size() > F.zqp_side_bytes) return "a side buffer smaller than its tensor";
    int c = n;
    for (int q = s + 1; q < n; ++q)
      if (P.steps[q].lhs == id || P.steps[q].rhs == id || P.steps[q].lhs2 == id) { c = q; break; }
    for (const Live& l : live)
      if (l.k == k && l.from <= c && s - 1 <= l.to) return "two live side buffers share index " + std::to_string(k);
    live.push_back({k, s - 1, c});
  }
  return "ok";
}

// DESC=1: what the launch of the sweep would be given
static std::string sweep_desc(const FusedForms& F) {
  const SweepDesc& sd = F.sweep;
  if (!sd.on) return " desc=-";
  auto list = [](const auto& v) { std::string t; for (auto x : v) t += (t.empty() ? "" : ",") + std::to_string(x); return t; };
  return " desc=in" + std::to_string(sd.idIn) + "/out" + std::to_string(sd.idOut) + "/S" + std::to_string(sd.sites()) + "/J" +
         std::to_string(sd.J) + "/M" + std::to_string(sd.M) + "/D" + std::to_string(sd.D) + "/P" + std::to_string(sd.Pd) + "/ld" +
         list(std::vector<int64_t>{sd.ldIn, sd.ldOut, sd.ldWl, sd.ldWp, sd.ldX}) + "/ids" + list(sd.ids) + "/offs" + list(F.sweep_offs) +
         "/slots" + list(F.sweep_slots);
}

static void print_line(int plan, int set, const Plan& P, const FusedForms& F, bool desc) {
  const int n = P.n_steps;
  std::string roles, forms, lat, cplx, partials, offs, sweep, ares, dot, groups, side;
  auto item = [](std::string* to, const std::string& s) { *to += (to->empty() ? "" : ",") + s; };
  for (int s = 0; s < n; ++s) {
    roles += "PAZLC"[(int)F.role[s]];
    if (F.role[s] == Role::Zip)
      item(&forms, std::to_string(s) + ":" + std::to_string(F.zip[s].form) + "/zu" + std::to_string(F.zip[s].zu) + "/zm" + std::to_string(F.zip[s].zm));
    if (F.role[s] == Role::ZipLat)
      item(&lat, std::to_string(s) + ":mp" + std::to_string(F.zl[s].mp) + "/prev" + std::to_string(F.zl[s].from_prev) + "/next" +
                     std::to_string(F.zl[s].feeds_next) + "/buf" + std::to_string(F.zl[s].buf));
    if (F.role[s] == Role::Cplx) item(&cplx, std::to_string(F.cplx[s].sp) + "+" + std::to_string(s));
    item(&partials, std::to_string(F.step_partials[s]));
    item(&offs, std::to_string(F.step_off[s]));
    if (F.ares_ntw[s]) item(&ares, std::to_string(s) + ":" + std::to_string(F.ares_ntw[s]));
    if (F.dot_tr[s].on) item(&dot, std::to_string(s));
    if (F.groups[s].len) item(&groups, std::to_string(s) + ":" + std::to_string(F.groups[s].len));
  }
  for (int s : F.sweep.steps) item(&sweep, std::to_string(s));
  for (size_t id = 0; id < F.zqp_side.size(); ++id)
    if (F.zqp_side[id] >= 0) item(&side, std::to_string(id) + ":" + std::to_string(F.zqp_side[id]));
  printf("plan %d set %d rc=0 roles=%s forms=[%s] lat=[%s] cplx=[%s] partials=%s off=%s slots=%lld scratch=%lld "
         "bufs=slab:%zu,fold:%zu,zl:%lld,group:%d,sweep:%zu/%zu/%zu/%zu/%zu,tabs:%zu sweep=[%s]%s ares=[%s] dot=[%s] groups=[%s] "
         "side=[%s]x%lldx%d %s%s\n",
         plan, set, roles.c_str(), forms.c_str(), lat.c_str(), cplx.c_str(), partials.c_str(), offs.c_str(), (long long)F.part_slots,
         (long long)F.scratch_need, F.slab_elems, F.fold_elems, (long long)F.zl_slab_elems, F.group_args, F.sweep_a, F.sweep_s,
         F.sweep_z, F.sweep_l, F.sweep_e, F.cplx_tabs.size(), sweep.c_str(), F.sweep.on && F.sweep.tr ? (F.sweep.f64 ? "small2f64/tr" : F.sweep.two ? "small2/tr" : "small1/tr") : !F.sweep.on ? "-" : F.sweep.small ? (F.sweep.f64 ? "small2f64" : F.sweep.two ? "small2" : "small1") : F.sweep.f64 ? "f64" : "f32",
         ares.c_str(), dot.c_str(), groups.c_str(), side.c_str(), (long long)F.zqp_side_bytes, F.zqp_side_bufs,
         invariants(P, F).c_str(), desc ? sweep_desc(F).c_str() : "");
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
      // (a small-bond sweep that is asked for takes a chain plan from the chain walker: the executor's own first decision)
      Plan Q = sweep_small_unchains(P, sets[j].R, sets[j].cu, sets[j].sw) ? unchained(P) : P;
      SweepDesc sd;
      const bool found = sweep_small_match(Q, &sd, sets[j].sw.sweep_small_tr != 0);
      if (sets[j].w_ldl > 0 && found && sd.f64)
        for (size_t i = 0; i < sd.ids.size(); i += 2) {
          Tensor& core = Q.tensors[sd.ids[i]];
          for (int64_t& st : core.strides) if (st == sd.ldWl) st = sets[j].w_ldl;
        }
      if (sets[j].alias_ld > 0 && found && sd.two && sd.idIn >= Q.n_inputs) {
        Tensor& out = Q.tensors[Q.steps[sd.steps.back()].out];
        out.ws_offset = Q.tensors[sd.idIn].ws_offset;
        for (int64_t& st : out.strides) if (st != 1) st = sets[j].alias_ld;
      }
      const FusedForms F = fused_forms(Q, sets[j].R, sets[j].cu, sets[j].sw);
      if (invariants(Q, F) != "ok") ++n_fail;
      print_line(n_plans, (int)j, Q, F, sets[j].desc != 0);
    }
  }
  return n_fail ? 1 : 0;
}
