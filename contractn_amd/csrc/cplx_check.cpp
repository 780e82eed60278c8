// cplx_check.cpp - host-only driver of cplx_match (cplx_match.h), for sanitizer runs on the CPU.
//
//   make -C contractn_amd/csrc cplx_check   ->  ../lib/cplx_check_asan   (-fsanitize=address,undefined)
//   cplx_check_asan < plans.txt             (the input format of plan_check.cpp; fp32 plans)
//
// For every plan, every step pair the matcher takes is replayed on the CPU with the offsets k_cmfma_f32 uses INSIDE each
// tensor: through the pair-granular tables, padding included (every padded entry must stay inside its tensor, as the
// kernel loads from it unconditionally), with eight distinct integers in S.  The replay keeps every tensor in a host
// vector of its own, so it says nothing about WHERE the tensors lie in the workspace; that is checked separately
// (`workspace_clear`): the regions of `small` and `big` of a taken pair must not meet the result of any step between
// the S step and the GEMM, the GEMM's own included - the arena has released `small` by then.  The result is compared, element by element and
// exactly (small integers in doubles), with the two plan steps evaluated as the planner states them: `mid` from the
// LABELS of `small`, S and mid, then step s through its own m / n / k tables.  Pairs whose replay would take more than
// `kMaxWork` multiply-adds are only checked for bounds.  One line per plan: the pairs taken (S step + GEMM step), the
// GEMM steps refused for that aliasing alone, and `ok` or what failed.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "cplx_match.h"
#include "plan.h"

using namespace ctn;

static const int64_t kMaxWork = 1 << 24;

static bool replay(const Plan& P, int s, const CplxDesc& d, const std::vector<int32_t>& tabs, std::string* why) {
  const Step& g = P.steps[s];
  const Tensor &TS = P.tensors[d.sid], &Tx = P.tensors[d.small], &Ty = P.tensors[d.big], &Tm = P.tensors[P.steps[d.sp].out],
               &Tc = P.tensors[g.out];
  const int32_t *txr = tabs.data() + d.txr, *txk = tabs.data() + d.txk, *tyn = tabs.data() + d.tyn, *tyk = tabs.data() + d.tyk,
                *tcx = tabs.data() + d.tcx, *tcy = tabs.data() + d.tcy;
  auto up = [](int64_t n, int64_t m) { return (n + m - 1) / m * m; };
  const int64_t padX = up(d.Mx, CX_TX), padY = up(d.Ny, CX_TY), padK = up(d.Kc, CX_BK) + 2 * CX_BK;
  // bounds of everything a workgroup may touch: loads use the padded entries too, stores only the valid ones
  for (int64_t i = 0; i < padX; ++i)
    for (int64_t k = 0; k < padK; ++k) {
      const int64_t off = (int64_t)txr[i] + txk[k];
      if (off < 0 || off + d.legx >= Tx.numel || (d.legx == 1 && off % 2)) { *why = "small: address out of range or odd"; return false; }
      if (i >= d.Mx && txr[i] != 0) { *why = "small: padding not zero"; return false; }
    }
  for (int64_t n = 0; n < padY; ++n)
    for (int64_t k = 0; k < padK; ++k) {
      const int64_t off = (int64_t)tyn[n] + tyk[k];
      if (off < 0 || off + d.legy >= Ty.numel || (d.legy == 1 && off % 2)) { *why = "big: address out of range or odd"; return false; }
    }
  for (int64_t i = 0; i < d.Mx; ++i)
    for (int64_t n = 0; n < d.Ny; ++n) {
      const int64_t off = (int64_t)tcx[i] + tcy[n];
      if (off < 0 || off >= Tc.numel || off + d.sO < 0 || off + d.sO >= Tc.numel) { *why = "C: address out of range"; return false; }
      if (d.cvec2 && (off % 2 || d.sO != 1)) { *why = "C: 8-byte store not aligned"; return false; }
    }
  for (int v : {0, d.sa, d.sb, d.so, d.sa + d.sb + d.so})
    if (v < 0 || v >= 8) { *why = "S: stride out of range"; return false; }
  if ((int64_t)d.Mx * d.Ny * d.Kc * 8 > kMaxWork) return true;

  std::vector<double> X((size_t)Tx.numel), Y((size_t)Ty.numel), S(8), M((size_t)Tm.numel, 0.0), C((size_t)Tc.numel, 0.0), Cr((size_t)Tc.numel, 0.0);
  uint32_t rng = 12345u + (uint32_t)s;
  auto next = [&]() { rng = rng * 1664525u + 1013904223u; return (double)((int)((rng >> 20) % 7) - 3); };
  for (auto& v : X) v = next();
  for (auto& v : Y) v = next();
  for (int i = 0; i < 8; ++i) S[(size_t)i] = (double)(i + 2) * (i % 2 ? -1 : 1);   // eight distinct values
  // the fused form, as the kernel addresses it
  for (int64_t i = 0; i < d.Mx; ++i)
    for (int64_t n = 0; n < d.Ny; ++n)
      for (int o = 0; o < 2; ++o) {
        double acc = 0;
        for (int64_t k = 0; k < d.Kc; ++k)
          for (int b = 0; b < 2; ++b) {
            const double* x = &X[(size_t)(txr[i] + txk[k])];
            const double mid = S[(size_t)(b * d.sb + o * d.so)] * x[0] + S[(size_t)(d.sa + b * d.sb + o * d.so)] * x[d.legx];
            acc += mid * Y[(size_t)(tyn[n] + tyk[k] + b * d.legy)];
          }
        C[(size_t)(tcx[i] + tcy[n] + o * d.sO)] = acc;
      }
  // the two plan steps: mid by labels ...
  auto pos = [](const Tensor& t, int32_t lab) {
    for (size_t i = 0; i < t.labels.size(); ++i) if (t.labels[i] == lab) return (int)i;
    return -1;
  };
  int32_t xs = -1;
  for (int32_t lab : TS.labels) if (pos(Tx, lab) >= 0) xs = lab;
  std::vector<int64_t> idx(Tm.labels.size(), 0);
  for (int64_t e = 0; e < Tm.numel; ++e) {
    int64_t om = 0, ox = 0, os = 0;
    for (size_t a = 0; a < Tm.labels.size(); ++a) {
      om += idx[a] * Tm.strides[a];
      const int px = pos(Tx, Tm.labels[a]), psx = pos(TS, Tm.labels[a]);
      if (px >= 0) ox += idx[a] * Tx.strides[(size_t)px];
      if (psx >= 0) os += idx[a] * TS.strides[(size_t)psx];
    }
    double v = 0;
    for (int a2 = 0; a2 < 2; ++a2)
      v += X[(size_t)(ox + a2 * Tx.strides[(size_t)pos(Tx, xs)])] * S[(size_t)(os + a2 * TS.strides[(size_t)pos(TS, xs)])];
    M[(size_t)om] = v;
    for (int a = (int)idx.size() - 1; a >= 0; --a) { if (++idx[(size_t)a] < Tm.dims[(size_t)a]) break; idx[(size_t)a] = 0; }
  }
  // ... then step s through its own tables
  const int32_t* T = P.tables.data();
  const std::vector<double>& A = g.lhs == P.steps[d.sp].out ? M : Y;
  const std::vector<double>& B = g.lhs == P.steps[d.sp].out ? Y : M;
  for (int64_t m = 0; m < g.M; ++m)
    for (int64_t n = 0; n < g.N; ++n) {
      double acc = 0;
      for (int64_t k = 0; k < g.K; ++k)
        acc += A[(size_t)(T[g.t.omA + m] + T[g.t.okA + k])] * B[(size_t)(T[g.t.onB + n] + T[g.t.okB + k])];
      Cr[(size_t)(T[g.t.omC + m] + T[g.t.onC + n])] = acc;
    }
  for (size_t e = 0; e < C.size(); ++e)
    if (C[e] != Cr[e]) { *why = "fused result differs from the two steps at element " + std::to_string(e); return false; }
  return true;
}

// the workspace bytes of tensor `id` ([0, 0) for a network input or the final result: the caller's buffers)
static void ws_range(const Plan& P, int id, int64_t* b0, int64_t* b1) {
  *b0 = *b1 = 0;
  if (id < P.n_inputs || id >= P.n_inputs + P.n_steps - 1) return;
  *b0 = P.tensors[id].ws_offset;
  *b1 = *b0 + P.tensors[id].numel * (int64_t)P.elem_size();
}

// no result written in (sp, s] lies on an operand the fused launch of step s reads
static bool workspace_clear(const Plan& P, int s, const CplxDesc& d) {
  for (int id : {d.small, d.big}) {
    int64_t a0, a1;
    ws_range(P, id, &a0, &a1);
    const int born = id >= P.n_inputs ? P.tensors[id].producer : -1;     // (results before its own producer: not its concern)
    for (int q = std::max(d.sp, born) + 1; q <= s; ++q) {
      int64_t b0, b1;
      ws_range(P, P.steps[q].out, &b0, &b1);
      if (a0 < b1 && b0 < a1) return false;
    }
  }
  return true;
}

int main() {
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
    in_dims.push_back(0); in_labels.push_back(0); olab.push_back(0);
    d.in_ndim = in_ndim.data(); d.in_dims = in_dims.data(); d.in_labels = in_labels.data(); d.in_strides = nullptr;
    d.step_lhs = lhs.data(); d.step_rhs = rhs.data(); d.step_out_ndim = ond.data(); d.step_out_labels = olab.data();
    d.stabilize = 1; d.min_norm = 1e-7;
    Plan P;
    std::string err;
    const int rc = build_plan(d, P, err);
    ++n_plans;
    if (rc != CTN_OK) { printf("plan %d rc=%d %s\n", n_plans, rc, err.c_str()); continue; }
    std::vector<int32_t> tabs;
    std::string taken, aliased, why;
    bool ok = true;
    for (int s = 1; s < P.n_steps && ok; ++s) {
      CplxDesc cd;
      const size_t before = tabs.size();
      if (!cplx_match(P, s, &cd, &tabs)) {
        if (tabs.size() != before) { ok = false; why = "a refused pair left tables behind"; }
        if (cd.aliased) aliased += (aliased.empty() ? "" : ",") + std::to_string(s);
        continue;
      }
      taken += (taken.empty() ? "" : ",") + std::to_string(cd.sp) + "+" + std::to_string(s);
      ok = replay(P, s, cd, tabs, &why);
      if (ok && !workspace_clear(P, s, cd)) { ok = false; why = "an operand of the fused launch lies where a result is written"; }
      if (!ok) why = "pair " + std::to_string(s) + ": " + why;
    }
    if (!ok) ++n_fail;
    printf("plan %d rc=0 pairs=[%s] aliased=[%s] %s\n", n_plans, taken.c_str(), aliased.c_str(), ok ? "ok" : why.c_str());
  }
  return n_fail ? 1 : 0;
}
