// cplx_match.h - finds the complex x complex step pairs of a plan that k_cmfma_f32 (kernels_cmfma.h) runs as one launch
// and builds their pair-granular offset tables.  Pure host code (no HIP), on the plan's own tables and tensor records:
// engine.hip calls it when an executor is created, cplx_check.cpp drives it on the CPU under a sanitizer.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "plan.h"

namespace ctn {

// k_cmfma_f32's workgroup tile: CX_TX pairs of `small` x CX_TY entries of `big`'s free group, k-tiles of CX_BK pairs
constexpr int CX_TX = 64, CX_TY = 128, CX_BK = 16;

// the fused launch of step s with the S step sp; t*: offsets of the tables inside the vector cplx_match appends them to
struct CplxDesc {
  bool on = false, mid_is_a = false, kfx = false, kfy = false, cvec2 = false;
  int small = -1, big = -1, sid = -1, Mx = 0, Ny = 0, Kc = 0, sa = 0, sb = 0, so = 0, sO = 0;
  int sp = -1;              // the S step: the producer of mid (step s - 1, or earlier where the leaf steps were moved to the front)
  bool aliased = false;     // set on a REFUSED pair: everything matched, but `small`'s workspace region is written before the launch ends
  int legx = 1, legy = 1;   // strides of the legs of `small` and `big`: 1 = an array of (re, im) pairs, read 8 bytes at a time
  int64_t txr = 0, txk = 0, tyn = 0, tyk = 0, tcx = 0, tcy = 0;
};

// Do step s and the step that produces one of its operands form a complex x complex step that k_cmfma_f32 can run as
// one launch?  The producer (step s - 1 as lowered; earlier where Plan moved the leaf steps to the front) contracts a
// 2 x 2 x 2 network input S into `small` (a streaming step, K = 2, N = 4) and step s, a plain fp32 GEMM, is the only
// consumer of the result `mid`.  Which label is which is read off the tensors that carry it, nothing else: of S's three
// labels, the one `small` carries is summed in the S step, the one `big` carries is contracted in step s, the third is
// free.  An operand that is an array of pairs (stride 1 along its leg, even strides elsewhere: every network input) is
// read 8 bytes at a time; any other leg stride - an earlier step's result keeps its leg between the row and the column
// group - is read as two 4-byte loads that distance apart (legx / legy).  The tables of
// step s must enumerate the pairs next to each other - entries (2 i, 2 i + 1) of mid's free group differ by o alone,
// entries (2 j, 2 j + 1) of the contracted group by b alone - which is what the planner's stride order gives; any
// other order is refused.  On success the pair-granular tables are appended to `tabs`: every even entry of mid's two
// tables decoded (through mid's dims and strides) into the offset of the same element in `small`, the even entries of
// big's contracted group and of C's group on mid's side, and big's free and C's other group as they are - each padded
// with zeros as the kernel's loaders expect.  A pair whose `small` lies where a later result is written is refused
// (CplxDesc::aliased), see below.
inline bool cplx_match_mid(const Plan& P, int s, int mid, CplxDesc* d, std::vector<int32_t>* tabs) {
  const Step& g = P.steps[s];
  if (mid < P.n_inputs) return false;
  const int sp = P.tensors[mid].producer;
  if (sp < 0 || sp >= s) return false;
  const Step& a = P.steps[sp];
  if (a.kernel != CTN_KERNEL_ELEMENT || a.Bt != 1 || a.K != 2 || a.N != 4 || a.rhs < 0 || a.lhs2 >= 0 || a.epw || a.out != mid) return false;
  if ((g.lhs == mid) == (g.rhs == mid)) return false;
  for (int q = 0; q < P.n_steps; ++q)
    if (q != s && (P.steps[q].lhs == mid || P.steps[q].rhs == mid || P.steps[q].lhs2 == mid)) return false;
  auto is_s = [&](int id) {
    const Tensor& t = P.tensors[id];
    return id < P.n_inputs && t.dims.size() == 3 && t.dims[0] == 2 && t.dims[1] == 2 && t.dims[2] == 2;
  };
  if (is_s(a.lhs) == is_s(a.rhs)) return false;
  const int sid = is_s(a.lhs) ? a.lhs : a.rhs, small = is_s(a.lhs) ? a.rhs : a.lhs;
  const bool mid_is_a = g.lhs == mid;
  const int big = mid_is_a ? g.rhs : g.lhs;
  if (big == small || big == sid) return false;
  const Tensor &TS = P.tensors[sid], &Tx = P.tensors[small], &Ty = P.tensors[big], &Tm = P.tensors[mid], &Tc = P.tensors[g.out];
  auto pos = [](const Tensor& t, int32_t lab) {
    for (size_t i = 0; i < t.labels.size(); ++i) if (t.labels[i] == lab) return (int)i;
    return -1;
  };
  for (const Tensor* t : {&TS, &Tx, &Ty, &Tm, &Tc})
    for (size_t i = 0; i < t->labels.size(); ++i)
      for (size_t j = i + 1; j < t->labels.size(); ++j) if (t->labels[i] == t->labels[j]) return false;   // no diagonals
  int ps = -1, pb = -1, po = -1;   // positions in S of the legs of `small`, of `big`, and of the free one
  for (int i = 0; i < 3; ++i) {
    const int32_t lab = TS.labels[i];
    const bool inX = pos(Tx, lab) >= 0, inY = pos(Ty, lab) >= 0, inM = pos(Tm, lab) >= 0, inC = pos(Tc, lab) >= 0;
    if (inX && !inM && !inY && !inC && ps < 0) ps = i;
    else if (!inX && inM && inY && !inC && pb < 0) pb = i;
    else if (!inX && inM && !inY && inC && po < 0) po = i;
    else return false;
  }
  if (ps < 0 || pb < 0 || po < 0) return false;
  const int32_t xs = TS.labels[ps], xb = TS.labels[pb], xo = TS.labels[po];
  if (Tm.labels.size() != Tx.labels.size() + 1) return false;
  for (int32_t lab : Tx.labels) if (lab != xs && pos(Tm, lab) < 0) return false;
  // `small` is read by the fused launch at step s, but the plan's arena released it right after the S step (its only
  // consumer as planned): the result of any step launched in (sp, s] - that of step s itself, C, included, which the
  // same launch writes from other workgroups while `small` is still being loaded - may have been given its region.
  // Such a pair keeps its two launches.  (`big` is an operand of step s itself and lives until that step is done.)
  if (small >= P.n_inputs) {
    const int64_t es = (int64_t)P.elem_size();
    const int64_t a0 = Tx.ws_offset, a1 = a0 + Tx.numel * es;
    for (int q = sp + 1; q <= s; ++q) {
      const int oq = P.steps[q].out;
      if (P.steps[q].kernel == CTN_KERNEL_FUSED || oq >= P.n_inputs + P.n_steps - 1) continue;   // nothing written / the caller's buffer
      const int64_t b0 = P.tensors[oq].ws_offset, b1 = b0 + P.tensors[oq].numel * es;
      if (a0 < b1 && b0 < a1) { d->aliased = true; return false; }
    }
  }
  const int64_t legx = Tx.strides[(size_t)pos(Tx, xs)], legy = Ty.strides[(size_t)pos(Ty, xb)];
  if (legx < 1 || legy < 1 || legx >= (1LL << 31) || legy >= (1LL << 31)) return false;
  if (Tx.dims[(size_t)pos(Tx, xs)] != 2 || Ty.dims[(size_t)pos(Ty, xb)] != 2) return false;
  bool pairx = legx == 1, pairy = legy == 1;   // 8-byte loads: every other stride even (checked on the tables below)
  if (P.tables64[g.t.obA] != 0 || P.tables64[g.t.obB] != 0 || P.tables64[g.t.obC] != 0) return false;
  const int32_t* T = P.tables.data();
  const int32_t *fm = T + (mid_is_a ? g.t.omA : g.t.onB), *km = T + (mid_is_a ? g.t.okA : g.t.okB);
  const int32_t *fb = T + (mid_is_a ? g.t.onB : g.t.omA), *kb = T + (mid_is_a ? g.t.okB : g.t.okA);
  const int32_t *cm = T + (mid_is_a ? g.t.omC : g.t.onC), *cb = T + (mid_is_a ? g.t.onC : g.t.omC);
  const int64_t Fm = mid_is_a ? g.M : g.N, Fb = mid_is_a ? g.N : g.M, K = g.K;
  if (Fm % 2 != 0 || K % 2 != 0 || Fm < 2 || K < 2 || Fb < 1) return false;
  const int mpb = pos(Tm, xb), mpo = pos(Tm, xo);
  // an offset inside mid (its (b, o) part zero) -> the offset of the same element of `small`
  auto decode = [&](int64_t v, int64_t* off) {
    int64_t back = 0;
    *off = 0;
    if (v < 0 || v >= Tm.numel) return false;
    for (size_t i = 0; i < Tm.labels.size(); ++i) {
      if (Tm.strides[i] <= 0) return false;
      const int64_t c = (v / Tm.strides[i]) % Tm.dims[i];
      back += c * Tm.strides[i];
      if ((int)i == mpb || (int)i == mpo) { if (c != 0) return false; continue; }
      *off += c * Tx.strides[(size_t)pos(Tx, Tm.labels[i])];
    }
    return back == v;
  };
  const int64_t Mx = Fm / 2, Kc = K / 2;
  std::vector<int32_t> xr((size_t)Mx), xk((size_t)Kc), yk((size_t)Kc), cx((size_t)Mx);
  const int64_t sO = (int64_t)cm[1] - cm[0];
  if (sO == 0) return false;
  bool cvec2 = sO == 1;
  for (int64_t i = 0; i < Mx; ++i) {
    int64_t off;
    if (fm[2 * i + 1] != fm[2 * i] + Tm.strides[(size_t)mpo] || !decode(fm[2 * i], &off)) return false;
    if ((int64_t)cm[2 * i + 1] - cm[2 * i] != sO) return false;
    xr[(size_t)i] = (int32_t)off;
    pairx = pairx && off % 2 == 0;
    cx[(size_t)i] = cm[2 * i];
    cvec2 = cvec2 && cm[2 * i] % 2 == 0;
  }
  for (int64_t j = 0; j < Kc; ++j) {
    int64_t off;
    if (km[2 * j + 1] != km[2 * j] + Tm.strides[(size_t)mpb] || !decode(km[2 * j], &off)) return false;
    if (kb[2 * j + 1] != kb[2 * j] + legy) return false;
    pairx = pairx && off % 2 == 0;
    pairy = pairy && kb[2 * j] % 2 == 0;
    xk[(size_t)j] = (int32_t)off;
    yk[(size_t)j] = kb[2 * j];
  }
  for (int64_t n = 0; n < Fb; ++n) {
    pairy = pairy && fb[n] % 2 == 0;
    cvec2 = cvec2 && cb[n] % 2 == 0;
  }
  if (legx == 1 && !pairx) return false;   // (a unit-stride leg at odd offsets: no planner layout gives it)
  if (legy == 1 && !pairy) return false;
  // which index runs along the lanes of a load: the k pairs when more of them than of the rows are dense
  auto dense = [](const int32_t* t, int64_t n, int step) {
    int64_t c = 0;
    for (int64_t i = 0; i + 1 < n; ++i) c += t[i + 1] - t[i] == step;
    return n > 1 ? (double)c / (double)(n - 1) : 0.0;
  };
  d->kfx = dense(xk.data(), Kc, pairx ? 2 : 1) > dense(xr.data(), Mx, pairx ? 2 : 1);
  d->kfy = dense(yk.data(), Kc, pairy ? 2 : 1) > dense(fb, Fb, pairy ? 2 : 1);
  d->legx = (int)legx; d->legy = (int)legy;
  auto emit = [&](const int32_t* src, int64_t n, int64_t padded) {
    const int64_t off = (int64_t)tabs->size();
    tabs->resize((size_t)(off + padded), 0);
    std::copy(src, src + n, tabs->begin() + off);
    return off;
  };
  auto up = [](int64_t n, int64_t m) { return (n + m - 1) / m * m; };
  d->txr = emit(xr.data(), Mx, up(Mx, CX_TX));
  d->txk = emit(xk.data(), Kc, up(Kc, CX_BK) + 2 * CX_BK);   // the loaders ask for table entries two tiles ahead
  d->tyn = emit(fb, Fb, up(Fb, CX_TY));
  d->tyk = emit(yk.data(), Kc, up(Kc, CX_BK) + 2 * CX_BK);
  d->tcx = emit(cx.data(), Mx, up(Mx, CX_TX));
  d->tcy = emit(cb, Fb, up(Fb, CX_TY));
  d->on = true; d->aliased = false; d->mid_is_a = mid_is_a; d->cvec2 = cvec2;
  d->small = small; d->big = big; d->sid = sid; d->sp = sp;
  d->Mx = (int)Mx; d->Ny = (int)Fb; d->Kc = (int)Kc;
  d->sa = (int)TS.strides[(size_t)ps]; d->sb = (int)TS.strides[(size_t)pb]; d->so = (int)TS.strides[(size_t)po];
  d->sO = (int)sO;
  return true;
}

inline bool cplx_match(const Plan& P, int s, CplxDesc* d, std::vector<int32_t>* tabs) {
  if (s < 1 || s >= P.n_steps || P.dtype != CTN_F32) return false;
  const Step& g = P.steps[s];
  if (g.kernel != CTN_KERNEL_MFMA_F32 || g.Bt != 1 || g.rhs < 0 || g.lhs2 >= 0 || g.epw) return false;
  return cplx_match_mid(P, s, g.lhs, d, tabs) || cplx_match_mid(P, s, g.rhs, d, tabs);
}

}  // namespace ctn
