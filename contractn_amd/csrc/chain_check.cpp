// chain_check.cpp - host-only driver of chain_pack (chain_pack.h), for sanitizer runs on the CPU.
//
//   make -C contractn_amd/csrc chain_check   ->  ../lib/chain_check_asan   (-fsanitize=address,undefined)
//   chain_check_asan < plans.txt
//
// Input, one description per plan (plan_check.cpp's format with strides and one directive):
//
//   plan <dtype 0|1> <n_inputs> <n_steps> <force: -1 | step whose kernel is set to CTN_KERNEL_FUSED after planning>
//   in <ndim> <dim>*ndim <label>*ndim  |  ins <ndim> <dim>*ndim <label>*ndim <stride>*ndim     (n_inputs lines)
//   step <lhs> <rhs|-1> <out_ndim> <label>*out_ndim                                            (n_steps lines)
//
// For every plan the packed program is replayed on the CPU exactly as k_chain_lds (kernels_chain.h) addresses memory:
// a ring of kClRing slots of kClSlotWords words and an arena of kClArenaBytes as plain arrays, one array per tensor for
// global memory, and the kernel's own iteration: stage R (record s + 3), P (pointers of s + 2), D (images of s + 1), then
// step s, through the records' (base, stride) pairs and explicit tables only.  Elements are unsigned integers of the
// dtype's size with wrapping arithmetic, so long chains stay exact; "dividing by the producer's scale" is modelled as a
// multiplication by an odd constant per producing step, which shows a division applied twice or not at all.  Every
// step's result, read from the home the program gave it, is compared EXACTLY with the step evaluated from the plan's own
// padded tables on one array per tensor.  Along the way the replay asserts what the kernel relies on:
//   * a slot is refilled only when the step that owned it has ended, and poisoned before the refill;
//   * a stage reads only what an earlier iteration completed (R before P before D before the step itself);
//   * every LDS offset lies inside its slot or the arena, and no two live tensors overlap in the arena.
// One line per plan: `chain=0` for a plan that is no chain plan, `refused: <reason>`, or the counts and `ok` / what failed.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "chain_pack.h"
#include "plan.h"

using namespace ctn;

namespace {

struct Fail { std::string why; };
#define CHECK(cond, msg) do { if (!(cond)) throw Fail{std::string(msg) + " (step " + std::to_string(s) + ")"}; } while (0)

template <typename U>
struct Replay {
  const Plan& P;
  const ChainProgram& cp;
  std::vector<std::vector<U>> glob;   // "global memory": the caller's tensors and the workspace slots, by tensor id
  std::vector<std::vector<U>> ref;    // the plan evaluated by its own tables
  std::vector<int32_t> ring;          // [kClRing][kClSlotWords]
  std::vector<unsigned char> arena;
  int owner[kClRing], r_done[kClRing], p_done[kClRing], d_done[kClRing];
  struct Live { int64_t off, bytes; int id; };
  std::vector<Live> live;
  int explicit_tabs = 0;

  Replay(const Plan& p, const ChainProgram& c) : P(p), cp(c) {
    const size_t nt = P.tensors.size();
    glob.resize(nt + 1); ref.resize(nt + 1);
    uint32_t rng = 2463534242u;
    for (size_t id = 0; id < nt; ++id) {
      glob[id].assign((size_t)std::max<int64_t>(P.tensors[id].numel, 1), (U)0xA5A5A5A5u);
      if ((int)id < P.n_inputs) {
        // a strided input spans more than numel elements
        int64_t span = 1;
        for (size_t a = 0; a < P.tensors[id].dims.size(); ++a) span += (P.tensors[id].dims[a] - 1) * P.tensors[id].strides[a];
        glob[id].assign((size_t)std::max<int64_t>(span, 1), 0);
        for (auto& v : glob[id]) { rng ^= rng << 13; rng ^= rng >> 17; rng ^= rng << 5; v = (U)(int64_t)((int)(rng % 7) - 3); }
      }
      ref[id] = glob[id];
    }
    glob[nt].assign(1, (U)1); ref[nt].assign(1, (U)1);   // the ones scalar of unary steps
    ring.assign((size_t)kClRing * kClSlotWords, 0x7f7f7f7f);
    arena.assign((size_t)kClArenaBytes, 0xEE);
    for (int i = 0; i < kClRing; ++i) owner[i] = r_done[i] = p_done[i] = d_done[i] = -1000;
  }

  static U scale_of(int prod) { return prod < 0 ? (U)1 : (U)(2 * (uint32_t)prod + 3); }

  int32_t* slot(int st) { return ring.data() + (size_t)(st & (kClRing - 1)) * kClSlotWords; }
  static ClRec header(const int32_t* rec) { ClRec r; memcpy(&r, rec, sizeof r); return r; }

  int tab(const int32_t* rec, const ClTab& t, int64_t i, int64_t n, int len, int s) {
    CHECK(i >= 0 && i < n, "table index out of range");
    if (t.pos < 0) return t.base + (int32_t)i * t.stride;
    CHECK(t.pos >= kClHeaderWords && t.pos + n <= len, "explicit table outside the record");
    return rec[t.pos + i];
  }

  // an element of an operand or of the result, wherever the record says it lives
  U* at(const ClRec& c, int32_t* rec, int which, int64_t off, int s) {
    const int home = which == 0 ? c.homeA : which == 1 ? c.homeB : c.homeC;
    const int loc = which == 0 ? c.locA : which == 1 ? c.locB : c.locC;
    const int id = which == 0 ? c.idA : which == 1 ? c.idB : c.idC;
    if (home == CL_HOME_ARENA) {
      const int64_t numel = P.tensors[(size_t)id].numel;
      CHECK(off >= 0 && off < numel, "arena element outside its tensor");
      CHECK(loc >= 0 && loc % kClArenaAlign == 0 && loc + numel * (int64_t)sizeof(U) <= kClArenaBytes, "arena tensor outside the budget");
      return reinterpret_cast<U*>(arena.data() + loc) + off;
    }
    if (home == CL_HOME_IMAGE) {
      const int64_t n = which == 0 ? c.imgA : c.imgB;
      CHECK(which < 2 && off >= 0 && off < n, "image element outside the image");
      return reinterpret_cast<U*>(rec + loc) + off;
    }
    if (home == CL_HOME_ONE) { CHECK(which == 1 && off == 0, "the ones scalar addressed past its element"); return &glob[P.tensors.size()][0]; }
    const uint64_t p = c.ptr[which];                       // stage P wrote tensor id + 1 where the kernel has the address
    CHECK(p == (uint64_t)id + 1, "pointer not the one stage P looked up");
    CHECK(off >= 0 && off < (int64_t)glob[(size_t)id].size(), "global element outside its tensor");
    return &glob[(size_t)id][(size_t)off];
  }

  void run(int len0) {
    const int n = P.n_steps;
    for (int s = -kClD; s < n; ++s) {
      const int sr = s + 3, sp = s + 2, sd = s + 1;
      if (sr < n) {                                                            // R
        int off = 0, len = len0;
        if (sr > 0) {
          CHECK(owner[(sr - 1) & (kClRing - 1)] == sr - 1 && r_done[(sr - 1) & (kClRing - 1)] < s, "record before this one not complete");
          const ClRec p = header(slot(sr - 1));
          off = p.next_off; len = p.next_len;
        }
        CHECK(off == cp.steps[(size_t)sr].off && len == cp.steps[(size_t)sr].len, "record chain broken");
        CHECK(len >= kClHeaderWords && len <= kClSlotWords && (size_t)off + (size_t)len <= cp.words.size(), "record outside the slot or the program");
        const int sl = sr & (kClRing - 1);
        CHECK(owner[sl] < s, "slot refilled before its last reader's step has ended");
        std::fill(slot(sr), slot(sr) + kClSlotWords, 0x7f7f7f7f);
        memcpy(slot(sr), cp.words.data() + off, (size_t)len * 4);
        owner[sl] = sr; r_done[sl] = s; p_done[sl] = d_done[sl] = 1 << 30;
      }
      if (sp >= 0 && sp < n) {                                                 // P
        const int sl = sp & (kClRing - 1);
        CHECK(owner[sl] == sp && r_done[sl] < s, "pointers looked up before the record is complete");
        ClRec p = header(slot(sp));
        const int ids[3] = {p.idA, p.idB, p.idC};
        for (int i = 0; i < 3; ++i) {
          CHECK(ids[i] >= 0 && ids[i] <= (int)P.tensors.size(), "tensor id outside the pointer table");
          p.ptr[i] = (uint64_t)ids[i] + 1;
        }
        memcpy(reinterpret_cast<char*>(slot(sp)) + offsetof(ClRec, ptr), p.ptr, sizeof p.ptr);
        p_done[sl] = s;
      }
      if (sd >= 0 && sd < n) {                                                 // D
        const int sl = sd & (kClRing - 1);
        CHECK(owner[sl] == sd && p_done[sl] < s, "images gathered before the pointers are there");
        int32_t* drec = slot(sd);
        const ClRec p = header(drec);
        const int len = cp.steps[(size_t)sd].len;
        int64_t used = len;
        for (int w = 0; w < 2; ++w) {
          const int64_t cnt = w == 0 ? p.imgA : p.imgB;
          if (cnt == 0) continue;
          const int loc = w == 0 ? p.locA : p.locB, id = w == 0 ? p.idA : p.idB;
          CHECK((w == 0 ? p.homeA : p.homeB) == CL_HOME_IMAGE && id < P.n_inputs, "an image of something that is no staged input");
          CHECK(cnt == (int64_t)p.Bt * (w == 0 ? p.M : p.N) * p.K, "image size");
          CHECK(loc >= used && loc % 4 == 0 && loc * 4 + cnt * (int64_t)sizeof(U) <= (int64_t)kClSlotWords * 4, "image outside the slot or over the record");
          used = loc + (cnt * (int64_t)sizeof(U) + 3) / 4;
          CHECK(p.ptr[w] == (uint64_t)id + 1, "image source pointer");
          const std::vector<U>& src = glob[(size_t)id];
          U* img = reinterpret_cast<U*>(drec + loc);
          for (int64_t i = 0; i < cnt; ++i) {
            int64_t o;
            if (w == 0) { const int64_t k = i % p.K, q = i / p.K; o = (int64_t)tab(drec, p.sbA, q / p.M, p.Bt, len, s) + tab(drec, p.smA, q % p.M, p.M, len, s) + tab(drec, p.skA, k, p.K, len, s); }
            else { const int64_t nn = i % p.N, q = i / p.N; o = (int64_t)tab(drec, p.sbB, q / p.K, p.Bt, len, s) + tab(drec, p.snB, nn, p.N, len, s) + tab(drec, p.skB, q % p.K, p.K, len, s); }
            CHECK(o >= 0 && o < (int64_t)src.size(), "image gather outside the input");
            img[i] = src[(size_t)o];
          }
        }
        d_done[sl] = s;
      }
      if (s < 0) continue;
      // ---- step s, from its slot alone
      const int sl = s & (kClRing - 1);
      CHECK(owner[sl] == s && r_done[sl] < s && p_done[sl] < s && d_done[sl] < s, "step started before its record, pointers and images were complete");
      int32_t* rec = slot(s);
      const ClRec c = header(rec);
      const Step& st = P.steps[(size_t)s];
      const int len = cp.steps[(size_t)s].len;
      CHECK(c.Bt == st.Bt && c.M == st.M && c.N == st.N && c.K == st.K && c.numelC == (double)P.tensors[(size_t)st.out].numel, "extents");
      for (const ClTab* t : {&c.obA, &c.omA, &c.okA, &c.obB, &c.onB, &c.okB, &c.obC, &c.omC, &c.onC}) explicit_tabs += t->pos >= 0;
      const int64_t total = (int64_t)c.Bt * c.M * c.N;
      const U gA = scale_of(c.prodA), gB = scale_of(c.prodB);
      CHECK(c.prodA == (st.lhs >= P.n_inputs ? P.tensors[(size_t)st.lhs].producer : -1), "producer of A");
      CHECK(c.prodB == (st.rhs >= P.n_inputs ? P.tensors[(size_t)st.rhs].producer : -1), "producer of B");
      if (c.homeC == CL_HOME_ARENA) {           // the result's region is free of every live tensor (its operands included)
        const int64_t bytes = P.tensors[(size_t)c.idC].numel * (int64_t)sizeof(U);
        CHECK(c.locC >= 0 && c.locC + bytes <= kClArenaBytes, "result outside the arena");
        for (const Live& l : live) CHECK(c.locC + bytes <= l.off || l.off + l.bytes <= c.locC, "two live tensors overlap in the arena");
        live.push_back(Live{c.locC, bytes, c.idC});
      }
      for (int w = 0; w < 2; ++w) {             // an arena operand is where its producer put it
        const int home = w == 0 ? c.homeA : c.homeB, id = w == 0 ? c.idA : c.idB, loc = w == 0 ? c.locA : c.locB;
        if (home != CL_HOME_ARENA) continue;
        bool found = false;
        for (const Live& l : live) if (l.id == id && l.off == loc) found = true;
        CHECK(found, "an arena operand that is not live there");
      }
      bool divA = c.prodA >= 0, divB = c.prodB >= 0;
      if (c.normA || c.normB) {
        CHECK(total > kClSmall, "in-place pass in a step wave 0 computes alone");
        if (c.normA) { CHECK(c.homeA == CL_HOME_ARENA && c.numelA == P.tensors[(size_t)c.idA].numel, "in-place pass on A"); for (int64_t i = 0; i < c.numelA; ++i) { U* x = at(c, rec, 0, i, s); *x = (U)(*x * gA); } divA = false; }
        if (c.normB) { CHECK(c.homeB == CL_HOME_ARENA && c.numelB == P.tensors[(size_t)c.idB].numel, "in-place pass on B"); for (int64_t i = 0; i < c.numelB; ++i) { U* x = at(c, rec, 1, i, s); *x = (U)(*x * gB); } divB = false; }
      }
      for (int64_t o = 0; o < total; ++o) {
        const int64_t nn = o % c.N, q = o / c.N, m = q % c.M, b = q / c.M;
        const int64_t a0 = (int64_t)tab(rec, c.obA, b, c.Bt, len, s) + tab(rec, c.omA, m, c.M, len, s);
        const int64_t b0 = (int64_t)tab(rec, c.obB, b, c.Bt, len, s) + tab(rec, c.onB, nn, c.N, len, s);
        U acc = 0;
        for (int64_t k = 0; k < c.K; ++k) {
          U a = *at(c, rec, 0, a0 + tab(rec, c.okA, k, c.K, len, s), s), bb = *at(c, rec, 1, b0 + tab(rec, c.okB, k, c.K, len, s), s);
          if (divA) a = (U)(a * gA);
          if (divB) bb = (U)(bb * gB);
          acc = (U)(acc + (U)(a * bb));
        }
        *at(c, rec, 2, (int64_t)tab(rec, c.obC, b, c.Bt, len, s) + tab(rec, c.omC, m, c.M, len, s) + tab(rec, c.onC, nn, c.N, len, s), s) = acc;
      }
      // the same step from the plan's own tables
      {
        const int32_t* T = P.tables.data();
        const int64_t* T8 = P.tables64.data();
        const std::vector<U>& A = ref[(size_t)st.lhs];
        const std::vector<U>& B = ref[st.rhs >= 0 ? (size_t)st.rhs : P.tensors.size()];
        std::vector<U>& C = ref[(size_t)st.out];
        for (int64_t b = 0; b < st.Bt; ++b)
          for (int64_t m = 0; m < st.M; ++m)
            for (int64_t nn = 0; nn < st.N; ++nn) {
              U acc = 0;
              for (int64_t k = 0; k < st.K; ++k) {
                const U a = A[(size_t)(T8[st.t.obA + b] + T[st.t.omA + m] + T[st.t.okA + k])];
                const U bb = B[(size_t)(T8[st.t.obB + b] + T[st.t.onB + nn] + T[st.t.okB + k])];
                acc = (U)(acc + (U)((U)(a * gA) * (U)(bb * gB)));
              }
              C[(size_t)(T8[st.t.obC + b] + T[st.t.omC + m] + T[st.t.onC + nn])] = acc;
            }
        CHECK((c.homeC == CL_HOME_ARENA) == (s != n - 1 && cp.home[(size_t)st.out] == CL_HOME_ARENA), "home of the result");
        CHECK(s != n - 1 || c.homeC == CL_HOME_GLOBAL, "the final result does not go to the caller's buffer");
        for (int64_t e = 0; e < P.tensors[(size_t)st.out].numel; ++e)
          CHECK(*at(c, rec, 2, e, s) == C[(size_t)e], "result differs from the plan's own tables at element " + std::to_string(e));
      }
      for (int id : {c.idA, c.idB})              // consumed: dead from here on
        for (size_t i = 0; i < live.size(); ++i)
          if (live[i].id == id) { live.erase(live.begin() + (long)i); break; }
    }
  }
};

}  // namespace

int main() {
  std::string tok;
  int n_plans = 0, n_fail = 0;
  while (std::cin >> tok) {
    if (tok != "plan") { fprintf(stderr, "expected 'plan', got '%s'\n", tok.c_str()); return 2; }
    ctn_plan_desc d{};
    int force = -1;
    std::cin >> d.dtype >> d.n_inputs >> d.n_steps >> force;
    std::vector<int32_t> in_ndim, in_labels, lhs, rhs, ond, olab;
    std::vector<int64_t> in_dims, in_strides;
    bool strided = false;
    for (int i = 0; i < d.n_inputs; ++i) {
      int nd;
      std::cin >> tok >> nd;
      in_ndim.push_back(nd);
      const size_t d0 = in_dims.size();
      for (int a = 0; a < nd; ++a) { int64_t x; std::cin >> x; in_dims.push_back(x); }
      for (int a = 0; a < nd; ++a) { int32_t x; std::cin >> x; in_labels.push_back(x); }
      if (tok == "ins") {
        strided = true;
        for (int a = 0; a < nd; ++a) { int64_t x; std::cin >> x; in_strides.push_back(x); }
      } else {
        std::vector<int64_t> st((size_t)nd, 1);
        for (int a = nd - 2; a >= 0; --a) st[(size_t)a] = st[(size_t)a + 1] * in_dims[d0 + (size_t)a + 1];
        in_strides.insert(in_strides.end(), st.begin(), st.end());
      }
    }
    for (int s = 0; s < d.n_steps; ++s) {
      int l, r, nd;
      std::cin >> tok >> l >> r >> nd;
      lhs.push_back(l); rhs.push_back(r); ond.push_back(nd);
      for (int a = 0; a < nd; ++a) { int32_t x; std::cin >> x; olab.push_back(x); }
    }
    if (!std::cin) { fprintf(stderr, "truncated plan description\n"); return 2; }
    in_dims.push_back(0); in_labels.push_back(0); olab.push_back(0); in_strides.push_back(0);
    d.in_ndim = in_ndim.data(); d.in_dims = in_dims.data(); d.in_labels = in_labels.data();
    d.in_strides = strided ? in_strides.data() : nullptr;
    d.step_lhs = lhs.data(); d.step_rhs = rhs.data(); d.step_out_ndim = ond.data(); d.step_out_labels = olab.data();
    d.stabilize = 1; d.min_norm = 1e-7;
    Plan P;
    std::string err;
    const int rc = build_plan(d, P, err);
    ++n_plans;
    if (rc != CTN_OK) { printf("plan %d rc=%d %s\n", n_plans, rc, err.c_str()); continue; }
    if (!P.chain) { printf("plan %d rc=0 chain=0\n", n_plans); continue; }
    if (force >= 0 && force < P.n_steps) P.steps[(size_t)force].kernel = CTN_KERNEL_FUSED;
    ChainProgram cp;
    std::string why;
    if (!chain_pack(P, &cp, &why)) {
      printf("plan %d rc=0 chain=1 refused: %s\n", n_plans, why.c_str());
      continue;
    }
    int max_len = 0, explicit_tabs = 0;
    for (const ClStepInfo& si : cp.steps) max_len = std::max(max_len, si.len);
    std::string res = "ok";
    try {
      if (P.dtype == CTN_F64) { Replay<uint64_t> rp(P, cp); rp.run(cp.steps[0].len); explicit_tabs = rp.explicit_tabs; }
      else { Replay<uint32_t> rp(P, cp); rp.run(cp.steps[0].len); explicit_tabs = rp.explicit_tabs; }
    } catch (const Fail& f) {
      res = f.why;
      ++n_fail;
    }
    printf("plan %d rc=0 chain=1 steps=%d arena=%d spilled=%d images=%d explicit=%d maxlen=%d words=%zu %s\n", n_plans, P.n_steps,
           cp.n_arena, cp.n_spilled, cp.n_images, explicit_tabs, max_len, cp.words.size(), res.c_str());
  }
  return n_fail ? 1 : 0;
}
