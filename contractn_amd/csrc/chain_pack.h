// chain_pack.h - host-side packer of a chain plan into the "program" k_chain_lds walks (kernels_chain.h).
//
// Pure host code (no HIP), like cplx_match.h: the record layout and the constants below are shared with the kernel,
// the packer itself runs at ctn_exec_create and in the stand-alone driver chain_check.cpp (sanitizer runs on the CPU).
//
// A program is one int32 buffer: one RECORD per step, back to back.  A record is a ClRec header followed by the step's
// explicit gather tables, so one contiguous read of `len` words brings everything the step needs.  Gather offsets are
// not the plan's padded tables: a table that is an arithmetic progression is (base, stride), any other exactly its Bt /
// M / N / K entries (32 bits: every tensor of a chain plan is tiny; a batch offset beyond that refuses the plan).
//
// The walker keeps kClRing slots of kClSlotWords words in LDS.  Record s lives in slot s % kClRing and goes through
// three stages, one per step of the walk, each behind the barrier that ends the step before it (D = kClD = 3):
//   while step s - 3 runs: the record's words are copied from the program        (stage R)
//   while step s - 2 runs: the pointers of its three tensors are looked up        (stage P, into ClRec::ptr)
//   while step s - 1 runs: the images of its staged INPUT operands are gathered   (stage D, behind the tables)
// so a step of the walk costs one round trip to memory, the three stages of three later steps in flight together,
// instead of k_chain's three dependent ones.  An image is the dense [b][m][k] (A) or [b][k][n] (B) copy k_chain stages;
// only network inputs have one (their values do not depend on the walk), and only where record + images fit the slot -
// a larger input is read from global memory in place.  The compute tables of an imaged operand address the image.
//
// Intermediates live in an LDS arena of kClArenaBytes, placed by liveness, first fit, as plan.cpp's arena places them
// in the workspace; one that does not fit keeps its workspace slot (stored, then loaded after the barrier, as k_chain
// does).  Either home is addressed with the element offsets of the tensor's global layout.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "plan.h"

namespace ctn {

constexpr int kClD = 3;                     // record s + kClD is brought in while step s runs
constexpr int kClRing = kClD + 1;           // ring slots: the steps s .. s + kClD
constexpr int kClSlotWords = 3072;          // one slot: 12 KiB (record, then the images of its staged inputs)
constexpr int kClArenaBytes = 72 * 1024;    // intermediates; two 4096-element float64 tensors take 64 KiB
constexpr int kClArenaAlign = 16;
constexpr int kClSmall = 64;                // a step with at most this many outputs is computed by wave 0 alone

// where a tensor of a step lives
enum : int32_t { CL_HOME_GLOBAL = 0, CL_HOME_ARENA = 1, CL_HOME_IMAGE = 2, CL_HOME_ONE = 3 };

struct ClTab { int32_t base, stride, pos; };   // pos < 0: offset(i) = base + i * stride; else the record's word pos + i

struct ClRec {
  int32_t next_off, next_len;        // the record of step s + 1: word offset in the program and length (0, 0 at the end)
  int32_t Bt, M, N, K;
  int32_t idA, idB, idC;             // rows of the pointer table (stage P reads all three)
  int32_t prodA, prodB;              // producing step of each operand, -1 for inputs
  int32_t homeA, homeB, homeC;       // CL_HOME_*
  int32_t locA, locB, locC;          // arena: byte offset; image: word offset in the slot
  int32_t normA, normB;              // an arena operand of a large step with K >= 4 is divided by its scale in place, once
  int32_t numelA, numelB;            // elements of the operand (the in-place pass)
  int32_t imgA, imgB;                // elements of the staged image (0: none)
  int32_t pad0;
  double numelC;
  uint64_t ptr[3];                   // A, B, C: filled by stage P in LDS (zero in the program)
  ClTab obA, omA, okA, obB, onB, okB, obC, omC, onC;   // what the MAC loop addresses
  ClTab sbA, smA, skA, sbB, snB, skB;                  // imaged operands: the gather from the input itself (stage D)
};
constexpr int kClHeaderWords = (int)(sizeof(ClRec) / 4);
static_assert(offsetof(ClRec, next_off) == 0 && offsetof(ClRec, next_len) == 4 && sizeof(ClRec) % 8 == 0 && offsetof(ClRec, numelC) % 8 == 0 && offsetof(ClRec, ptr) % 8 == 0, "ClRec layout");

// what the packer decided, for the engine, the driver and the tests
struct ClStepInfo { int32_t off = 0, len = 0; };
struct ChainProgram {
  std::vector<int32_t> words;
  std::vector<ClStepInfo> steps;
  std::vector<int32_t> home;        // per tensor: CL_HOME_ARENA or CL_HOME_GLOBAL (inputs and the result: global)
  std::vector<int32_t> arena_off;   // per tensor: byte offset in the arena (-1: not there)
  int n_arena = 0, n_spilled = 0, n_images = 0;
};

namespace clpack {

// first fit over [0, kClArenaBytes), lowest address first
struct LdsArena {
  struct Block { int64_t off, size; };
  std::vector<Block> live;   // sorted by offset
  int64_t alloc(int64_t bytes) {
    bytes = (std::max<int64_t>(bytes, 1) + kClArenaAlign - 1) / kClArenaAlign * kClArenaAlign;
    int64_t at = 0;
    size_t i = 0;
    for (; i < live.size(); ++i) {
      if (live[i].off - at >= bytes) break;
      at = live[i].off + live[i].size;
    }
    if (at + bytes > kClArenaBytes) return -1;
    live.insert(live.begin() + (long)i, Block{at, bytes});
    return at;
  }
  void release(int64_t off) {
    for (size_t i = 0; i < live.size(); ++i)
      if (live[i].off == off) { live.erase(live.begin() + (long)i); return; }
  }
};

template <typename I>
inline bool make_tab(const I* t, int64_t n, std::vector<int32_t>& extra, int header_words, ClTab* out) {
  for (int64_t i = 0; i < n; ++i)
    if (t[i] < INT32_MIN || t[i] > INT32_MAX) return false;
  const int64_t stride = n > 1 ? (int64_t)t[1] - (int64_t)t[0] : 0;
  bool prog = stride >= INT32_MIN && stride <= INT32_MAX;
  for (int64_t i = 1; i < n && prog; ++i)
    if ((int64_t)t[i] - (int64_t)t[i - 1] != stride) prog = false;
  if (prog) { *out = ClTab{(int32_t)t[0], (int32_t)stride, -1}; return true; }
  *out = ClTab{0, 0, header_words + (int32_t)extra.size()};
  for (int64_t i = 0; i < n; ++i) extra.push_back((int32_t)t[i]);
  return true;
}

}  // namespace clpack

// Packs plan P (P.chain set) for k_chain_lds.  False, with the reason in *why, when the plan keeps k_chain.
inline bool chain_pack(const Plan& P, ChainProgram* out, std::string* why) {
  using namespace clpack;
  *out = ChainProgram();
  if (!P.chain) { *why = "not a chain plan"; return false; }
  const int64_t es = (int64_t)P.elem_size();
  const int n_tensors = (int)P.tensors.size();
  out->home.assign((size_t)n_tensors, CL_HOME_GLOBAL);
  out->arena_off.assign((size_t)n_tensors, -1);
  out->steps.resize((size_t)P.n_steps);
  LdsArena arena;
  for (int s = 0; s < P.n_steps; ++s) {
    const Step& st = P.steps[s];
    if (st.kernel == CTN_KERNEL_FUSED || st.lhs2 >= 0) { *why = "step " + std::to_string(s) + ": a fused step"; return false; }
    ClRec r;
    memset(&r, 0, sizeof r);
    std::vector<int32_t> extra;
    r.Bt = (int32_t)st.Bt; r.M = (int32_t)st.M; r.N = (int32_t)st.N; r.K = (int32_t)st.K;
    r.idA = st.lhs; r.idB = st.rhs >= 0 ? st.rhs : n_tensors; r.idC = st.out;   // (the ones scalar: the row behind the tensors)
    r.prodA = st.lhs >= P.n_inputs ? P.tensors[st.lhs].producer : -1;
    r.prodB = st.rhs >= P.n_inputs ? P.tensors[st.rhs].producer : -1;
    r.numelC = (double)P.tensors[st.out].numel;
    r.numelA = (int32_t)P.tensors[st.lhs].numel;
    r.numelB = st.rhs >= 0 ? (int32_t)P.tensors[st.rhs].numel : 1;
    const int32_t* T = P.tables.data();
    const int64_t* T8 = P.tables64.data();
    ClTab gbA, gmA, gkA, gbB, gnB, gkB;   // the operands' own offsets
    bool ok = make_tab(T8 + st.t.obA, st.Bt, extra, kClHeaderWords, &gbA) && make_tab(T + st.t.omA, st.M, extra, kClHeaderWords, &gmA) &&
              make_tab(T + st.t.okA, st.K, extra, kClHeaderWords, &gkA) && make_tab(T8 + st.t.obB, st.Bt, extra, kClHeaderWords, &gbB) &&
              make_tab(T + st.t.onB, st.N, extra, kClHeaderWords, &gnB) && make_tab(T + st.t.okB, st.K, extra, kClHeaderWords, &gkB) &&
              make_tab(T8 + st.t.obC, st.Bt, extra, kClHeaderWords, &r.obC) && make_tab(T + st.t.omC, st.M, extra, kClHeaderWords, &r.omC) &&
              make_tab(T + st.t.onC, st.N, extra, kClHeaderWords, &r.onC);
    if (!ok) { *why = "step " + std::to_string(s) + ": a batch offset beyond 32 bits"; return false; }
    int64_t len = kClHeaderWords + (int64_t)extra.size();
    len = (len + 3) / 4 * 4;                       // images start 16-byte aligned
    if (len > kClSlotWords) {
      *why = "step " + std::to_string(s) + ": a record of " + std::to_string(len) + " words exceeds a ring slot of " + std::to_string(kClSlotWords);
      return false;
    }
    // operands: an intermediate where its producer left it, an input as an image where the slot has room
    int64_t used = len;
    auto place = [&](int id, bool isA) {
      int32_t &home = isA ? r.homeA : r.homeB, &loc = isA ? r.locA : r.locB, &img = isA ? r.imgA : r.imgB;
      if (id < 0) { home = CL_HOME_ONE; return; }
      if (id >= P.n_inputs) {
        home = out->home[(size_t)id];
        loc = home == CL_HOME_ARENA ? out->arena_off[(size_t)id] : 0;
        return;
      }
      const int64_t n = st.Bt * (isA ? st.M : st.N) * st.K;
      const int64_t words = (n * es + 15) / 16 * 4;
      if (used + words > kClSlotWords) { home = CL_HOME_GLOBAL; return; }
      home = CL_HOME_IMAGE; loc = (int32_t)used; img = (int32_t)n;
      used += words;
      ++out->n_images;
    };
    place(st.lhs, true);
    place(st.rhs, false);
    r.obA = gbA; r.omA = gmA; r.okA = gkA; r.obB = gbB; r.onB = gnB; r.okB = gkB;
    if (r.homeA == CL_HOME_IMAGE) {   // [b][m][k]
      r.sbA = gbA; r.smA = gmA; r.skA = gkA;
      r.obA = ClTab{0, (int32_t)(st.M * st.K), -1}; r.omA = ClTab{0, (int32_t)st.K, -1}; r.okA = ClTab{0, 1, -1};
    }
    if (r.homeB == CL_HOME_IMAGE) {   // [b][k][n]
      r.sbB = gbB; r.snB = gnB; r.skB = gkB;
      r.obB = ClTab{0, (int32_t)(st.K * st.N), -1}; r.onB = ClTab{0, 1, -1}; r.okB = ClTab{0, (int32_t)st.N, -1};
    }
    if (r.homeB == CL_HOME_ONE) { r.obB = r.onB = r.okB = ClTab{0, 0, -1}; }
    const bool large = st.Bt * st.M * st.N > kClSmall;
    const bool same = st.lhs == st.rhs;
    r.normA = large && st.K >= 4 && !same && r.homeA == CL_HOME_ARENA && r.prodA >= 0;
    r.normB = large && st.K >= 4 && !same && r.homeB == CL_HOME_ARENA && r.prodB >= 0;
    // the result: allocated before the operands are released, as in the workspace
    if (s != P.n_steps - 1) {
      const int64_t at = arena.alloc(P.tensors[st.out].numel * es);
      if (at >= 0) {
        out->home[(size_t)st.out] = CL_HOME_ARENA; out->arena_off[(size_t)st.out] = (int32_t)at;
        r.homeC = CL_HOME_ARENA; r.locC = (int32_t)at;
        ++out->n_arena;
      } else {
        ++out->n_spilled;
      }
    }
    for (int id : {st.lhs, st.rhs})
      if (id >= P.n_inputs && out->home[(size_t)id] == CL_HOME_ARENA) arena.release(out->arena_off[(size_t)id]);
    // emit
    out->steps[(size_t)s].off = (int32_t)out->words.size();
    out->steps[(size_t)s].len = (int32_t)len;
    out->words.resize(out->words.size() + (size_t)len, 0);
    int32_t* dst = out->words.data() + out->steps[(size_t)s].off;
    memcpy(dst, &r, sizeof r);
    if (!extra.empty()) memcpy(dst + kClHeaderWords, extra.data(), extra.size() * 4);
  }
  for (int s = 0; s + 1 < P.n_steps; ++s) {   // each record names the next one
    int32_t* r = out->words.data() + out->steps[(size_t)s].off;   // ClRec::next_off, next_len: the first two words
    r[0] = out->steps[(size_t)s + 1].off;
    r[1] = out->steps[(size_t)s + 1].len;
  }
  return true;
}

}  // namespace ctn
