// tape_check.cpp - host-only driver of the backward tape's layout (grad_tape.h), for sanitizer runs on the CPU.
//
//   make -C contractn_amd/csrc tape_check   ->  ../lib/tape_check_asan   (-fsanitize=address,undefined)
//   tape_check_asan < tapes.txt
//
// Input, one description per tape:
//
//   tape <n_records> <n_slots> <n_ext> <n_regs> <given: 0 = lay the arena out with tape_layout | 1 = offsets are given |
//                                                 2 = as 0, static checks only: a layout too large to replay word by word>
//   slot <external 0|1> <ext_index> <bytes> <offset>            (n_slots lines; offset is read only when given = 1)
//   rec <kind> <plan> <in0> <in1> <in2> <out> <aux> <reg0> <reg1> <reg2> <reg3> [<reserved>]   (n_records lines; reserved:
//                                                 bit 0 = a RUN record that closes, CTN_GRAD_CLOSE=1; left out = 0)
//   arena <bytes>                                               (only when given = 1)
//
// Two things are checked for every tape, and both must pass:
//   static  tape_check_records + tape_check_layout - what ctn_grad_tape_create runs before it allocates anything;
//   replay  the sequence is run twice (a tape is replayed: the second run meets the first one's leftovers, with fresh
//           external inputs) on ONE byte array laid out as the arena - registers at its head as the kernels address
//           them - and on separately allocated buffers, with small-integer stand-ins for the three record kinds
//           (wrapping 32-bit words; an output word reads operand words at other positions than its own, as a contraction does,
//           and every register the real record reads), and
//           every record's output is compared EXACTLY.  The arena replay also keeps, per word, which slot wrote it last:
//           a slot that is read before it is written in this run, or after another slot reused its bytes, fails there.
// One line per tape: `records=.. slots=.. arena=.. static=<ok|why> replay=<ok|why|skipped|static_only> <ok|FAIL>`.
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "grad_tape.h"

using namespace ctn;

namespace {

struct Fail { std::string why; };

struct Tape {
  ctn_tape_desc d{};
  std::vector<ctn_tape_record> recs;
  std::vector<ctn_tape_slot> slots;
  std::vector<int64_t> off;
  int64_t arena_bytes = 0;
};

uint32_t next_rand(uint32_t* s) { *s ^= *s << 13; *s ^= *s >> 17; *s ^= *s << 5; return *s; }

// Memory as the replay sees it.  `arena` = true: arena slots live in one array at their offsets, registers at its head.
struct Mem {
  const Tape& t;
  bool in_arena;
  std::vector<uint32_t> arena;            // words
  std::vector<int> owner;                 // per arena word: the slot that wrote it in this run, -1 none, -2 a register
  std::vector<std::vector<uint32_t>> buf; // separate buffers: per slot (reference), per external index (both)
  std::vector<std::vector<uint32_t>> ext;
  std::vector<uint64_t> regs;             // reference registers

  Mem(const Tape& tape, bool a) : t(tape), in_arena(a) {
    ext.resize(t.d.n_ext);
    for (const auto& s : t.slots)
      if (s.external) ext[s.ext_index].resize(std::max(ext[s.ext_index].size(), (size_t)std::max<int64_t>(s.bytes / 4, 1)));
    if (in_arena) {
      arena.assign((size_t)(t.arena_bytes / 4), 0xA5A5A5A5u);
      owner.assign(arena.size(), -1);
    } else {
      buf.resize(t.slots.size());
      for (size_t s = 0; s < t.slots.size(); ++s)
        if (!t.slots[s].external) buf[s].assign((size_t)(t.slots[s].bytes / 4), 0x5A5A5A5Au);
      regs.assign(t.d.n_regs, 0);
    }
  }
  void begin_run(uint32_t seed) {
    for (auto& e : ext)
      for (auto& w : e) w = next_rand(&seed) & 0xFFFF;
    if (in_arena) {
      std::fill(owner.begin(), owner.end(), -1);
      const size_t rw = (size_t)tape_round_up((int64_t)t.d.n_regs * 8) / 4;     // the memset at the head of the sequence
      if (rw > arena.size()) throw Fail{"the register block leaves the arena"};
      for (size_t i = 0; i < rw; ++i) { arena[i] = 0; owner[i] = -2; }
    } else {
      std::fill(regs.begin(), regs.end(), 0);
    }
  }
  void slot_ok(int s) const { if (s < 0 || s >= (int)t.slots.size()) throw Fail{"slot index " + std::to_string(s) + " out of range"}; }
  size_t words(int s) const {
    slot_ok(s);
    return t.slots[s].external ? ext[t.slots[s].ext_index].size() : (size_t)(t.slots[s].bytes / 4);
  }
  size_t word_at(int s, size_t i) const {
    const int64_t o = t.off[s];
    if (o < 0 || o % 4) throw Fail{"slot " + std::to_string(s) + " has no word-aligned offset"};
    const size_t w = (size_t)(o / 4) + i;
    if (i >= words(s) || w >= arena.size()) throw Fail{"slot " + std::to_string(s) + " leaves the arena"};
    return w;
  }
  uint32_t load(int s, size_t i) const {
    slot_ok(s);
    if (t.slots[s].external) return ext[t.slots[s].ext_index].at(i);
    if (!in_arena) return buf[s].at(i);
    const size_t w = word_at(s, i);
    if (owner[w] != s)
      throw Fail{"slot " + std::to_string(s) + " is read " + (owner[w] == -1 ? "before it is written" : "after its bytes were reused")};
    return arena[w];
  }
  void store(int s, size_t i, uint32_t v) {
    slot_ok(s);
    if (t.slots[s].external) { ext[t.slots[s].ext_index].at(i) = v; return; }
    if (!in_arena) { buf[s].at(i) = v; return; }
    const size_t w = word_at(s, i);
    arena[w] = v; owner[w] = s;
  }
  void reg_ok(int r) const { if (r < 0 || r >= t.d.n_regs) throw Fail{"register " + std::to_string(r) + " leaves the block"}; }
  uint64_t rload(int r) const {
    reg_ok(r);
    if (!in_arena) return regs[r];
    const size_t w = 2 * (size_t)r;
    if (w + 1 >= arena.size() || owner[w] != -2 || owner[w + 1] != -2) throw Fail{"register " + std::to_string(r) + " was overwritten by a slot"};
    return (uint64_t)arena[w] | ((uint64_t)arena[w + 1] << 32);
  }
  void rstore(int r, uint64_t v) {
    reg_ok(r);
    if (!in_arena) { regs[r] = v; return; }
    const size_t w = 2 * (size_t)r;
    if (w + 1 >= arena.size()) throw Fail{"register " + std::to_string(r) + " leaves the arena"};
    arena[w] = (uint32_t)v; arena[w + 1] = (uint32_t)(v >> 32);
    owner[w] = owner[w + 1] = -2;
  }
};

uint64_t slot_sum(const Mem& m, int s) {
  uint64_t v = 0;
  for (size_t i = 0; i < m.words(s); ++i) v += m.load(s, i);
  return v;
}

void eval(const ctn_tape_record& r, Mem& m) {
  const size_t wo = m.words(r.out);
  const size_t w0 = m.words(r.in[0]);
  if (w0 == 0 || (r.in[1] >= 0 && m.words(r.in[1]) == 0) || (r.kind == CTN_TAPE_SEED && m.words(r.aux) == 0)) throw Fail{"an empty slot"};
  if (r.kind == CTN_TAPE_RUN) {
    const size_t w1 = r.in[1] >= 0 ? m.words(r.in[1]) : 1;
    for (size_t i = 0; i < wo; ++i)
      m.store(r.out, i, 2654435761u * (uint32_t)(r.plan + 1) + m.load(r.in[0], (i * 5 + 1) % w0) * 3u +
                            (r.in[1] >= 0 ? m.load(r.in[1], w1 - 1 - i % w1) * 5u : 7u) + (uint32_t)i);
    uint64_t v = slot_sum(m, r.out);
    m.rstore(r.reg[0], v);
    if (r.reg[2] >= 0) v += m.rload(r.reg[2]);
    if (r.reg[3] >= 0) v += m.rload(r.reg[3]);
    m.rstore(r.reg[1], v);
  } else if (r.kind == CTN_TAPE_SEED) {
    const size_t w1 = r.in[1] >= 0 ? m.words(r.in[1]) : 1;
    const size_t ws = std::min<size_t>(m.words(r.aux), 8);
    for (size_t i = 0; i < ws; ++i) m.store(r.aux, i, m.load(r.in[0], i % w0) ^ 0x9E37u);
    const uint32_t z = (uint32_t)m.rload(r.reg[0]), g = r.reg[1] >= 0 ? (uint32_t)m.rload(r.reg[1]) : 0u;
    for (size_t i = 0; i < wo; ++i)
      m.store(r.out, i, m.load(r.in[0], w0 - 1 - i % w0) * 3u + (r.in[1] >= 0 ? m.load(r.in[1], (i * 5 + 1) % w1) * 5u : 0u) +
                            (r.in[2] >= 0 ? m.load(r.in[2], 0) * 7u : 0u) + m.load(r.aux, i % ws) + z * 11u + g * 13u);
    m.rstore(r.reg[2], m.rload(r.reg[0]) * 17u + (r.reg[1] >= 0 ? m.rload(r.reg[1]) : 0) + slot_sum(m, r.out));
  } else {
    const uint32_t g = r.reg[0] >= 0 ? (uint32_t)m.rload(r.reg[0]) * 23u : 1u;
    for (size_t i = 0; i < wo; ++i) m.store(r.out, i, m.load(r.in[0], w0 - 1 - i % w0) * 19u + g);
  }
}

std::string replay(const Tape& t) {
  try {
    Mem a(t, true), b(t, false);
    for (int run = 0; run < 2; ++run) {
      a.begin_run(88172645u + run); b.begin_run(88172645u + run);
      for (size_t i = 0; i < t.recs.size(); ++i) {
        const ctn_tape_record& r = t.recs[i];
        if (r.kind != CTN_TAPE_RUN && r.kind != CTN_TAPE_SEED && r.kind != CTN_TAPE_LEAF) throw Fail{"unknown kind"};
        if (r.kind == CTN_TAPE_SEED) a.slot_ok(r.aux);
        // a closing RUN record leaves what a plain one and its k_tape_regs leave: eval() is the same for both
        if (tape_closes(r) && r.kind != CTN_TAPE_RUN) throw Fail{"record " + std::to_string(i) + ": only a RUN record closes"};
        try {
          eval(r, b);
          eval(r, a);
          for (size_t w = 0; w < a.words(r.out); ++w)
            if (a.load(r.out, w) != b.load(r.out, w)) throw Fail{"output differs from the separately allocated run"};
          for (int j = 0; j < 4; ++j)
            if (r.reg[j] >= 0 && a.rload(r.reg[j]) != b.rload(r.reg[j])) throw Fail{"a register differs from the separately allocated run"};
        } catch (Fail& f) {
          throw Fail{"run " + std::to_string(run) + " record " + std::to_string(i) + ": " + f.why};
        }
      }
    }
  } catch (Fail& f) {
    return f.why;
  }
  return "ok";
}

std::string squash(std::string s) {
  for (auto& c : s)
    if (c == ' ') c = '_';
  return s;
}

}  // namespace

int main() {
  std::string word;
  int bad = 0;
  while (std::cin >> word) {
    if (word != "tape") { printf("parse error: expected 'tape', got '%s'\n", word.c_str()); return 2; }
    Tape t;
    int given = 0;
    int nr = 0, ns = 0;
    std::cin >> nr >> ns >> t.d.n_ext >> t.d.n_regs >> given;
    if (!std::cin || nr < 0 || ns < 0 || nr > (1 << 22) || ns > (1 << 22)) { printf("parse error in the tape header\n"); return 2; }
    const bool static_only = given == 2;
    if (static_only) given = 0;
    t.slots.resize(ns); t.recs.resize(nr); t.off.assign(ns, -1);
    for (int s = 0; s < ns; ++s) {
      int64_t o = -1;
      std::cin >> word >> t.slots[s].external >> t.slots[s].ext_index >> t.slots[s].bytes >> o;
      if (!std::cin || word != "slot") { printf("parse error at slot %d\n", s); return 2; }
      if (given && !t.slots[s].external) t.off[s] = o;
    }
    int max_plan = -1;
    for (int i = 0; i < nr; ++i) {
      ctn_tape_record& r = t.recs[i];
      r = ctn_tape_record{};
      std::cin >> word >> r.kind >> r.plan >> r.in[0] >> r.in[1] >> r.in[2] >> r.out >> r.aux >> r.reg[0] >> r.reg[1] >> r.reg[2] >> r.reg[3];
      if (!std::cin || word != "rec") { printf("parse error at record %d\n", i); return 2; }
      while (std::cin.peek() == ' ' || std::cin.peek() == '\t') std::cin.get();
      if (std::cin.peek() >= '0' && std::cin.peek() <= '9') {          // the optional twelfth field
        std::cin >> r.reserved;
        if (!std::cin) { printf("parse error at record %d\n", i); return 2; }
      }
      r.numel = 1;
      max_plan = std::max(max_plan, r.plan);
    }
    if (given) {
      std::cin >> word >> t.arena_bytes;
      if (!std::cin || word != "arena" || t.arena_bytes < 0 || t.arena_bytes > ((int64_t)1 << 32)) { printf("parse error at arena\n"); return 2; }
    }
    t.d.n_records = nr; t.d.n_slots = ns; t.d.n_plans = max_plan + 1; t.d.n_axes = 0;
    t.d.records = t.recs.data(); t.d.slots = t.slots.data();
    std::vector<TapeLife> life;
    std::string st = tape_check_records(t.d, &life);
    bool can_replay = true;
    if (st.empty()) {
      if (!given) t.arena_bytes = tape_layout(t.d, life, &t.off);
      st = tape_check_layout(t.d, life, t.off, t.arena_bytes);
    } else if (!given) {
      can_replay = false;                       // no layout to replay: the sequence itself was refused
    }
    for (const auto& s : t.slots)
      if (s.external && (s.ext_index < 0 || s.ext_index >= t.d.n_ext || s.bytes < 0 || s.bytes > ((int64_t)1 << 30))) can_replay = false;
    if (t.arena_bytes % 4 || t.arena_bytes > ((int64_t)1 << 32)) can_replay = false;
    if (st.empty()) st = "ok";
    const std::string rp = static_only ? "static_only" : can_replay ? replay(t) : "skipped";
    const bool ok = st == "ok" && (rp == "ok" || static_only);
    bad += ok ? 0 : 1;
    printf("records=%d slots=%d arena=%lld static=%s replay=%s %s\n", nr, ns, (long long)t.arena_bytes, squash(st).c_str(),
           squash(rp).c_str(), ok ? "ok" : "FAIL");
  }
  return bad ? 1 : 0;
}
