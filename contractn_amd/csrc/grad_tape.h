// grad_tape.h - host side of the backward tape (include/ctn_abi.h, ctn_grad_tape_*): what a record reads and writes, the
// arena layout by liveness, and the checks a tape must pass before anything is launched.  Host code, no HIP calls:
// engine.hip builds its tapes with it and tape_check.cpp replays its layouts on the CPU under the sanitizers.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "ctn_abi.h"

namespace ctn {

constexpr int64_t kTapeAlign = 16;
constexpr int64_t kTapeDefaultMaxBytes = (int64_t)1 << 30;

inline int64_t tape_round_up(int64_t v) { return (v + kTapeAlign - 1) / kTapeAlign * kTapeAlign; }

// Bit 0 of ctn_tape_record.reserved: this RUN record closes - its finish and its register work are one launch.
constexpr int32_t kTapeClose = 1;
inline bool tape_closes(const ctn_tape_record& r) { return (r.reserved & kTapeClose) != 0; }

// The slots a record reads and the slots it writes (the seed's scratch is written and read inside the record).
struct TapeAccess { int reads[3]; int n_reads = 0; int writes[2]; int n_writes = 0; };
inline TapeAccess tape_access(const ctn_tape_record& r) {
  TapeAccess a;
  for (int j = 0; j < 3; ++j)
    if (r.in[j] >= 0) a.reads[a.n_reads++] = r.in[j];
  a.writes[a.n_writes++] = r.out;
  if (r.kind == CTN_TAPE_SEED) a.writes[a.n_writes++] = r.aux;
  return a;
}

// How many of reg[0..4) a record of this kind uses, and which of them may be -1.
inline bool tape_regs_ok(const ctn_tape_record& r, int n_regs) {
  auto in = [&](int v) { return v >= 0 && v < n_regs; };
  auto opt = [&](int v) { return v == -1 || in(v); };
  switch (r.kind) {
    case CTN_TAPE_RUN: return in(r.reg[0]) && in(r.reg[1]) && opt(r.reg[2]) && opt(r.reg[3]);
    case CTN_TAPE_SEED: return in(r.reg[0]) && opt(r.reg[1]) && in(r.reg[2]) && r.reg[3] == -1;
    case CTN_TAPE_LEAF: return opt(r.reg[0]) && r.reg[1] == -1 && r.reg[2] == -1 && r.reg[3] == -1;
  }
  return false;
}

struct TapeLife { int first = -1, last = -1; };   // record of the first write and of the last access

// Structure of the sequence alone (no layout yet): indices in range, every arena slot written before it is read, no
// record that writes what it reads.  Fills the lifetimes of the slots.  Returns "" or what is wrong.
inline std::string tape_check_records(const ctn_tape_desc& d, std::vector<TapeLife>* life) {
  if (d.n_records < 1 || d.n_slots < 1 || d.n_ext < 0 || d.n_regs < 1 || d.n_plans < 0 || d.n_axes < 0 || !d.records || !d.slots)
    return "empty or NULL tape description";
  life->assign(d.n_slots, TapeLife{});
  for (int s = 0; s < d.n_slots; ++s) {
    const ctn_tape_slot& sl = d.slots[s];
    if (sl.external) {
      if (sl.ext_index < 0 || sl.ext_index >= d.n_ext) return "slot " + std::to_string(s) + ": external index out of range";
    } else if (sl.bytes <= 0 || sl.bytes % 4) {
      return "slot " + std::to_string(s) + ": arena size must be a positive multiple of 4 bytes";
    }
  }
  for (int i = 0; i < d.n_records; ++i) {
    const ctn_tape_record& r = d.records[i];
    const std::string at = "record " + std::to_string(i) + ": ";
    if (r.kind != CTN_TAPE_RUN && r.kind != CTN_TAPE_SEED && r.kind != CTN_TAPE_LEAF) return at + "unknown kind";
    if (!tape_regs_ok(r, d.n_regs)) return at + "a register index leaves the block";
    if (r.reserved & ~kTapeClose) return at + "unknown bits in reserved";
    if (tape_closes(r) && r.kind != CTN_TAPE_RUN) return at + "only a RUN record closes";
    auto slot_ok = [&](int v) { return v >= 0 && v < d.n_slots; };
    if (!slot_ok(r.in[0]) || !slot_ok(r.out)) return at + "slot index out of range";
    for (int j = 1; j < 3; ++j)
      if (r.in[j] != -1 && !slot_ok(r.in[j])) return at + "slot index out of range";
    if (r.kind == CTN_TAPE_RUN) {
      if (r.plan < 0 || r.plan >= d.n_plans || r.in[2] != -1 || r.aux != -1) return at + "bad RUN record";
      if (d.slots[r.out].external) return at + "a RUN record writes into the arena only";
    } else if (r.kind == CTN_TAPE_SEED) {
      if (!slot_ok(r.aux) || d.slots[r.aux].external || d.slots[r.aux].bytes < (int64_t)CTN_GRAD_SCRATCH * 8 || r.numel < 1)
        return at + "bad SEED record";
    } else {
      if (r.in[1] != -1 || r.in[2] != -1 || r.aux != -1 || r.ndim < 0 || r.ndim > CTN_GRAD_MAX_DIMS || r.axes < 0 ||
          r.axes + r.ndim > d.n_axes || (r.ndim > 0 && (!d.leaf_dims || !d.leaf_strides || !d.leaf_first)))
        return at + "bad LEAF record";
    }
    if ((r.src_dtype != CTN_F32 && r.src_dtype != CTN_F64) || (r.kind != CTN_TAPE_RUN && r.dst_dtype != CTN_F32 && r.dst_dtype != CTN_F64))
      return at + "dtypes must be f32 or f64";
    const TapeAccess a = tape_access(r);
    for (int j = 0; j < a.n_reads; ++j) {
      const int s = a.reads[j];
      for (int w = 0; w < a.n_writes; ++w)
        if (a.writes[w] == s) return at + "writes a slot it reads";
      if (d.slots[s].external) continue;
      if ((*life)[s].first < 0) return at + "slot " + std::to_string(s) + " is read before it is written";
      (*life)[s].last = i;
    }
    if (a.n_writes == 2 && a.writes[0] == a.writes[1]) return at + "output and scratch are one slot";
    for (int w = 0; w < a.n_writes; ++w) {
      const int s = a.writes[w];
      if ((*life)[s].first < 0) (*life)[s].first = i;
      (*life)[s].last = i;
    }
  }
  return "";
}

// Arena layout: the register block first, then every arena slot at the lowest 16-byte aligned offset at which it shares
// no byte with a slot whose lifetime [first write, last access] meets its own (first fit, slots in order of their first
// write).  A record's inputs and outputs are alive together in that record, so they never share bytes either.
// off[s] = -1 for external slots and for arena slots no record touches.  Returns the arena's size.
inline int64_t tape_layout(const ctn_tape_desc& d, const std::vector<TapeLife>& life, std::vector<int64_t>* off) {
  const int64_t regs_bytes = tape_round_up((int64_t)d.n_regs * 8);
  off->assign(d.n_slots, -1);
  std::vector<int> order;
  for (int s = 0; s < d.n_slots; ++s)
    if (!d.slots[s].external && life[s].first >= 0) order.push_back(s);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return life[a].first < life[b].first; });
  int64_t top = regs_bytes;
  std::vector<int> alive;                                    // placed slots whose lifetime has not ended yet
  std::vector<std::pair<int64_t, int64_t>> busy;
  for (int s : order) {
    alive.erase(std::remove_if(alive.begin(), alive.end(), [&](int t) { return life[t].last < life[s].first; }), alive.end());
    busy.clear();
    for (int t : alive) busy.push_back({(*off)[t], (*off)[t] + tape_round_up(d.slots[t].bytes)});
    std::sort(busy.begin(), busy.end());
    const int64_t need = tape_round_up(d.slots[s].bytes);
    int64_t at = regs_bytes;
    for (const auto& b : busy) {
      if (b.first - at >= need) break;
      at = std::max(at, b.second);
    }
    (*off)[s] = at;
    top = std::max(top, at + need);
    alive.push_back(s);
  }
  return top;
}

// A layout (off[], arena_bytes) against the sequence: alignment, bounds, the register block left alone, and no two slots
// that are alive together sharing a byte.  Returns "" or what is wrong.
inline std::string tape_check_layout(const ctn_tape_desc& d, const std::vector<TapeLife>& life, const std::vector<int64_t>& off,
                                     int64_t arena_bytes) {
  const int64_t regs_bytes = tape_round_up((int64_t)d.n_regs * 8);
  std::vector<int> used;
  for (int s = 0; s < d.n_slots; ++s) {
    if (d.slots[s].external || life[s].first < 0) continue;
    const std::string at = "slot " + std::to_string(s) + ": ";
    if (off[s] % kTapeAlign) return at + "offset is not 16-byte aligned";
    if (off[s] < regs_bytes) return at + "overlaps the register block";
    if (off[s] + d.slots[s].bytes > arena_bytes) return at + "leaves the arena";
    used.push_back(s);
  }
  // sweep in order of first write; compare with the slots still alive
  std::stable_sort(used.begin(), used.end(), [&](int a, int b) { return life[a].first < life[b].first; });
  std::vector<int> alive;
  for (int s : used) {
    alive.erase(std::remove_if(alive.begin(), alive.end(), [&](int t) { return life[t].last < life[s].first; }), alive.end());
    for (int t : alive)
      if (off[s] < off[t] + d.slots[t].bytes && off[t] < off[s] + d.slots[s].bytes)
        return "slots " + std::to_string(t) + " and " + std::to_string(s) + " are alive together and overlap";
    alive.push_back(s);
  }
  return "";
}

}  // namespace ctn
