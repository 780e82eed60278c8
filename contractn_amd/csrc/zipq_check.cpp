// zipq_check.cpp - host-only driver of the work-item arithmetic of k_zipqp_f32 (zipq_items.h), for sanitizer runs on the CPU.
//
//   make -C contractn_amd/csrc zipq_check   ->  ../lib/zipq_check_asan   (-fsanitize=address,undefined)
//   zipq_check_asan < commands.txt
//
// Input, one command per line; one line of output per command:
//
//   walk <items> <grid>          every block id 0 .. grid - 1 walks its items exactly as the kernel does (pid = zipq_pid, then
//                                item = zipq_item(pid, k, grid) while it is < items).  Checked: the remap is a permutation of
//                                0 .. grid - 1; every item is walked exactly once; a workgroup's rounds number ceil or floor of
//                                items / grid and equal zipq_rounds; for an even grid items 2 r and 2 r + 1 fall in the same
//                                round.  `items=.. grid=.. perm=<ok|why> once=.. rounds=.. pair=.. <ok|FAIL>`
//   dump <items> <grid>          `bid:pid:item,item,...` for every block id, separated by blanks (the test checks a few itself)
//   grid <items> <n_cu> <cap>    `cap=<zipq_cap> grid=<zipq_grid>`
//   rt <item> <per>              `r=.. t=..`
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "zipq_items.h"

using namespace ctn;

namespace {

std::string walk(int64_t items, int grid) {
  std::string perm = "ok", once = "ok", rounds = "ok", pair = "ok";
  std::vector<int> seen_pid((size_t)grid, 0), walked((size_t)items, 0), round_of((size_t)items, -1);
  const int lo = (int)(items / grid), hi = (int)((items + grid - 1) / grid);
  for (int bid = 0; bid < grid; ++bid) {
    const int pid = zipq_pid(bid, grid);
    if (pid < 0 || pid >= grid) { perm = "pid_out_of_range"; continue; }
    if (seen_pid[(size_t)pid]++) perm = "pid_twice";
    int k = 0;
    for (;; ++k) {
      const int64_t item = zipq_item(pid, k, grid);
      if (item >= items) break;
      if (item < 0) { once = "negative_item"; break; }
      if (walked[(size_t)item]++) once = "item_twice";
      round_of[(size_t)item] = k;
    }
    if (k != lo && k != hi) rounds = "neither_floor_nor_ceil";
    if (k != zipq_rounds(pid, items, grid)) rounds = "zipq_rounds_differs";
  }
  for (int64_t i = 0; i < items; ++i)
    if (walked[(size_t)i] != 1) once = walked[(size_t)i] ? "item_twice" : "item_never";
  if (grid % 2 == 0)
    for (int64_t i = 0; i + 1 < items; i += 2)
      if (round_of[(size_t)i] != round_of[(size_t)i + 1]) pair = "rounds_differ";
  const bool ok = perm == "ok" && once == "ok" && rounds == "ok" && pair == "ok";
  std::ostringstream o;
  o << "items=" << items << " grid=" << grid << " perm=" << perm << " once=" << once << " rounds=" << rounds << " pair=" << pair
    << (ok ? " ok" : " FAIL");
  return o.str();
}

}  // namespace

int main() {
  std::string line;
  bool all_ok = true;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    if (!(in >> cmd)) continue;
    if (cmd == "walk" || cmd == "dump") {
      int64_t items = 0;
      int grid = 0;
      in >> items >> grid;
      if (items < 1 || grid < 1 || grid > items || items > (1 << 24)) { std::cout << "bad arguments FAIL\n"; all_ok = false; continue; }
      if (cmd == "walk") {
        const std::string res = walk(items, grid);
        all_ok = all_ok && res.size() > 3 && res.compare(res.size() - 3, 3, " ok") == 0;
        std::cout << res << "\n";
      } else {
        for (int bid = 0; bid < grid; ++bid) {
          const int pid = zipq_pid(bid, grid);
          std::cout << (bid ? " " : "") << bid << ":" << pid << ":";
          for (int k = 0; zipq_item(pid, k, grid) < items; ++k) std::cout << (k ? "," : "") << zipq_item(pid, k, grid);
        }
        std::cout << "\n";
      }
    } else if (cmd == "grid") {
      int64_t items = 0;
      int n_cu = 0, cap = 0;
      in >> items >> n_cu >> cap;
      std::cout << "cap=" << zipq_cap(cap, n_cu) << " grid=" << zipq_grid(items, n_cu, cap) << "\n";
    } else if (cmd == "rt") {
      int64_t item = 0;
      int per = 0, r = -1, t = -1;
      in >> item >> per;
      if (per < 1) { std::cout << "bad arguments FAIL\n"; all_ok = false; continue; }
      zipq_item_rt(item, per, &r, &t);
      std::cout << "r=" << r << " t=" << t << "\n";
    } else {
      std::cout << "unknown command FAIL\n";
      all_ok = false;
    }
  }
  return all_ok ? 0 : 1;
}
