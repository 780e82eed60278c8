// zipq_items.h - how the work items of one k_zipqp_f32 launch (kernels_zipqp.h) are spread over its workgroups.
// Plain inline functions that compile for host and device alike: the engine sizes the grid with them, the kernel walks its
// items with them, and zipq_check.cpp replays them on the CPU under the sanitizers (make zipq_check).
//
// An item is one (replica, block of 128 values of u) of a site pair - what one workgroup of k_zipq_f32 computes.  The grid
// is min(items, CUs), or a cap set for tests; workgroup `pid` walks items pid, pid + grid, pid + 2 grid, ...: round k of
// all workgroups is items [k grid, (k + 1) grid), so the items of a replica run in the same round on neighbouring pids.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CTN_ZQI_FN __host__ __device__ inline
#else
#define CTN_ZQI_FN inline
#endif

namespace ctn {

// items of a launch: R replicas x U / zu blocks of u
CTN_ZQI_FN int64_t zipq_items(int R, int U, int zu) { return (int64_t)R * (U / zu); }

// the grid cap as the engine applies it: unset (<= 0) means n_cu, anything else is clamped to [1, n_cu]
CTN_ZQI_FN int zipq_cap(int cap, int n_cu) {
  const int top = n_cu < 1 ? 1 : n_cu;
  return cap <= 0 ? top : cap > top ? top : cap;
}

// workgroups of a launch
CTN_ZQI_FN int zipq_grid(int64_t items, int n_cu, int cap) {
  const int c = zipq_cap(cap, n_cu);
  return items < (int64_t)c ? (items < 1 ? 1 : (int)items) : c;
}

// The XCD remap of every kernel that remaps its block id (the zipper kernels, the k_mfma_* tiles, k_cmfma_f32):
// consecutive block ids go round the 8 XCDs, so block `bid` becomes the workgroup `pid` for which consecutive pids share
// an XCD (and its L2).  A permutation of 0 .. nwg - 1.
CTN_ZQI_FN int zipq_pid(int bid, int nwg) {
  const int xcd = bid & 7, slot = bid >> 3, q8 = nwg >> 3, r8 = nwg & 7;
  return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + slot;
}

// item of round k for workgroup pid (walked while it is < items), and how many rounds that workgroup has
CTN_ZQI_FN int64_t zipq_item(int pid, int k, int grid) { return (int64_t)pid + (int64_t)k * grid; }
CTN_ZQI_FN int zipq_rounds(int pid, int64_t items, int grid) {
  return (int64_t)pid >= items ? 0 : (int)((items - 1 - pid) / grid) + 1;
}

// (replica, block of u) of an item: `per` = U / zu blocks per replica
CTN_ZQI_FN void zipq_item_rt(int64_t item, int per, int* r, int* t) {
  *r = (int)(item / per);
  *t = (int)(item - (int64_t)*r * per);
}

}  // namespace ctn
