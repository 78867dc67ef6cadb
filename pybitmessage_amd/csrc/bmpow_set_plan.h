// bmpow_set_plan.h -- where a launch set ends (host only, no HIP: tests/native/setplan_sim.cpp builds it with
// g++).  The receive-side host units send their rows, sorted by block count, through the device in sets of at
// most max_objects rows and max_pool_bytes of 64-byte blocks; this is the one rule that cuts them.  Used by
// bmpow_host_sig.hip, bmpow_host_rows.h (msgs and objects), ecies_set_end (bmpow_host_ecies.hip) and, for the
// rows it does not seal, bmpow_host_send.hip.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace bmhost {

struct SetCut {
  size_t i1;        // the set is rows[i0 .. i1)
  uint64_t blocks;  // the blocks its rows reserve together
};

// The set that starts at rows[i0] (rows: anything with size() and operator[]; bound(rows[i]): that row's
// blocks).  Rows are taken in order while fewer than max_objects are in the set and the next one's blocks still
// fit the pool.  The first row is always taken, so a row that is above the pool on its own forms a set of one
// (the caller's check of `blocks` decides what becomes of it).
template <class Rows, class Bound>
SetCut plan_set(const Rows& rows, size_t i0, Bound bound, size_t max_objects, uint64_t max_pool_bytes) {
  SetCut c{i0, 0};
  while (c.i1 < rows.size() && c.i1 - i0 < max_objects &&
         (c.i1 == i0 || (c.blocks + bound(rows[c.i1])) * 64 <= max_pool_bytes))
    c.blocks += bound(rows[c.i1++]);
  return c;
}

}  // namespace bmhost
