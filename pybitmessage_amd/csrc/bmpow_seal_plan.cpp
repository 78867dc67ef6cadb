// bmpow_seal_plan.cpp -- see bmpow_seal_plan.h.
#include "bmpow_seal_plan.h"

#include <algorithm>

namespace bmseal {

int64_t plan_slots(size_t n, const uint64_t* slots, uint64_t max_rows, uint64_t max_bytes, uint32_t* set_out,
                   uint64_t* off_out) {
  if (max_rows == 0 || max_bytes == 0) return kPlanBadArg;
  if (n && (!slots || !set_out || !off_out)) return kPlanBadArg;
  uint64_t set = 0, rows = 0, bytes = 0;
  for (size_t i = 0; i < n; ++i) {
    const uint64_t s = slots[i];
    if (s % 16 || s > (1ull << 32)) return kPlanBadArg;
    // bytes <= max(max_bytes, 2^32) and s <= 2^32: the sum stays far below 2^64 whatever max_bytes is
    if (rows && (rows == max_rows || s > max_bytes || bytes > max_bytes - s)) {
      ++set;
      rows = bytes = 0;
    }
    if (set > 0xffffffffull) return kPlanBadArg;
    set_out[i] = (uint32_t)set;
    off_out[i] = bytes;
    bytes += s;
    ++rows;
  }
  return n ? (int64_t)set + 1 : 0;
}

int64_t plan_seal(size_t n, const uint64_t* lens, uint64_t max_rows, uint64_t max_bytes, uint32_t* set_out,
                  uint64_t* off_out) {
  if (n && !lens) return kPlanBadArg;
  std::vector<uint64_t> slots(n);
  for (size_t i = 0; i < n; ++i) {
    if (lens[i] > kMaxPlain) return kPlanBadArg;
    slots[i] = seal_slot_bytes(lens[i]);
  }
  return plan_slots(n, slots.data(), max_rows, max_bytes, set_out, off_out);
}

Sets cut_sets(const std::vector<uint32_t>& set, const std::vector<uint64_t>& off, const std::vector<uint64_t>& slots) {
  Sets s;
  const size_t n = set.size();
  for (size_t i = 0; i < n; ++i) {
    if (i == 0 || set[i] != set[i - 1]) s.begin.push_back(i);
    s.max_pool = std::max(s.max_pool, off[i] + slots[i]);
  }
  s.begin.push_back(n);
  for (size_t k = 0; k + 1 < s.begin.size(); ++k) s.max_rows = std::max(s.max_rows, s.begin[k + 1] - s.begin[k]);
  return s;
}

}  // namespace bmseal
