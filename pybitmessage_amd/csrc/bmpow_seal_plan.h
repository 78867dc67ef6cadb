// bmpow_seal_plan.h -- how the rows of a seal or CBC call are laid out in device sets (host only, no HIP:
// plain g++ compiles it; tests/native/seal_sim.cpp runs it under the sanitizers).
//
// A call's rows, in the order they go to the device (sorted by block count, descending), are cut into
// sets of at most max_rows rows and max_bytes of pool; inside a set every row owns a slot of the pool, a
// multiple of 16 bytes at a multiple of 16.  A row whose slot alone is above max_bytes gets a set of its
// own.  All sums are in 64 bits over lengths checked to be at most kMaxPlain, so no offset wraps.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

// Where the host puts a row's plaintext in its seal slot: the first multiple of 16 not below the longest
// head (86 bytes), so the ciphertext written behind the head never reaches a block still to be read.
constexpr uint32_t SL_PLAIN_AT = 96;

namespace bmseal {

constexpr uint64_t kMaxPlain = 0x7fffffffu - 16;  // bmpow_ecies_seal's bound on a plaintext
constexpr uint64_t kDevicePlain = 256u << 10;     // the protocol's object limit: longer rows are sealed on the host
constexpr int64_t kPlanBadArg = -3;               // BMPOW_E_ARG

inline uint64_t cbc_len(uint64_t len) { return 16 * (len / 16 + 1); }  // PKCS#7: always one more byte at least

// The seal kernel's slot (bmpow_seal_rows.h): the plaintext at 96, the blob of at most 86 + clen + 32 bytes,
// and the inner hash's padded blocks, ceil((86 + clen + 9) / 64) * 64.
inline uint64_t seal_slot_bytes(uint64_t len) {
  const uint64_t clen = cbc_len(len), hashed = (clen + 95 + 63) / 64 * 64, blob = clen + 118;
  static_assert(SL_PLAIN_AT <= 118, "the plaintext's end lies inside the blob's bound");
  return ((hashed > blob ? hashed : blob) + 15) / 16 * 16;
}

// slots[i]: the slot of row i in bytes, a multiple of 16.  set_out[i] = the row's set (counted from 0, never
// decreasing), off_out[i] = its slot's offset in that set's pool.  Returns the number of sets, or
// kPlanBadArg for a zero limit or a slot that is no multiple of 16.
int64_t plan_slots(size_t n, const uint64_t* slots, uint64_t max_rows, uint64_t max_bytes, uint32_t* set_out,
                   uint64_t* off_out);

// The same over plaintext lengths with seal_slot_bytes; a length above kMaxPlain is kPlanBadArg.
int64_t plan_seal(size_t n, const uint64_t* lens, uint64_t max_rows, uint64_t max_bytes, uint32_t* set_out,
                  uint64_t* off_out);

// The sets of a planned call: rows begin[k] .. begin[k + 1] are set k (begin ends at the number of rows), with
// the largest set's rows and the largest pool, what a call's buffers are sized for once.
struct Sets {
  std::vector<size_t> begin;
  uint64_t max_pool = 16;
  size_t max_rows = 0;
  size_t count() const { return begin.empty() ? 0 : begin.size() - 1; }
};

// From plan_slots' results: set[i], off[i] and the slots[i] it was given.
Sets cut_sets(const std::vector<uint32_t>& set, const std::vector<uint64_t>& off, const std::vector<uint64_t>& slots);

// A call's whole plan: the caller fills slot[], plan() lays the rows out and cuts the sets.
struct SlotPlan {
  std::vector<uint64_t> slot, off;
  std::vector<uint32_t> set;
  Sets sets;
  bool plan(uint64_t max_rows, uint64_t max_bytes) {  // false where plan_slots refuses
    off.resize(slot.size()), set.resize(slot.size());
    if (plan_slots(slot.size(), slot.data(), max_rows, max_bytes, set.data(), off.data()) < 0) return false;
    sets = cut_sets(set, off, slot);
    return true;
  }
  uint64_t pool_bytes(size_t k) const {  // of set k
    const size_t last = sets.begin[k + 1] - 1;
    return off[last] + slot[last];
  }
};

}  // namespace bmseal
