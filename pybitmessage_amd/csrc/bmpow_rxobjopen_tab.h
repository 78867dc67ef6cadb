// bmpow_rxobjopen_tab.h -- what bmpow_rx_sealed_objects decides on the host before any key is tried (host only,
// no HIP: tests/native/rxobjopen_sim.cpp builds it with g++): the table that finds the entry filed under a
// 32-byte tag, and the walk of one object's head with the routing of processpubkey (:410).  Used by
// bmpow_host_rxobjopen.hip.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "bmpow_rx_fmt.h"

namespace bmhost {

// Tags (32 bytes each, entry after entry) -> the index of the FIRST entry with that tag.  Open addressing over a
// power of two of at least twice the entries, so a probe always ends at an empty slot; the hash is the tag's
// first eight bytes (a tag is the second half of a double SHA-512: uniform already), but nothing relies on that:
// colliding tags only probe further.
class TagTable {
 public:
  TagTable(const uint8_t* tags32, size_t n) : tags_(tags32), mask_(0) {
    if (n == 0) return;
    size_t cap = 4;
    while (cap < 2 * n) cap <<= 1;
    mask_ = cap - 1;
    slots_.assign(cap, -1);
    for (size_t i = 0; i < n; ++i) {
      size_t s = hash(tags32 + 32 * i) & mask_;
      while (slots_[s] >= 0 && memcmp(tags_ + 32 * (size_t)slots_[s], tags32 + 32 * i, 32) != 0) s = (s + 1) & mask_;
      if (slots_[s] < 0) slots_[s] = (int32_t)i;  // an entry whose tag is there already is never found
    }
  }
  // the index of the first entry filed under tag[0 .. 32), or -1
  int32_t find(const uint8_t* tag) const {
    if (slots_.empty()) return -1;
    size_t s = hash(tag) & mask_;
    while (slots_[s] >= 0) {
      if (memcmp(tags_ + 32 * (size_t)slots_[s], tag, 32) == 0) return slots_[s];
      s = (s + 1) & mask_;
    }
    return -1;
  }

 private:
  static size_t hash(const uint8_t* t) {
    uint64_t h;
    memcpy(&h, t, 8);
    return (size_t)(h * 0x9E3779B97F4A7C15ull >> 16);
  }
  const uint8_t* tags_;
  size_t mask_;
  std::vector<int32_t> slots_;
};

enum RouteClass : uint8_t {
  ROUTE_DONE = 0,      // the record is final as the host's walk left it: a head that refuses, a clear pubkey's refusal
  ROUTE_CLEAR = 1,     // a clear pubkey the walk accepts: uploaded as a row
  ROUTE_TRIAL = 2,     // a v4 broadcast: every trial key
  ROUTE_TAG = 3,       // a v5 broadcast with a whole tag: the key under it
  ROUTE_NEEDED = 4,    // a v4 pubkey of at least 350 bytes: the needed entry under its tag
  ROUTE_NO_TAG = 5,    // a tag that is not 32 whole bytes (the object's end cuts it short): in nobody's table
  ROUTE_V4_SHORT = 6,  // a v4 pubkey below 350 bytes (:411)
};

constexpr uint64_t kV4PubkeyMin = 350;  // src/class_objectProcessor.py:411

// The head of one object of kind BMPOW_RXO_KIND_BROADCAST or BMPOW_RXO_KIND_PUBKEY: rec as
// bmpow_rx_walk_object leaves it for the header alone (for the whole object where it is a clear pubkey), with
// rec.kind the kind after routing; the statuses that depend on tables and keys are the caller's.
inline RouteClass route_object(int kind, const uint8_t* obj, uint64_t len, bmpow_rx_obj_rec& rec) {
  const uint32_t hlen = (uint32_t)std::min<uint64_t>(len, rxf::kObjHeadBytes);
  memset(&rec, 0, sizeof rec);
  if (kind == BMPOW_RXO_KIND_BROADCAST) {
    rec.kind = BMPOW_RXO_KIND_BROADCAST;
    rxf::walk_broadcast_header(obj, hlen, rec);
    if (rec.status != BMPOW_RXO_OK) return ROUTE_DONE;
    if (rec.object_version == 4) return ROUTE_TRIAL;
    return rec.payload_off - rec.tag_off == 32 ? ROUTE_TAG : ROUTE_NO_TAG;
  }
  rxf::obj_walk w;
  rxf::walk_object(BMPOW_RXO_KIND_PUBKEY, obj, hlen, obj, len, rec, w);
  if (rec.status == BMPOW_RXO_OK) return ROUTE_CLEAR;
  if (rec.status != BMPOW_RXO_NEEDS_DECRYPTION) return ROUTE_DONE;
  memset(&rec, 0, sizeof rec);
  rec.kind = BMPOW_RXO_KIND_PUBKEY_V4;
  rxf::walk_pubkey_v4_header(obj, hlen, rec);
  if (len < kV4PubkeyMin) return ROUTE_V4_SHORT;
  // 350 bytes hold the 32 of the tag behind any two varints; a slice that is not 32 bytes is in no table, as a
  // v5 broadcast's
  return rec.payload_off - rec.tag_off == 32 ? ROUTE_NEEDED : ROUTE_NO_TAG;
}

}  // namespace bmhost
