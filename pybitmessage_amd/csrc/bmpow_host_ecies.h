// bmpow_host_ecies.h -- what the host units that run the ECIES trial decryption share (internal): the payload
// parse, the key recoding, one call's device buffers and the work of one set.  Used by bmpow_host_ecies.hip
// (bmpow_ecies_match) and bmpow_host_rxopen.hip (bmpow_rx_sealed_msgs), which goes on with the set's MAC pool,
// key_e and match[] where they lie on the device.
#pragma once
#include "bmpow_host.h"

#include "../../include/bmpow_ecies.h"
#include "bmpow_ecies_kernels.h"
#include "bmpow_set_plan.h"

namespace bmhost {

constexpr size_t kSetObjects = 1u << 18;  // 4,096 waves: every SIMD of an MI355X holds its 4 even with one key
constexpr size_t kSetPoolBytes = 256ull << 20;
constexpr size_t kLaunchPairs = 1u << 21;  // ~30 ms of ladder

struct U256 {
  uint64_t w[4];  // little-endian words
};

struct Parsed {
  U256 x, y;
  size_t body_off;
};

struct Item {  // a well-formed object
  uint32_t orig;
  uint32_t nblk;
  Parsed hdr;
};

struct EciesBufs {  // one call's buffers on the device
  DevBuf<ec::ge> pts, tab;
  DevBuf<uint32_t> ok;
  DevBuf<int32_t> dig;
  DevBuf<uint64_t> kout, key_e;
  DevBuf<ec_obj> objs;
  DevBuf<uint4> pool;
  DevBuf<int> match;
  DevBuf<ec::fe> x;
  Event ev[3];
};

struct EciesStage {  // one call's staging vectors on the host, reused from set to set
  std::vector<ec::ge> pts;
  std::vector<ec_obj> objs;
  std::vector<uint8_t> pool;
  std::vector<int> match;
};

U256 u256_from_be(const uint8_t* b);
bool key_in_range(const U256& k);
void recode_key(const U256& key, int32_t* dig);
bool ecies_parse(const uint8_t* p, size_t len, Parsed& out);
uint32_t mac_blocks(size_t maced_len);
int ecies_events(EciesBufs& b, int dev);

// Where the set that starts at items[i0] ends (at most kSetObjects objects and kSetPoolBytes of pool; items are
// sorted by nblk, descending); blocks: its MAC blocks.
size_t ecies_set_end(const std::vector<Item>& items, size_t i0, uint64_t& blocks);

// One set, items[0 .. n) with `blocks` MAC blocks between them (payloads / lens indexed by Item::orig): stage
// and upload the points, the ec_objs and the padded pool, the preparation launch, and for every group of keys
// the ladder, MAC and (with want_key_e) gather launches, b.dig holding every key's digits.  The abort flag is
// read before the preparation and between key groups.  The times, launches and pairs are added to st.  The
// download of match[0 .. n) into h.match is left enqueued on sh.stream: the caller synchronises.  b.pool,
// b.objs, b.key_e and b.match stay as the kernels left them.
int ecies_match_set(Shard& sh, EciesBufs& b, EciesStage& h, const Item* items, uint32_t n, uint64_t blocks,
                    const uint8_t* const* payloads, const uint64_t* lens, size_t n_keys, bool want_key_e,
                    bmpow_ecies_stats& st);

// The two halves of ecies_match_set, for a unit whose set holds rows that are not tried against every key
// (bmpow_host_rxobjopen.hip).  ecies_stage_set: the staging, the uploads, the two memsets and the preparation
// launch over all n rows, with room in b.kout for the key groups of n_keys keys (at least one key's).
// ecies_try_keys: the ladder, MAC and gather launches of every key group over rows 0 .. n of a set of n_set
// rows staged with the same n_keys; nothing is launched for n == 0.  Neither downloads match[].
int ecies_stage_set(Shard& sh, EciesBufs& b, EciesStage& h, const Item* items, uint32_t n, uint64_t blocks,
                    const uint8_t* const* payloads, const uint64_t* lens, size_t n_keys, bool want_key_e,
                    bmpow_ecies_stats& st);
int ecies_try_keys(Shard& sh, EciesBufs& b, uint32_t n, uint32_t n_set, size_t n_keys, bool want_key_e,
                   bmpow_ecies_stats& st);

}  // namespace bmhost
