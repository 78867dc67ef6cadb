// bmpow_host_seal.h -- what the host units share of the device seal (bmpow_host_seal.hip): the mode knob,
// the counters, and one set's trip through the seal kernel, which bmpow_host_send.hip calls behind its
// ladder.  Internal.
#pragma once
#include "bmpow_host_sendkit.h"

#include "../../include/bmpow_send.h"
#include "bmpow_seal_kernels.h"
#include "bmpow_seal_plan.h"

namespace bmhost {

constexpr size_t kSealSetRows = 1u << 18;  // the send side's set: 4,096 waves
constexpr size_t kSealSetPoolBytes = 256ull << 20;

// The mode without BMPOW_SEAL in the environment: the device, which profiles/send/seal_ab_l200.json and
// seal_ab_l2000.json measured faster per call than the host's threads by 53 % and 21 % with identical blobs
// (send side).  -DBMPOW_SEAL_DEFAULT=0 builds a library that seals on the host unless told otherwise.
#ifndef BMPOW_SEAL_DEFAULT
#define BMPOW_SEAL_DEFAULT 1
#endif

extern bmpow_seal_stats g_seal_stats;  // under g_mu
int seal_mode();                       // 0: bmpow_ecies_encrypt seals on the host's threads, 1: on the device

// One call's pool and per-row arrays, on the device and on the host, for the seal kernel and for the CBC
// kernel (which also takes a key per row).  Sized once for the call's largest set.  The pools hold plaintext
// and the keys are keys: their owners zero them before they are released.
struct SealIo {
  WipeDevBuf<uint8_t> pool;
  WipeDevBuf<uint4> keys;  // CBC only: two per row
  DevBuf<sl_row> rows;
  DevBuf<uint4> iv;
  DevBuf<int32_t> out_len;  // CBC: -1 for a refused padding; the seal's lengths are below 2^31
  Event ev[4];
  WipedBytes host;  // the pool's staging copy: packed, uploaded, downloaded over, scattered
  Wiped<uint8_t> hkeys;
  std::vector<sl_row> hrows;
  std::vector<uint8_t> hiv;
  std::vector<int32_t> hlen;
  int init(int dev, size_t max_rows, uint64_t max_pool, bool with_keys = false);
};

// Rows 0 .. n of a set in device order: set row j is the caller's row row[j], its slot at off[j] of the pool.
struct SealSet {
  uint32_t n = 0, stride = 0;
  const uint32_t* row = nullptr;
  const uint64_t* off = nullptr;
  uint64_t pool_bytes = 0;
  const uint8_t* const* plains = nullptr;
  const uint64_t* lens = nullptr;
  const uint8_t* ivs = nullptr;  // 16 bytes per caller's row
  uint8_t* const* outs = nullptr;
  uint64_t* out_lens = nullptr;
};

// Pack the set's plaintexts (the host's threads; the stream may still be running what makes kout and pt),
// upload, seal, download, scatter into outs / out_lens; the stream is drained on return.  kout, pt, ok as
// sl_launch_seal takes them.
int seal_set(Shard& sh, SealIo& io, const SealSet& s, const uint64_t* kout, const ec::ge* pt, const uint32_t* ok);

}  // namespace bmhost
