// bmpow_host_sig.h -- what the host units that run the signature kernels share (internal): the set limits,
// one call's device buffers and the verification launches of a set.  Used by bmpow_host_sig.hip
// (bmpow_sig_verify, bmpow_ecdsa_verify_digest) and, through bmpow_host_rows.h, by bmpow_host_rx.hip
// (bmpow_rx_msgs), bmpow_host_rxobj.hip (bmpow_rx_objects) and bmpow_host_rxopen.hip (bmpow_rx_sealed_msgs);
// the fixed-base comb table they all pass on is addr_comb16_table (bmpow_host.h).
#pragma once
#include "bmpow_host.h"

#include "bmpow_ecies_kernels.h"
#include "bmpow_set_plan.h"
#include "bmpow_sig_kernels.h"

namespace bmhost {

constexpr size_t kSigSetObjects = 1u << 18;  // as the ECIES sets: 4,096 waves, 128 MB of key tables
constexpr size_t kSigSetPoolBytes = 256ull << 20;

struct SigBufs {  // one call's buffers on the device
  DevBuf<sg_sig> sigs;
  DevBuf<uint4> pool;
  DevBuf<sn::sc> e;
  DevBuf<sg_kw> u1;
  DevBuf<int8_t> dig;
  DevBuf<uint8_t> flip, tinf, verdict;
  DevBuf<ec::ge> pts, tab;
  DevBuf<uint32_t> ok;
  DevBuf<sg_pt> T;
  Event ev[4];

  // Room for a set of stride rows (a multiple of SG_BLOCK) and pool_chunks of padded blocks in 16-byte units.
  int grow(Shard& sh, uint32_t stride, uint64_t pool_chunks);
};

// What follows the hash on sh.stream: scalars, key tables (ec_prep_kernel), ladder and combs, four launches
// over sigs, e and pts of n rows.  Between the scalars and the key tables `mid` is recorded: the boundary of
// every caller's scalar and curve phases.  The events around the four are the caller's own.
int sig_launch_verify(Shard& sh, SigBufs& b, const ec::ge* comb, uint32_t n, uint32_t stride, int nhash, const Event& mid);

}  // namespace bmhost
