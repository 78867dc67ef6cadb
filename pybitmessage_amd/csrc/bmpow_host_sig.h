// bmpow_host_sig.h -- what the host units that run the signature kernels share (internal): the set limits
// and one call's device buffers.  Used by bmpow_host_sig.hip (bmpow_sig_verify, bmpow_ecdsa_verify_digest)
// and bmpow_host_rx.hip (bmpow_rx_msgs); the fixed-base comb table they both pass to sg_launch_comb is
// addr_comb16_table (bmpow_host.h).
#pragma once
#include "bmpow_host.h"

#include "bmpow_ecies_kernels.h"
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
};

inline int sig_elapsed(double& acc, const Event& a, const Event& b) {
  float ms = 0;
  HIPTRY(hipEventElapsedTime(&ms, a.get(), b.get()));
  acc += ms;
  return 0;
}

}  // namespace bmhost
