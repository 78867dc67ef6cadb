// bmpow_host_sendkit.h -- what the send side's host units share (internal): bmpow_host_send.hip (keys,
// signatures, ECIES encryption), bmpow_host_tx.hip (outgoing objects in one call) and bmpow_host_seal.hip (the
// seal and CBC kernels' round trip).  Small arithmetic and the wall-clock guard, the conversions into the
// kernels' types, the ECIES key agreement of a set over buffers that wipe themselves (KeySet), and the loop
// that signs the rare row with r = 0 or s = 0 again.  The scalar and byte toolkit is bmpow_host_scalar.h.
#pragma once
#include "bmpow_host.h"

#include "bmpow_ecies_kernels.h"
#include "bmpow_host_scalar.h"
#include "bmpow_send_kernels.h"

namespace bmhost {

constexpr int kSignPasses = 3;  // a call signs at most this often: a row fails one pass in 2^127

inline uint32_t round_up(uint32_t n, uint32_t q) { return (n + q - 1) / q * q; }

inline double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

struct WallClock {  // a call's wall time into acc (a counter under g_mu), on every return path
  double& acc;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  ~WallClock() { acc += ms_since(t0); }
};

inline sg_kw kw_from_be(const uint8_t* b) {  // 32 big-endian bytes as the fixed-base comb takes a scalar
  sg_kw k;
  for (int i = 0; i < 4; ++i) k.w[i] = bmsched::load_be64(b + 8 * i);
  return k;
}

inline ec::ge ge_from_be(const uint8_t xy[64]) {  // X || Y, big-endian, into little-endian limbs
  ec::ge g;
  const sc x = sc_from_be(xy), y = sc_from_be(xy + 32);
  for (int i = 0; i < 8; ++i) g.x.d[i] = x.d[i], g.y.d[i] = y.d[i];
  return g;
}

// The ECIES key agreement of a set of rows: an ephemeral key kw and a recipient point pts per row in;
// R = kw G (pt), SHA512(x(kw Q)) (kout, as sd_launch_shared lays it out) and whether Q is on the curve (ok32)
// out.  Sized once per call for its largest set; what held a key is zeroed before it is released, on the
// device (WipeDevBuf) and on the host (Wiped).  Without recipients (alloc's last argument) only kw and pt
// exist: the comb alone, for public keys and for a signature's k G.
struct KeySet {
  WipeDevBuf<sg_kw> kw;
  DevBuf<ec::ge> pt, pts, tab;
  WipeDevBuf<int8_t> dig;
  WipeDevBuf<uint64_t> kout;
  DevBuf<uint32_t> ok32;
  Wiped<sg_kw> hkw;
  std::vector<ec::ge> hpts;

  int alloc(int dev, size_t cap_stride, bool recipients = true) {
    if (cap_stride == 0) return 0;
    HIPTRY(kw.alloc(dev, cap_stride));
    HIPTRY(pt.alloc(dev, cap_stride));
    hkw.v.resize(cap_stride);
    if (!recipients) return 0;
    HIPTRY(pts.alloc(dev, cap_stride));
    HIPTRY(tab.alloc(dev, (size_t)EC_ENTRIES * cap_stride));
    HIPTRY(dig.alloc(dev, (size_t)SG_DIGITS * cap_stride));
    HIPTRY(kout.alloc(dev, (size_t)8 * cap_stride));
    HIPTRY(ok32.alloc(dev, cap_stride));
    hpts.resize(cap_stride);
    return 0;
  }
  // row j of the set: its scalar (32 bytes) and, with recipients, its point (X || Y)
  void stage(size_t j, const uint8_t* scalar, const uint8_t* pub) {
    hkw.v[j] = kw_from_be(scalar);
    if (pub) hpts[j] = ge_from_be(pub);
  }
  int upload(hipStream_t st, uint32_t n) {
    HIPTRY(hipMemcpyAsync(kw.get(), hkw.v.data(), n * sizeof(sg_kw), hipMemcpyHostToDevice, st));
    if (pts) HIPTRY(hipMemcpyAsync(pts.get(), hpts.data(), n * sizeof(ec::ge), hipMemcpyHostToDevice, st));
    return 0;
  }
  // the ephemeral half: R = kw G, then kw's digits; `mid`, if given, is recorded between the two
  int launch_ephemeral(hipStream_t st, const ec::ge* comb, uint32_t n, uint32_t stride, const Event* mid = nullptr) {
    HIPTRY(sd_launch_comb(st, comb, kw.get(), n, stride, pt.get()));
    if (mid) HIPTRY(hipEventRecord(mid->get(), st));
    HIPTRY(sd_launch_digits(st, kw.get(), n, stride, dig.get()));
    return 0;
  }
  // the recipient half: the points' tables, then the ladder and the key derivation
  int launch_shared(hipStream_t st, uint32_t n, uint32_t stride) {
    HIPTRY(ec_launch_prep(st, pts.get(), n, stride, tab.get(), ok32.get()));
    HIPTRY(sd_launch_shared(st, tab.get(), n, stride, dig.get(), kout.get()));
    return 0;
  }
};

// The sign-again loop: run(rows) signs the rows; failed(row) says whether a row came back with r = 0 or
// s = 0.  Those draw another nonce into drawn[32 row ..) and go again, kSignPasses passes at the most.  With
// the caller's own nonces (drawn == nullptr) there is one pass.
template <class Run, class Failed>
int sign_passes(std::vector<uint32_t>& rows, uint8_t* drawn, Run run, Failed failed) {
  for (int pass = 0; pass < kSignPasses && !rows.empty(); ++pass) {
    if (const int rc = run(rows); rc < 0) return rc;
    if (!drawn) break;
    std::vector<uint32_t> again;
    for (uint32_t row : rows)
      if (failed(row)) again.push_back(row);
    for (uint32_t row : again)
      if (!draw_scalar(drawn + 32 * (size_t)row)) return set_err(BMPOW_E_ARG, "RAND_bytes failed");
    rows.swap(again);
  }
  return 0;
}

}  // namespace bmhost
