// bmpow_sig_kernels.h -- device data layout and launch wrappers of the signature verification
// (bmpow_sig.hip), shared with the host units that launch them (bmpow_host_sig.hip; bmpow_host_rows.h for
// the receive side's rows) and with the kernels that write their inputs (bmpow_rx_dev.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scalar_dev.h"
#include "secp256k1_dev.h"

constexpr uint32_t SG_BLOCK = 64;  // one wave: 64 signatures
constexpr int SG_DIGITS = 64;      // signed odd base-16 digits of u2, one int8 each

// One parsed signature: 1 <= r, s < n as little-endian limbs, and its message in the pool, padded as
// SHA-1 and SHA-256 both pad (data || 0x80 || zeros || the bit length), in 64-byte blocks.
struct sg_sig {
  sn::sc r, s;
  uint32_t blk;   // first 64-byte block in the pool
  uint32_t nblk;  // ceil((len + 9) / 64), >= 1; 0 when the digest is given (bmpow_ecdsa_verify_digest)
};

struct sg_kw {  // a scalar as the fixed-base comb takes it: 4 big-endian 64-bit words
  uint64_t w[4];
};

struct sg_pt {  // u2 Q in Jacobian coordinates
  ec::fe x, y, z;
};

// Signatures are indexed 0 .. n within a launch set; stride >= n is n rounded up to SG_BLOCK.
//   e[h * stride + o]         : the digest as an integer (little-endian limbs, not reduced); h = 0 SHA-1
//                               (or the caller's digest), h = 1 SHA-256
//   u1[h * stride + o]        : e_h / s mod n
//   dig[i * stride + o]       : digit i of u2 = r / s mod n, made odd
//   flip[o]                   : 1 when the digits are those of n - u2 (the ladder's result is negated)
//   T[o], tinf[o]             : u2 Q and whether it is the point at infinity
//   verdict[o]                : 0 invalid, 1 valid under digest 0, 2 valid under digest 1 only
// nhash is 2 for bmpow_sig_verify and 1 for bmpow_ecdsa_verify_digest.
hipError_t sg_launch_hash(hipStream_t st, const sg_sig* sigs, const uint4* pool, uint32_t n, uint32_t stride, sn::sc* e);
hipError_t sg_launch_scalars(hipStream_t st, const sg_sig* sigs, const sn::sc* e, uint32_t n, uint32_t stride, int nhash,
                             sg_kw* u1, int8_t* dig, uint8_t* flip);
hipError_t sg_launch_ladder(hipStream_t st, const ec::ge* tab, uint32_t n, uint32_t stride, const int8_t* dig,
                            const uint8_t* flip, sg_pt* T, uint8_t* tinf);
// table: the 16-bit fixed-base comb (table[i << 16 | v] = v 2^(16 i) G); ok[o]: the key is on the curve
hipError_t sg_launch_comb(hipStream_t st, const ec::ge* table, const sg_sig* sigs, const sg_kw* u1, const sg_pt* T,
                          const uint8_t* tinf, const uint32_t* ok, uint32_t n, uint32_t stride, int nhash,
                          uint8_t* verdict);
