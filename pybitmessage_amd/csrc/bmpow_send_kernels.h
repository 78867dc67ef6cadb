// bmpow_send_kernels.h -- device data layout and launch wrappers of the batched signing and ECIES
// encryption (bmpow_send.hip), shared with its host unit (bmpow_host_send.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bmpow_sig_kernels.h"

constexpr uint32_t SD_BLOCK = 64;  // one wave: 64 rows
static_assert(SD_BLOCK == SG_BLOCK, "the send path reuses the signature path's hash and table launches");

// Rows are indexed 0 .. n within a launch set; stride >= n is n rounded up to SD_BLOCK.
//   kw[o]                : the row's scalar in [1, n - 1] (the private key, the signature's nonce or the
//                          ephemeral key), 4 big-endian words
//   pt[o]                : kw[o] G, affine and canonical
//   d[o], e[o]           : the signing key and the digest as an integer (little-endian limbs; e not reduced)
//   rs[o], rs[stride + o]: r and s;  ok[o] = 0 when either is zero
//   dig[i * stride + o]  : digit i of kw[o] made odd (the sign flip dropped: only x(kw Q) is used)
//   kout[w * stride + o] : word w (big-endian u64) of SHA512(x(kw[o] Q_o)); words 0..3 key_e, 4..7 key_m
// table: the 16-bit fixed-base comb (table[i << 16 | v] = v 2^(16 i) G)
hipError_t sd_launch_comb(hipStream_t st, const ec::ge* table, const sg_kw* kw, uint32_t n, uint32_t stride, ec::ge* pt);
hipError_t sd_launch_sign(hipStream_t st, const ec::ge* pt, const sg_kw* kw, const sn::sc* d, const sn::sc* e, uint32_t n,
                          uint32_t stride, sn::sc* rs, uint8_t* ok);
hipError_t sd_launch_digits(hipStream_t st, const sg_kw* kw, uint32_t n, uint32_t stride, int8_t* dig);
// tab: ec_launch_prep's tables of the recipient points (the generator's where prep refused the point)
hipError_t sd_launch_shared(hipStream_t st, const ec::ge* tab, uint32_t n, uint32_t stride, const int8_t* dig,
                            uint64_t* kout);
