// bmpow_seal_kernels.h -- device data layout and launch wrappers of the ECIES seal and the raw AES-256-CBC
// (bmpow_seal.hip), shared with the host units (bmpow_host_send.hip, bmpow_host_ecies.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "secp256k1_dev.h"

constexpr uint32_t SL_BLOCK = 64;  // one wave: 64 rows

// One row's slot in the set's pool (bmpow_seal_rows.h) and the length of what the host put there.
struct sl_row {
  uint32_t off16;  // the slot's offset in 16-byte units
  uint32_t len;    // seal, CBC encrypt: plaintext bytes; CBC decrypt: ciphertext bytes, a positive multiple of 16
};

// Rows are indexed 0 .. n within a launch set, sorted by block count, descending; stride >= n is n rounded
// up to SL_BLOCK.
//   kout[w * stride + o] : word w (big-endian u64) of key_e || key_m, as sd_shared_kernel leaves it
//   pt[o]                : the ephemeral public key R, affine, as sd_comb_kernel leaves it
//   ok[o]                : 0 for a row ec_prep_kernel refused (no blob, out_len 0); ok == nullptr: every row
//   iv[o]                : the IV's 16 bytes
//   pool                 : rows[o]'s slot holds the plaintext at SL_PLAIN_AT (seal) or the message at 0 (CBC);
//                          the kernel leaves the blob (the output) at the slot's start
//   out_len[o]           : seal: the blob's length; CBC: the output's length, -1 for bad padding
// The slots come from bmseal::seal_slot_bytes / cbc_len (bmpow_seal_plan.h); pool_bytes bounds them all.
hipError_t sl_launch_seal(hipStream_t st, const uint64_t* kout, const ec::ge* pt, const uint32_t* ok, const uint4* iv,
                          const sl_row* rows, uint8_t* pool, uint32_t n, uint32_t stride, uint32_t* out_len);
//   keys[2 o], keys[2 o + 1] : the key's 32 bytes
hipError_t sl_launch_cbc(hipStream_t st, int decrypt, const uint4* keys, const uint4* iv, const sl_row* rows, uint8_t* pool,
                         uint32_t n, uint32_t stride, int32_t* out_len);
