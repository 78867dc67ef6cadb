// bmpow_rxopen_kernels.h -- device data layout and launch wrapper of the opening kernel (bmpow_rxopen.hip),
// shared with its host unit (bmpow_host_rxopen.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bmpow_rx_kernels.h"
#include "bmpow_rxobj_kernels.h"

constexpr uint32_t RXS_BLOCK = 64;  // one wave: 64 matched rows

// One matched row as the host uploads it beside its rx_row: where its ciphertext lies in the set's MAC pool.
struct rxs_row {
  uint32_t src;       // the row's index in the ECIES set: key_e[4 src ..] is its AES key
  uint32_t blk;       // its first 64-byte block in the MAC pool; the IV is that block's first 16 bytes
  uint32_t body_off;  // 22 + xl + yl: where the ciphertext starts behind the IV
  uint32_t clen;      // the ciphertext's length, a positive multiple of 16
};
static_assert(sizeof(rxs_row) == 16, "rxs_row is 16 bytes");

// Matched rows are indexed 0 .. n.  Row o decrypts pool[64 blk + body_off ..) of clen bytes under
// key_e[4 src .. 4 src + 4) (big-endian u64 words, as ec_launch_gather leaves them) into plain[rows[o].poff ..),
// a slot of clen bytes, and writes rows[o].plen (0 for bad padding) and opened[o] (the length, or -1).
// n_src: the rows key_e holds; pool_bytes / plain_bytes: the buffers' sizes; a row that would reach past any
// of them is refused (-1), not run.
hipError_t rxs_launch_open(hipStream_t st, const rxs_row* orows, const uint64_t* key_e, uint32_t n_src,
                           const uint8_t* pool, uint64_t pool_bytes, rx_row* rows, uint8_t* plain, uint64_t plain_bytes, uint32_t n,
                           int32_t* opened);
// The same for rows of the object family (rxo_row: a decrypted broadcast or v4 pubkey), for bmpow_host_rxobjopen.hip.
hipError_t rxo_launch_open(hipStream_t st, const rxs_row* orows, const uint64_t* key_e, uint32_t n_src,
                           const uint8_t* pool, uint64_t pool_bytes, rxo_row* rows, uint8_t* plain, uint64_t plain_bytes, uint32_t n,
                           int32_t* opened);
