// bmpow_tx_kernels.h -- device data layout and launch wrappers of the assembly of outgoing objects
// (bmpow_tx.hip), shared with its host unit (bmpow_host_tx.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bmpow_tx.h"
#include "bmpow_seal_kernels.h"
#include "bmpow_sig_kernels.h"

constexpr uint32_t TX_BLOCK = 64;       // one wave: 64 rows
constexpr uint32_t TX_PACK_LANES = 16;  // lanes that copy one row: 16 x 16 bytes = four SHA blocks a pass
static_assert(TX_BLOCK == SG_BLOCK && TX_BLOCK == SL_BLOCK, "the tx path reuses the signing and seal launches");
static_assert(sizeof(bmpow_tx_rec) == 152, "bmpow_tx_rec is 152 bytes without padding");

// One row as the host uploads it.  Its slot lies at byte 16 off16 of the pool, with the body at SL_PLAIN_AT
// of it; blk is the row's first block in the hash pool, where the host reserved
// txf::signed_blocks(head_len + body_len) blocks.
struct tx_row {
  uint32_t off16;
  uint32_t body_len;
  uint32_t blk;
  uint8_t head_len;  // 12 .. 62
  uint8_t kind;      // BMPOW_TX_SEALED / BMPOW_TX_CLEAR
  uint8_t digest;
  uint8_t pad;
  uint8_t head[64];  // zero behind head_len
};
static_assert(sizeof(tx_row) == 80, "tx_row is 80 bytes");

// Rows are indexed 0 .. n within a launch set, the sealed ones first (0 .. ns); stride >= n is n rounded up
// to TX_BLOCK.  pool_bytes / hpool_chunks: the buffers' sizes (nothing is read or written past them).
//   hpool[4 (blk + b) ..] : block b of the row's padded signed data; sigs[o].blk / .nblk: what sg_launch_hash reads
hipError_t tx_launch_pack(hipStream_t st, const tx_row* rows, const uint8_t* pool, uint64_t pool_bytes, uint32_t n,
                          uint4* hpool, uint64_t hpool_chunks, sg_sig* sigs);
//   rs[o], rs[stride + o], ok[o] : as sd_launch_sign leaves them
//   sl[o]                        : the seal's row: off16 as the tx row's, len = body_len + 1 + sig_len
//   recs[o]                      : sig, sig_len, plain_len, kind, digest; everything else zero
hipError_t tx_launch_tail(hipStream_t st, const tx_row* rows, const sn::sc* rs, const uint8_t* ok, uint32_t n,
                          uint32_t stride, uint8_t* pool, uint64_t pool_bytes, sl_row* sl, bmpow_tx_rec* recs);
//   blob_len[o], o < ns : sl_launch_seal's out_len
//   recs[o]             : status, obj_len and initial_hash
hipError_t tx_launch_finish(hipStream_t st, const tx_row* rows, const uint32_t* blob_len, uint32_t ns, const uint8_t* pool,
                            uint64_t pool_bytes, uint32_t n, bmpow_tx_rec* recs);
