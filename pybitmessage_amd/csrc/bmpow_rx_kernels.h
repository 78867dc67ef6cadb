// bmpow_rx_kernels.h -- device data layout and launch wrappers of the msg processing (bmpow_rx.hip),
// shared with the host units of the msg family (bmpow_host_rx.h: bmpow_host_rx.hip, bmpow_host_rxopen.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bmpow_ident.h"
#include "../../include/bmpow_rx.h"
#include "bmpow_sig_kernels.h"

constexpr uint32_t RX_PACK_LANES = 16;  // lanes that copy one row: 16 x 16 bytes = four SHA blocks a pass
constexpr uint32_t RX_REC_WORDS = 52;   // sizeof(bmpow_rx_msg_rec) / 4
constexpr uint8_t RX_FLAG_REAL = 1;     // the row's own signature and key went to the curve kernels (no dummy)
constexpr uint8_t RX_FLAG_DER = 2;      // the signature parsed: sigHash is computed

static_assert(sizeof(bmpow_rx_msg_rec) == 4 * RX_REC_WORDS, "bmpow_rx_msg_rec is 208 bytes without padding");

// One row as the host uploads it.  The plaintext lies at byte poff of the plaintext pool, poff a multiple
// of 16, in a slot of plen rounded up to 16 bytes; blk is the row's first block in the padded pool, where
// the host reserved rxf::signed_blocks_bound(plen) blocks.
struct rx_row {
  uint64_t poff;
  uint32_t plen;
  uint32_t blk;
  uint8_t head[38];  // the object's first bytes
  uint8_t hlen;      // how many of them there are
  uint8_t pad0;
  uint8_t to_ripe[20];
  uint8_t pad1[4];
};
static_assert(sizeof(rx_row) == 80, "rx_row is 80 bytes");

struct rx_pk {  // what the pack kernel needs of a row the walk accepted (nblk == 0 otherwise)
  uint32_t pre[6];  // the prefix of signedData, bytes in memory order
  uint32_t plen;    // its length
  uint32_t bottom;  // plaintext bytes behind it
};

// Rows are indexed 0 .. n within a launch set; stride >= n is n rounded up to SG_BLOCK.
//   recs[o]          : the walked fields and the walk's status
//   sigs[o], pts[o]  : r, s, blk, nblk and the signing key for sg_launch_* / ec_launch_prep; a row that is
//                      not verified as it stands gets r = s = 1, nblk = 0 and the generator
//   keys[8 o ..]     : the two keys' 128 bytes, versions[o], streams[o]: what id_launch_derive reads
//   flags[o]         : RX_FLAG_*
hipError_t rx_launch_walk(hipStream_t st, const rx_row* rows, const uint8_t* plain, uint32_t n, uint32_t stride,
                          bmpow_rx_msg_rec* recs, sg_sig* sigs, ec::ge* pts, uint4* keys, uint64_t* versions,
                          uint64_t* streams, rx_pk* pk, uint8_t* flags);
// pool[4 (blk + b) ..]: block b < nblk of each row's padded signedData; plain_chunks / pool_chunks: the
// buffers' sizes in 16-byte units (nothing is read or written past them)
hipError_t rx_launch_pack(hipStream_t st, const rx_row* rows, const uint4* plain, uint64_t plain_chunks,
                          const sg_sig* sigs, const rx_pk* pk, uint32_t n, uint4* pool, uint64_t pool_chunks);
// verdict[o]: sg_launch_comb's; ident[o]: id_launch_derive's
hipError_t rx_launch_finish(hipStream_t st, const rx_row* rows, const uint8_t* plain, const uint8_t* verdict,
                            const uint8_t* flags, const bmpow_ident_rec* ident, uint32_t n, bmpow_rx_msg_rec* recs);
