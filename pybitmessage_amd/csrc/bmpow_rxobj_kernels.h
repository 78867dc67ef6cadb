// bmpow_rxobj_kernels.h -- device data layout and launch wrappers of the broadcast and pubkey processing
// (bmpow_rxobj.hip), shared with its host unit (bmpow_host_rxobj.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/bmpow_ident.h"
#include "../../include/bmpow_rx.h"
#include "bmpow_rx_fmt.h"
#include "bmpow_sig_kernels.h"

constexpr uint32_t RXO_PACK_LANES = 16;  // lanes that copy one row: 16 x 16 bytes = four SHA blocks a pass
constexpr uint8_t RXO_FLAG_REAL = 1;     // the row's own signature and key went to the curve kernels (no dummy)
constexpr uint8_t RXO_FLAG_DER = 2;      // the signature parsed: a broadcast's sigHash is computed

constexpr int RXO_REC_RIPE_WORD = 23;       // offsetof(bmpow_rx_obj_rec, ripe) / 4
constexpr int RXO_REC_BEHAVIOUR_WORD = 52;  // offsetof(bmpow_rx_obj_rec, behaviour) / 4; the four flag bytes follow

static_assert(sizeof(bmpow_rx_obj_rec) == 216, "bmpow_rx_obj_rec is 216 bytes without padding");
static_assert(offsetof(bmpow_rx_obj_rec, ripe) == 4 * RXO_REC_RIPE_WORD &&
                  offsetof(bmpow_rx_obj_rec, behaviour) == 4 * RXO_REC_BEHAVIOUR_WORD &&
                  offsetof(bmpow_rx_obj_rec, digest) == 4 * RXO_REC_BEHAVIOUR_WORD + 4 &&
                  offsetof(bmpow_rx_obj_rec, keys_hashed) == 4 * RXO_REC_BEHAVIOUR_WORD + 7,
              "bmpow_rx_obj_rec layout");

// One row as the host uploads it.  The plaintext (the object itself for BMPOW_RXO_KIND_PUBKEY) lies at byte
// poff of the plaintext pool, poff a multiple of 16, in a slot of plen rounded up to 16 bytes; blk is the
// row's first block in the padded pool, where the host reserved rxf::signed_blocks_bound_obj(plen) blocks.
struct rxo_row {
  uint64_t poff;
  uint32_t plen;
  uint32_t blk;
  uint8_t head[rxf::kObjHeadBytes];  // the object's first bytes
  uint8_t hlen;                      // how many of them there are
  uint8_t kind;                      // BMPOW_RXO_KIND_*
  uint8_t expect[32];
};
static_assert(sizeof(rxo_row) == 120, "rxo_row is 120 bytes");

struct rxo_pk {  // what the pack kernel needs of a row that is hashed (nblk == 0 otherwise)
  uint32_t pre[rxf::kObjPrefixWords];  // the prefix of signedData, bytes in memory order
  uint32_t plen;                       // its length
  uint32_t bottom;                     // source bytes behind it
  uint32_t skip;                       // where they start in the source: 8 for a clear pubkey, else 0
  uint32_t pad;
};

// Rows are indexed 0 .. n within a launch set; stride >= n is n rounded up to SG_BLOCK.  The outputs are
// those of rx_launch_walk (bmpow_rx_kernels.h), for the same consumers.
hipError_t rxo_launch_walk(hipStream_t st, const rxo_row* rows, const uint8_t* plain, uint32_t n, uint32_t stride,
                           bmpow_rx_obj_rec* recs, sg_sig* sigs, ec::ge* pts, uint4* keys, uint64_t* versions,
                           uint64_t* streams, rxo_pk* pk, uint8_t* flags);
// pool[4 (blk + b) ..]: block b < nblk of each row's padded signedData; plain_chunks / pool_chunks: the
// buffers' sizes in 16-byte units (nothing is read or written past them)
hipError_t rxo_launch_pack(hipStream_t st, const rxo_row* rows, const uint4* plain, uint64_t plain_chunks,
                           const sg_sig* sigs, const rxo_pk* pk, uint32_t n, uint4* pool, uint64_t pool_chunks);
// verdict[o]: sg_launch_comb's; ident[o]: id_launch_derive's
hipError_t rxo_launch_finish(hipStream_t st, const rxo_row* rows, const uint8_t* plain, const uint8_t* verdict,
                             const uint8_t* flags, const bmpow_ident_rec* ident, uint32_t n, bmpow_rx_obj_rec* recs);
