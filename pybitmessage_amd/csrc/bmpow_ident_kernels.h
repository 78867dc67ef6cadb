// bmpow_ident_kernels.h -- launch wrappers of the sender-identification kernels (bmpow_ident.hip), used by
// bmpow_host_ident.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bmpow_ident.h"

#define ID_BLOCK 64      // one wave per workgroup: rows are independent, small batches spread over the CUs
#define ID_REC_WORDS 45  // sizeof(bmpow_ident_rec) / 4

static_assert(sizeof(bmpow_ident_rec) == 4 * ID_REC_WORDS, "bmpow_ident_rec is 180 bytes without padding");

// keys: 8 uint4 per row (pub_signing64 || pub_encryption64); out: n records
hipError_t id_launch_derive(hipStream_t st, const uint4* keys, const uint64_t* versions, const uint64_t* streams,
                            uint32_t n, bmpow_ident_rec* out);
// ripes: 5 words per row, the ripe's bytes in memory order
hipError_t id_launch_from_ripe(hipStream_t st, const uint32_t* ripes, const uint64_t* versions, const uint64_t* streams,
                               uint32_t n, bmpow_ident_rec* out);
