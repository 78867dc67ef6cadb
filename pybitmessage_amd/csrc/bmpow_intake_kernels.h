// bmpow_intake_kernels.h -- launch wrappers of the object-intake kernels (bmpow_intake.hip), used by
// bmpow_host_intake.hip.  Same pool, descriptors and bins as the verification kernels (bmpow_kernels.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bmpow_layout.h"

// Per sorted object k: pow_out[k] = the receive-side POW value (as bv_launch_pow), inv_out[2k .. 2k+1] =
// the 32 bytes of SHA512(SHA512(object))[:32].  lens[k] = the object's length in bytes (nonce included).
hipError_t bi_launch(hipStream_t st, const bv_obj* objs, const uint32_t* lens, uint32_t n, const uint4* pool,
                     uint64_t* pow_out, uint4* inv_out);
hipError_t bi_launch_binned(hipStream_t st, const bv_obj* objs, const uint32_t* lens, uint32_t n, const uint4* pool,
                            uint64_t* pow_out, uint4* inv_out, const uint32_t* bins, uint32_t nbins);
