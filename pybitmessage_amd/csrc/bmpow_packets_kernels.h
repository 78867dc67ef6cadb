// bmpow_packets_kernels.h -- launch wrappers of the packet kernels (bmpow_packets.hip), used by
// bmpow_host_packets.hip.  Rows as bmpow_packets_fmt.h lays them out: the n_obj object rows first, then the
// sum rows, each kind sorted by block count (descending) with its blocks back to back in the pool.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bmpow_layout.h"
#include "bmpow_packets_fmt.h"

// Rows [0, n): the pool's blocks of every row from the arena's bytes; for row k < n_obj also objs[k] =
// {blk, nblk, nonce}.  A row that does not lie inside the arena (arena_bytes) or whose blocks do not lie
// inside the pool (pool_blocks) writes no block, and an object row of that kind gets nblk = 0.
hipError_t pk_launch_pack(hipStream_t st, const pk_row* rows, uint32_t n, uint32_t n_obj, const uint4* arena,
                          uint64_t arena_bytes, uint4* pool, uint64_t pool_blocks, bv_obj* objs);
// Per object row k < n_obj: pow_out[k], inv_out[2k .. 2k+1] as bi_launch gives them, and sum_out[k] =
// SHA512(payload)[:4] as a big-endian number.  An object with nblk = 0 or blocks outside the pool gets zeros.
hipError_t pk_launch_object(hipStream_t st, const pk_row* rows, const bv_obj* objs, uint32_t n_obj, const uint4* pool,
                            uint64_t pool_blocks, uint64_t* pow_out, uint4* inv_out, uint32_t* sum_out);
hipError_t pk_launch_object_binned(hipStream_t st, const pk_row* rows, const bv_obj* objs, uint32_t n_obj,
                                   const uint4* pool, uint64_t pool_blocks, uint64_t* pow_out, uint4* inv_out,
                                   uint32_t* sum_out, const uint32_t* bins, uint32_t nbins);
// Per sum row j < n_sum (rows[j]): sum_out[j] the same way, 0 for a row whose blocks lie outside the pool.
hipError_t pk_launch_sum(hipStream_t st, const pk_row* rows, uint32_t n_sum, const uint4* pool, uint64_t pool_blocks,
                         uint32_t* sum_out);
