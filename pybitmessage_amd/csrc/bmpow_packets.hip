// bmpow_packets.hip -- packet kernels (gfx950): the padded block pool written on the device from the raw
// connection buffers, and per packet SHA512(payload)[:4] -- for an `object` packet out of the intake's own
// chain, with its receive-side POW value and inventory hash (include/bmpow_packets.h).
//
// Reference: state_bm_command, src/network/bmproto.py:106-111 (the checksum); for the object rows what
// bmpow_intake.hip restates.  Host side: bmpow_host_packets.hip.
//
//   pk_pack_kernel   : 16 lanes per row write data || 0x80 || zeros || bit length into the row's pool blocks,
//                      16 bytes per lane and pass, from two aligned 16-byte loads of the arena funnelled by
//                      the source's byte offset mod 16 (bmpow_packets_fmt.h, the text the host test runs); an
//                      object row's data is object[8:], and its nonce goes into its bv_obj: the device's
//                      counterpart of the host's pad_range.
//   pk_object_kernel : one lane per object row, sorted and binned forms as bi_intake_*: intake_chain with the
//                      checksum tapped where the inventory chain ends (bmpow_intake_dev.h).
//   pk_sum_kernel    : one lane per sum row: one plain SHA-512 chain over its pool blocks, four bytes out.
// Every index is checked against the arena's and the pool's size before it is used; lanes past n do nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bmpow_intake_dev.h"
#include "bmpow_packets_kernels.h"
#include "sha512_dev.h"

using namespace bm;

__global__ __launch_bounds__(64) void pk_pack_kernel(const pk_row* __restrict__ rows, uint32_t n, uint32_t n_obj,
                                                     const uint4* __restrict__ arena, uint64_t arena_bytes,
                                                     uint4* __restrict__ pool, uint64_t pool_blocks,
                                                     bv_obj* __restrict__ objs) {
  const uint32_t r = blockIdx.x * (64 / PK_PACK_LANES) + threadIdx.x / PK_PACK_LANES;
  const uint32_t sub = threadIdx.x % PK_PACK_LANES;
  if (r >= n) return;
  const pk_row row = rows[r];
  const uint32_t m = pkf::row_data_len(row.kind, row.len);
  uint32_t nblk = pkf::row_blocks(row.kind, row.len);
  if (row.kind > PK_SUM || (uint64_t)row.src + row.len > arena_bytes || (uint64_t)row.blk + nblk > pool_blocks)
    nblk = 0;  // never
  const uint8_t* bytes = reinterpret_cast<const uint8_t*>(arena);
  if (r < n_obj && sub == 0) {
    uint64_t nonce = 0;
    if (nblk)
      for (int i = 0; i < 8; ++i) nonce = nonce << 8 | bytes[(uint64_t)row.src + i];
    bv_obj o;
    o.blk = row.blk, o.nblk = nblk, o.nonce = nonce;
    objs[r] = o;
  }
  const uint64_t s = (uint64_t)row.src + (row.kind == PK_OBJECT ? 8u : 0u);
  const uint64_t arena_chunks = (arena_bytes + 15) >> 4;  // the arena's allocation holds whole chunks
  const uint64_t base = 8ull * row.blk;
#pragma unroll 1
  for (uint32_t c = sub; c < 8 * nblk; c += PK_PACK_LANES) {
    uint32_t w[4];
    pkf::pack_chunk(c, nblk, reinterpret_cast<const uint32_t*>(arena), arena_chunks, s, m, w);
    pool[base + c] = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

BM_DEV void object_store(uint32_t k, const pk_row* __restrict__ rows, const bv_obj* __restrict__ objs,
                         const uint4* __restrict__ pool, uint64_t pool_blocks, uint64_t* __restrict__ pow_out,
                         uint4* __restrict__ inv_out, uint32_t* __restrict__ sum_out) {
  const bv_obj o = objs[k];
  const uint32_t L = rows[k].len;
  uint64_t pow = 0, inv[4] = {0, 0, 0, 0};
  sum_out[k] = 0;
  // the pack's own bounds, once more: the chain never reads outside blocks [o.blk, o.blk + o.nblk)
  if (o.nblk != 0 && o.nblk == pkf::row_blocks(PK_OBJECT, L) && (uint64_t)o.blk + o.nblk <= pool_blocks)
    intake_chain<true>(o, L, pool, pow, inv, sum_out + k);
  pow_out[k] = pow;
  inv_out[2 * (uint64_t)k] = make_uint4(__builtin_bswap32(hi32(inv[0])), __builtin_bswap32(lo32(inv[0])),
                                        __builtin_bswap32(hi32(inv[1])), __builtin_bswap32(lo32(inv[1])));
  inv_out[2 * (uint64_t)k + 1] = make_uint4(__builtin_bswap32(hi32(inv[2])), __builtin_bswap32(lo32(inv[2])),
                                            __builtin_bswap32(hi32(inv[3])), __builtin_bswap32(lo32(inv[3])));
}

// One wave per group of BV_BLOCK object rows, the groups dispatched in sorted order (small calls).
__global__ __launch_bounds__(BV_BLOCK) void pk_object_kernel(const pk_row* __restrict__ rows,
                                                             const bv_obj* __restrict__ objs, uint32_t n,
                                                             const uint4* __restrict__ pool, uint64_t pool_blocks,
                                                             uint64_t* __restrict__ pow_out, uint4* __restrict__ inv_out,
                                                             uint32_t* __restrict__ sum_out) {
  const uint32_t k = blockIdx.x * BV_BLOCK + threadIdx.x;
  if (k >= n) return;
  object_store(k, rows, objs, pool, pool_blocks, pow_out, inv_out, sum_out);
}

// Floods: bi_intake_binned_kernel's shape over plan_bins' bins -- one 1024-thread workgroup per CU (its LDS
// request admits no second one), each wave taking groups from the bin of the SIMD it runs on, then from the
// CU's other bins, with the issue priority raised for a bin's first (longest) group.
constexpr uint32_t kPkBinnedLdsWords = (96u << 10) / 4;  // > half of the CU's 160 KiB

__global__ __launch_bounds__(BV_BINNED_WG) void pk_object_binned_kernel(
    const pk_row* __restrict__ rows, const bv_obj* __restrict__ objs, uint32_t n, const uint4* __restrict__ pool,
    uint64_t pool_blocks, uint64_t* __restrict__ pow_out, uint4* __restrict__ inv_out, uint32_t* __restrict__ sum_out,
    const uint32_t* __restrict__ bins, uint32_t nbins) {
  __shared__ uint32_t heads[kPkBinnedLdsWords];  // [0..3]: next group of each of the CU's 4 bins
  if (threadIdx.x < 4) heads[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63;
  // s_getreg_b32 hwreg(HW_REG_HW_ID, 4, 2): SIMD_ID of this wave
  const uint32_t simd = __builtin_amdgcn_s_getreg((1u << 11) | (4u << 6) | 4u) & 3u;
  const uint32_t* list = bins + nbins + 1;
  const uint32_t ngroups = (n + BV_BLOCK - 1) / BV_BLOCK;
  for (uint32_t t = 0; t < 4; ++t) {
    const uint32_t s = (simd + t) & 3u;
    const uint32_t b = blockIdx.x * 4 + s;
    const uint32_t lo = bins[b], hi = bins[b + 1];
    const uint32_t cnt = hi >= lo && hi <= ngroups ? hi - lo : 0;  // offsets into a list of ngroups entries
    for (;;) {
      uint32_t idx = 0;
      if (lane == 0) idx = atomicAdd(&heads[s], 1u);
      idx = __builtin_amdgcn_readfirstlane(idx);
      if (idx >= cnt) break;
      const uint32_t g = list[lo + idx];
      const uint32_t k = g * BV_BLOCK + lane;
      if (idx == 0) __builtin_amdgcn_s_setprio(3);
      if (g < ngroups && k < n) object_store(k, rows, objs, pool, pool_blocks, pow_out, inv_out, sum_out);
      if (idx == 0) __builtin_amdgcn_s_setprio(0);
    }
  }
}

__global__ __launch_bounds__(BV_BLOCK) void pk_sum_kernel(const pk_row* __restrict__ rows, uint32_t n,
                                                          const uint4* __restrict__ pool, uint64_t pool_blocks,
                                                          uint32_t* __restrict__ sum_out) {
  const uint32_t j = blockIdx.x * BV_BLOCK + threadIdx.x;
  if (j >= n) return;
  const pk_row row = rows[j];
  uint32_t nblk = pkf::row_blocks(PK_SUM, row.len);
  if ((uint64_t)row.blk + nblk > pool_blocks) nblk = 0;  // never
  uint64_t h[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) h[i] = IV(i);
  const uint4* p = pool + 8ull * row.blk;
#pragma unroll 1
  for (uint32_t b = 0; b < nblk; ++b, p += 8) {
    uint64_t w[16];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const uint4 v = p[q];
      w[2 * q] = be64(v.x, v.y);
      w[2 * q + 1] = be64(v.z, v.w);
    }
    compress(h, w);
  }
  sum_out[j] = nblk ? hi32(h[0]) : 0u;
}

// ---------------------------------------------------------------------------------------
// Launch wrappers (C++ linkage, used by bmpow_host_packets.hip).
// ---------------------------------------------------------------------------------------
hipError_t pk_launch_pack(hipStream_t st, const pk_row* rows, uint32_t n, uint32_t n_obj, const uint4* arena,
                          uint64_t arena_bytes, uint4* pool, uint64_t pool_blocks, bv_obj* objs) {
  if (n == 0) return hipSuccess;
  if (n_obj > n || !rows || !arena || !pool || (n_obj && !objs)) return hipErrorInvalidValue;
  const uint32_t per = 64 / PK_PACK_LANES;
  hipLaunchKernelGGL(pk_pack_kernel, dim3((n + per - 1) / per), dim3(64), 0, st, rows, n, n_obj, arena, arena_bytes, pool,
                     pool_blocks, objs);
  return hipGetLastError();
}

hipError_t pk_launch_object(hipStream_t st, const pk_row* rows, const bv_obj* objs, uint32_t n_obj, const uint4* pool,
                            uint64_t pool_blocks, uint64_t* pow_out, uint4* inv_out, uint32_t* sum_out) {
  if (n_obj == 0) return hipSuccess;
  if (!rows || !objs || !pool || !pow_out || !inv_out || !sum_out) return hipErrorInvalidValue;
  hipLaunchKernelGGL(pk_object_kernel, dim3((n_obj + BV_BLOCK - 1) / BV_BLOCK), dim3(BV_BLOCK), 0, st, rows, objs, n_obj,
                     pool, pool_blocks, pow_out, inv_out, sum_out);
  return hipGetLastError();
}

hipError_t pk_launch_object_binned(hipStream_t st, const pk_row* rows, const bv_obj* objs, uint32_t n_obj,
                                   const uint4* pool, uint64_t pool_blocks, uint64_t* pow_out, uint4* inv_out,
                                   uint32_t* sum_out, const uint32_t* bins, uint32_t nbins) {
  if (n_obj == 0) return hipSuccess;
  if (nbins == 0 || nbins % 4 || !bins || !rows || !objs || !pool || !pow_out || !inv_out || !sum_out)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(pk_object_binned_kernel, dim3(nbins / 4), dim3(BV_BINNED_WG), 0, st, rows, objs, n_obj, pool,
                     pool_blocks, pow_out, inv_out, sum_out, bins, nbins);
  return hipGetLastError();
}

hipError_t pk_launch_sum(hipStream_t st, const pk_row* rows, uint32_t n_sum, const uint4* pool, uint64_t pool_blocks,
                         uint32_t* sum_out) {
  if (n_sum == 0) return hipSuccess;
  if (!rows || !pool || !sum_out) return hipErrorInvalidValue;
  hipLaunchKernelGGL(pk_sum_kernel, dim3((n_sum + BV_BLOCK - 1) / BV_BLOCK), dim3(BV_BLOCK), 0, st, rows, n_sum, pool,
                     pool_blocks, sum_out);
  return hipGetLastError();
}
