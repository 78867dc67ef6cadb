// bmpow_intake.hip -- object-intake kernels (gfx950): per received object the receive-side POW value and
// the inventory hash, from one upload of the payload pool.
//
// Reference: src/network/bmproto.py:377-441 (bm_command_object) builds a BMObject per object, whose
// constructor hashes the whole object (src/network/bmobject.py:66, src/addresses.py:137-143:
// inventoryHash = SHA512(SHA512(object))[:32]) before protocol.isProofOfWorkSufficient hashes it again
// from byte 8 on (src/protocol.py:280-282).  Host side: bmpow_host_intake.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bmpow_intake_kernels.h"
#include "sha512_dev.h"

using namespace bm;

// ---------------------------------------------------------------------------------------
// One lane per object, over the verification's pool: object[8:] SHA-512-padded to nblk blocks.  The
// lane runs bv_pow_kernel's chain (nblk payload blocks, then the trial's two), and then the inventory
// chain over the same pool words: the full object is the payload stream shifted by one 64-bit word with
// the nonce in front, so with L the object's length and nblk2 = ceil((L + 17) / 128) (nblk or nblk + 1)
// word k of its padded message is
//     the nonce            k == 0
//     8 L                  k == 16 nblk2 - 1
//     0                    k >= 16 nblk        (the pool's own length word must not shift in)
//     P[k - 1]             otherwise
// (the 0x80 byte shifts with the payload; checked on the CPU against direct padding for every L in
// tests/test_intake.py).  The digest's own one-block hash follows.  One copy of the compression body
// serves all nblk + 2 + nblk2 + 1 blocks, as in pow_of: the message words come from selects, and the
// state restarts at the IV wherever a chain begins.
//
// The inventory chain reads each pool block once more, with the same aligned 16-B loads (L2 hits for
// all but the longest objects), and carries the block's last word into the next block's word 0: no
// unaligned access, 2 VGPRs.  BI_SHIFTED_LOADS (A/B) reads words k - 1 .. k + 14 with sixteen 8-B
// loads instead.
// ---------------------------------------------------------------------------------------
BM_DEV void intake_of(const bv_obj& o, uint32_t L, const uint4* __restrict__ pool, uint64_t& pow,
                      uint64_t (&inv)[4]) {
  uint64_t h[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) h[i] = IV(i);
  const uint4* base = pool + (uint64_t)o.blk * 8;
  const uint32_t nb = o.nblk;
  const uint32_t nb2 = (uint32_t)(((uint64_t)L + 17 + 127) >> 7);
  const uint32_t i0 = nb + 2;              // first block of the inventory chain
  const uint32_t total = i0 + nb2 + 1;     // ... and the digest's block after it
  const uint64_t nonce = o.nonce;
#ifndef BI_SHIFTED_LOADS
  uint64_t carry = 0;  // the previous block's last pool word
#endif
  pow = 0;
  for (uint32_t b = 0; b < total; ++b) {
    const bool pay = b < nb, t1 = b == nb;
    const uint32_t c = b - i0;             // block of the inventory chain (when ich)
    const bool ich = b >= i0 && c < nb2;
    const uint32_t lb = pay ? b : (ich && c < nb ? c : nb - 1);  // never past the object's blocks
    uint64_t w[16];
#ifdef BI_SHIFTED_LOADS
    if (ich) {
      const uint2* q = (const uint2*)base;
      const uint32_t k0 = 16 * lb;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const uint2 v = q[k0 + i > 0 ? k0 + i - 1 : 0];
        w[i] = be64(v.x, v.y);
      }
    } else
#endif
    {
      const uint4* p = base + (uint64_t)lb * 8;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const uint4 v = p[j];
        w[2 * j] = be64(v.x, v.y);
        w[2 * j + 1] = be64(v.z, v.w);
      }
    }
    if (!pay) {
      // a chain begins: trial block 1 and 2, the inventory chain's first block, the digest's block
      const bool restart = !ich || c == 0;
      uint64_t d[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) d[i] = h[i], h[i] = restart ? IV(i) : h[i];
      if (b == i0) pow = d[0];             // the trial's second digest
      if (ich) {
        const bool zero = c >= nb, last = c == nb2 - 1;
#ifdef BI_SHIFTED_LOADS
        if (c == 0) w[0] = nonce;
#else
        const uint64_t w15 = w[15];
#pragma unroll
        for (int i = 15; i > 0; --i) w[i] = w[i - 1];
        w[0] = c == 0 ? nonce : carry;
        carry = w15;
#endif
#pragma unroll
        for (int i = 0; i < 16; ++i) w[i] = zero ? 0 : w[i];
        if (last) w[15] = (uint64_t)L << 3;
      } else {
        // trial block 1: nonce || payload digest || padding (72 B); else a digest || padding (64 B)
        w[0] = t1 ? nonce : d[0];
#pragma unroll
        for (int i = 1; i < 8; ++i) w[i] = t1 ? d[i - 1] : d[i];
        w[8] = t1 ? d[7] : PAD;
        w[9] = t1 ? PAD : 0;
#pragma unroll
        for (int i = 10; i < 15; ++i) w[i] = 0;
        w[15] = t1 ? 72 * 8 : 64 * 8;
      }
    }
    compress(h, w);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) inv[i] = h[i];
}

BM_DEV void intake_store(uint32_t k, const bv_obj* __restrict__ objs, const uint32_t* __restrict__ lens,
                         const uint4* __restrict__ pool, uint64_t* __restrict__ pow_out,
                         uint4* __restrict__ inv_out) {
  uint64_t pow, inv[4];
  intake_of(objs[k], lens[k], pool, pow, inv);
  pow_out[k] = pow;
  // the digest's first 32 bytes, big-endian words as bytes
  inv_out[2 * (uint64_t)k] = make_uint4(__builtin_bswap32(hi32(inv[0])), __builtin_bswap32(lo32(inv[0])),
                                        __builtin_bswap32(hi32(inv[1])), __builtin_bswap32(lo32(inv[1])));
  inv_out[2 * (uint64_t)k + 1] = make_uint4(__builtin_bswap32(hi32(inv[2])), __builtin_bswap32(lo32(inv[2])),
                                            __builtin_bswap32(hi32(inv[3])), __builtin_bswap32(lo32(inv[3])));
}

// One wave per object group of BV_BLOCK lanes, the groups dispatched in sorted order (small floods).
__global__ __launch_bounds__(BV_BLOCK) void bi_intake_kernel(const bv_obj* __restrict__ objs,
                                                             const uint32_t* __restrict__ lens, uint32_t n,
                                                             const uint4* __restrict__ pool,
                                                             uint64_t* __restrict__ pow_out,
                                                             uint4* __restrict__ inv_out) {
  const uint32_t k = blockIdx.x * BV_BLOCK + threadIdx.x;
  if (k >= n) return;
  intake_store(k, objs, lens, pool, pow_out, inv_out);
}

// Balanced floods: bv_pow_binned_kernel's shape (bmpow_verify.hip), over the same bins -- one
// 1024-thread workgroup per CU (its LDS request admits no second one), each wave taking groups from
// the bin of the SIMD it runs on, then from the CU's other bins, with the issue priority raised for a
// bin's first (longest) group.  plan_bins weighs a group by nblk + 2; here it costs nblk + nblk2 + 3,
// the same order and nearly the same ratios, so the bins stay balanced.
constexpr uint32_t kBiBinnedLdsWords = (96u << 10) / 4;  // > half of the CU's 160 KiB

__global__ __launch_bounds__(BV_BINNED_WG) void bi_intake_binned_kernel(
    const bv_obj* __restrict__ objs, const uint32_t* __restrict__ lens, uint32_t n, const uint4* __restrict__ pool,
    uint64_t* __restrict__ pow_out, uint4* __restrict__ inv_out, const uint32_t* __restrict__ bins, uint32_t nbins) {
  __shared__ uint32_t heads[kBiBinnedLdsWords];  // [0..3]: next group of each of the CU's 4 bins
  if (threadIdx.x < 4) heads[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63;
  // s_getreg_b32 hwreg(HW_REG_HW_ID, 4, 2): SIMD_ID of this wave
  const uint32_t simd = __builtin_amdgcn_s_getreg((1u << 11) | (4u << 6) | 4u) & 3u;
  const uint32_t* list = bins + nbins + 1;
  for (uint32_t t = 0; t < 4; ++t) {
    const uint32_t s = (simd + t) & 3u;
    const uint32_t b = blockIdx.x * 4 + s;
    const uint32_t lo = bins[b], cnt = bins[b + 1] - lo;
    for (;;) {
      uint32_t idx = 0;
      if (lane == 0) idx = atomicAdd(&heads[s], 1u);
      idx = __builtin_amdgcn_readfirstlane(idx);
      if (idx >= cnt) break;
      const uint32_t k = list[lo + idx] * BV_BLOCK + lane;
      if (idx == 0) __builtin_amdgcn_s_setprio(3);
      if (k < n) intake_store(k, objs, lens, pool, pow_out, inv_out);
      if (idx == 0) __builtin_amdgcn_s_setprio(0);
    }
  }
}

// ---------------------------------------------------------------------------------------
// Launch wrappers (C++ linkage, used by bmpow_host_intake.hip).
// ---------------------------------------------------------------------------------------
hipError_t bi_launch(hipStream_t st, const bv_obj* objs, const uint32_t* lens, uint32_t n, const uint4* pool,
                     uint64_t* pow_out, uint4* inv_out) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(bi_intake_kernel, dim3((n + BV_BLOCK - 1) / BV_BLOCK), dim3(BV_BLOCK), 0, st, objs, lens, n,
                     pool, pow_out, inv_out);
  return hipGetLastError();
}

hipError_t bi_launch_binned(hipStream_t st, const bv_obj* objs, const uint32_t* lens, uint32_t n, const uint4* pool,
                            uint64_t* pow_out, uint4* inv_out, const uint32_t* bins, uint32_t nbins) {
  if (n == 0) return hipSuccess;
  if (nbins == 0 || nbins % 4) return hipErrorInvalidValue;
  hipLaunchKernelGGL(bi_intake_binned_kernel, dim3(nbins / 4), dim3(BV_BINNED_WG), 0, st, objs, lens, n, pool,
                     pow_out, inv_out, bins, nbins);
  return hipGetLastError();
}
