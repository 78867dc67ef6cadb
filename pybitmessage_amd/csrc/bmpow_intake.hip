// bmpow_intake.hip -- object-intake kernels (gfx950): per received object the receive-side POW value and
// the inventory hash, from one upload of the payload pool.
//
// Reference: src/network/bmproto.py:377-441 (bm_command_object) builds a BMObject per object, whose
// constructor hashes the whole object (src/network/bmobject.py:66, src/addresses.py:137-143:
// inventoryHash = SHA512(SHA512(object))[:32]) before protocol.isProofOfWorkSufficient hashes it again
// from byte 8 on (src/protocol.py:280-282).  Host side: bmpow_host_intake.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bmpow_intake_dev.h"  // intake_of: both chains of one object
#include "bmpow_intake_kernels.h"
#include "sha512_dev.h"

using namespace bm;

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
