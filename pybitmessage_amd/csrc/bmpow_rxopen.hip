// bmpow_rxopen.hip -- the AES pass of received msgs whose MAC verified, from the MAC pool to the plaintext
// pool without leaving the device (gfx950).
//
// Reference: the cipher of ECC.decrypt (src/pyelliptic/ecc.py:499-501) behind the MAC check (:494-498), for
// the key that processmsg's loop found (src/class_objectProcessor.py:459-477).  Host side:
// bmpow_host_rxopen.hip (bmpow_rx_sealed_msgs).
//
// One lane per matched row, 64 rows per wave, in the order of the ECIES set (MAC block count descending, so a
// wave's lanes iterate alike).  The ciphertext is read where ec_mac_kernel hashed it, the key where
// ec_gather_kernel left it: neither crossed the bus.  Each block copies the AES tables into LDS first
// (aes256_dev.h); the per-row work is bmpow_rxopen_rows.h.  Every loop bound comes from a host-validated
// length, checked once more against the buffers' sizes here; a lane writes its own slot, its own row's plen and
// its own opened[] only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bmpow_rxopen_kernels.h"
#include "bmpow_rxopen_rows.h"

// One lane's row: Row is rx_row (msgs) or rxo_row (broadcasts and pubkeys); both carry poff and plen.
template <class Row>
BM_DEV void rxs_open_lane(const aes::DecTab& tab, const rxs_row* __restrict__ orows, const uint64_t* __restrict__ key_e,
                          uint32_t n_src, const uint8_t* pool, uint64_t pool_bytes, Row* rows, uint8_t* plain,
                          uint64_t plain_bytes, uint32_t o, int32_t* __restrict__ opened) {
  const rxs_row r = orows[o];
  const uint64_t poff = rows[o].poff, at = 64ull * r.blk;
  // the padded pool row ends behind the ciphertext (bmpow_rxopen_rows.h); the slot holds clen bytes
  const bool fits = r.src < n_src && r.clen >= 16 && r.clen % 16 == 0 && r.body_off >= 16 && at + r.body_off + r.clen + 9 <= pool_bytes &&
                    poff % 16 == 0 && poff + r.clen <= plain_bytes;
  if (!fits) {
    rows[o].plen = 0;
    opened[o] = -1;
    return;
  }
  uint32_t key[8], ivw[4];
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const uint64_t e = key_e[4 * (size_t)r.src + w];
    key[2 * w] = (uint32_t)(e >> 32), key[2 * w + 1] = (uint32_t)e;
  }
  const uint4 iv = *reinterpret_cast<const uint4*>(pool + at);
  ivw[0] = __builtin_bswap32(iv.x), ivw[1] = __builtin_bswap32(iv.y), ivw[2] = __builtin_bswap32(iv.z),
  ivw[3] = __builtin_bswap32(iv.w);
  const int32_t got = rxs::open_row(pool + at + r.body_off, r.clen, key, ivw, plain + poff, tab);
  rows[o].plen = got < 0 ? 0u : (uint32_t)got;
  opened[o] = got;
}

__global__ __launch_bounds__(RXS_BLOCK) void rxs_open_kernel(const rxs_row* __restrict__ orows,
                                                             const uint64_t* __restrict__ key_e, uint32_t n_src,
                                                             const uint8_t* pool, uint64_t pool_bytes, rx_row* rows, uint8_t* plain,
                                                             uint64_t plain_bytes, uint32_t n, int32_t* __restrict__ opened) {
  __shared__ aes::DecTab tab;
  aes::fill_dec(tab, threadIdx.x, RXS_BLOCK);
  __syncthreads();
  const uint32_t o = blockIdx.x * RXS_BLOCK + threadIdx.x;
  if (o >= n) return;
  rxs_open_lane(tab, orows, key_e, n_src, pool, pool_bytes, rows, plain, plain_bytes, o, opened);
}

// The same over the rows of the object family (bmpow_host_rxobjopen.hip).
__global__ __launch_bounds__(RXS_BLOCK) void rxo_open_kernel(const rxs_row* __restrict__ orows,
                                                             const uint64_t* __restrict__ key_e, uint32_t n_src,
                                                             const uint8_t* pool, uint64_t pool_bytes, rxo_row* rows, uint8_t* plain,
                                                             uint64_t plain_bytes, uint32_t n, int32_t* __restrict__ opened) {
  __shared__ aes::DecTab tab;
  aes::fill_dec(tab, threadIdx.x, RXS_BLOCK);
  __syncthreads();
  const uint32_t o = blockIdx.x * RXS_BLOCK + threadIdx.x;
  if (o >= n) return;
  rxs_open_lane(tab, orows, key_e, n_src, pool, pool_bytes, rows, plain, plain_bytes, o, opened);
}

// ---------------------------------------------------------------------------------------
// Launch wrappers (C++ linkage).
// ---------------------------------------------------------------------------------------
hipError_t rxs_launch_open(hipStream_t st, const rxs_row* orows, const uint64_t* key_e, uint32_t n_src,
                           const uint8_t* pool, uint64_t pool_bytes, rx_row* rows, uint8_t* plain, uint64_t plain_bytes, uint32_t n,
                           int32_t* opened) {
  if (n == 0) return hipSuccess;
  if (!orows || !key_e || !pool || !rows || !plain || !opened) return hipErrorInvalidValue;
  hipLaunchKernelGGL(rxs_open_kernel, dim3((n + RXS_BLOCK - 1) / RXS_BLOCK), dim3(RXS_BLOCK), 0, st, orows, key_e, n_src,
                     pool, pool_bytes, rows, plain, plain_bytes, n, opened);
  return hipGetLastError();
}

hipError_t rxo_launch_open(hipStream_t st, const rxs_row* orows, const uint64_t* key_e, uint32_t n_src,
                           const uint8_t* pool, uint64_t pool_bytes, rxo_row* rows, uint8_t* plain, uint64_t plain_bytes, uint32_t n,
                           int32_t* opened) {
  if (n == 0) return hipSuccess;
  if (!orows || !key_e || !pool || !rows || !plain || !opened) return hipErrorInvalidValue;
  hipLaunchKernelGGL(rxo_open_kernel, dim3((n + RXS_BLOCK - 1) / RXS_BLOCK), dim3(RXS_BLOCK), 0, st, orows, key_e, n_src,
                     pool, pool_bytes, rows, plain, plain_bytes, n, opened);
  return hipGetLastError();
}
