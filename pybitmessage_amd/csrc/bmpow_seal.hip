// bmpow_seal.hip -- the AES-256-CBC and HMAC-SHA256 pass of outgoing ECIES blobs, and raw AES-256-CBC
// (gfx950).
//
// Reference: everything of ECC.raw_encrypt after the key derivation (src/pyelliptic/ecc.py:472-482):
//     ciphertext = AES-256-CBC(key_e, iv, PKCS#7(plain));  blob = iv | pubkey | ciphertext
//     mac = HMAC-SHA256(key_m, blob);                      return blob | mac
// and the cipher of ECC.decrypt (:499-501) the other way.  Host side: bmpow_host_send.hip (the seal),
// bmpow_host_ecies.hip (the raw call).
//
// One lane per row, 64 rows per wave; the host sorts the rows of a set by block count, descending, so a
// wave's lanes iterate alike (as the MAC pool of bmpow_host_ecies.hip), and gives every row a slot of its
// own in the set's pool.  The seal kernel reads the derived keys and the ephemeral point where
// sd_shared_kernel and sd_comb_kernel left them: neither reaches the host.  Each block copies the AES
// tables into LDS first (aes256_dev.h); the per-row work is bmpow_seal_rows.h.  Every loop bound comes
// from a host-validated length and a lane touches its own slot only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "bmpow_seal_kernels.h"
#include "bmpow_seal_rows.h"

BM_DEV void be_words(uint32_t (&w)[4], const uint4 v) {
  w[0] = __builtin_bswap32(v.x), w[1] = __builtin_bswap32(v.y), w[2] = __builtin_bswap32(v.z), w[3] = __builtin_bswap32(v.w);
}

__global__ __launch_bounds__(SL_BLOCK) void sl_seal_kernel(const uint64_t* __restrict__ kout, const ec::ge* __restrict__ pt,
                                                           const uint32_t* __restrict__ ok, const uint4* __restrict__ iv,
                                                           const sl_row* __restrict__ rows, uint8_t* pool, uint32_t n,
                                                           uint32_t stride, uint32_t* __restrict__ out_len) {
  __shared__ aes::EncTab tab;
  aes::fill_enc(tab, threadIdx.x, SL_BLOCK);
  __syncthreads();
  const uint32_t o = blockIdx.x * SL_BLOCK + threadIdx.x;
  if (o >= n) return;
  if (ok && !ok[o]) {
    out_len[o] = 0;
    return;
  }
  uint32_t ke[8], km[8], X[8], Y[8], ivw[4];
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const uint64_t e = kout[(size_t)w * stride + o], m = kout[(size_t)(4 + w) * stride + o];
    ke[2 * w] = (uint32_t)(e >> 32), ke[2 * w + 1] = (uint32_t)e;
    km[2 * w] = (uint32_t)(m >> 32), km[2 * w + 1] = (uint32_t)m;
  }
  const ec::ge R = pt[o];
#pragma unroll
  for (int i = 0; i < 8; ++i) X[i] = R.x.d[7 - i], Y[i] = R.y.d[7 - i];
  be_words(ivw, iv[o]);
  const sl_row r = rows[o];
  out_len[o] = sl::seal_row(pool + (size_t)r.off16 * 16, r.len, ke, km, ivw, X, Y, tab.te0);
}

template <bool kDecrypt>
__global__ __launch_bounds__(SL_BLOCK) void sl_cbc_kernel(const uint4* __restrict__ keys, const uint4* __restrict__ iv,
                                                          const sl_row* __restrict__ rows, uint8_t* pool, uint32_t n,
                                                          int32_t* __restrict__ out_len) {
  __shared__ typename std::conditional<kDecrypt, aes::DecTab, aes::EncTab>::type tab;
  if constexpr (kDecrypt) aes::fill_dec(tab, threadIdx.x, SL_BLOCK);
  else aes::fill_enc(tab, threadIdx.x, SL_BLOCK);
  __syncthreads();
  const uint32_t o = blockIdx.x * SL_BLOCK + threadIdx.x;
  if (o >= n) return;
  uint32_t key[8], ivw[4], lo[4], hi[4];
  be_words(lo, keys[2 * (size_t)o]);
  be_words(hi, keys[2 * (size_t)o + 1]);
#pragma unroll
  for (int i = 0; i < 4; ++i) key[i] = lo[i], key[4 + i] = hi[i];
  be_words(ivw, iv[o]);
  const sl_row r = rows[o];
  uint8_t* slot = pool + (size_t)r.off16 * 16;
  if constexpr (kDecrypt) out_len[o] = sl::cbc_decrypt_row(slot, r.len, key, ivw, tab);
  else out_len[o] = (int32_t)sl::cbc_encrypt_row(slot, r.len, key, ivw, tab.te0);
}

// ---------------------------------------------------------------------------------------
// Launch wrappers (C++ linkage).  stride is a multiple of SL_BLOCK.
// ---------------------------------------------------------------------------------------
static bool sl_shape_ok(uint32_t n, uint32_t stride) { return n <= stride && stride % SL_BLOCK == 0; }

hipError_t sl_launch_seal(hipStream_t st, const uint64_t* kout, const ec::ge* pt, const uint32_t* ok, const uint4* iv,
                          const sl_row* rows, uint8_t* pool, uint32_t n, uint32_t stride, uint32_t* out_len) {
  if (n == 0) return hipSuccess;
  if (!sl_shape_ok(n, stride) || !kout || !pt || !iv || !rows || !pool || !out_len) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sl_seal_kernel, dim3(stride / SL_BLOCK), dim3(SL_BLOCK), 0, st, kout, pt, ok, iv, rows, pool, n, stride,
                     out_len);
  return hipGetLastError();
}

hipError_t sl_launch_cbc(hipStream_t st, int decrypt, const uint4* keys, const uint4* iv, const sl_row* rows, uint8_t* pool,
                         uint32_t n, uint32_t stride, int32_t* out_len) {
  if (n == 0) return hipSuccess;
  if (!sl_shape_ok(n, stride) || !keys || !iv || !rows || !pool || !out_len) return hipErrorInvalidValue;
  if (decrypt)
    hipLaunchKernelGGL(sl_cbc_kernel<true>, dim3(stride / SL_BLOCK), dim3(SL_BLOCK), 0, st, keys, iv, rows, pool, n, out_len);
  else
    hipLaunchKernelGGL(sl_cbc_kernel<false>, dim3(stride / SL_BLOCK), dim3(SL_BLOCK), 0, st, keys, iv, rows, pool, n, out_len);
  return hipGetLastError();
}
