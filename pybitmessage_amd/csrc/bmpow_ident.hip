// bmpow_ident.hip -- sender identification on gfx950: per row the ripe of two public keys, the keys and
// the tag derived from it, and its BM- address (include/bmpow_ident.h).
//
// Reference: the ripe, src/class_objectProcessor.py:877-879 and src/protocol.py:493-495; the tag and the
// keys, :889-892 and src/shared.py:169-184; the address, src/addresses.py:146-180.
//
// One lane per row, rows independent, no LDS.  A row is two SHA-512 blocks over the 130 key bytes, two
// RIPEMD-160 blocks over that digest, and then four one-block SHA-512 hashes: data_full, its digest,
// the checksum's data (the ripe with its leading zero bytes dropped) and its digest.  Each of the three
// groups loops over its blocks with `#pragma unroll 1`, so the kernel holds two SHA-512 compression
// bodies and one RIPEMD-160 body however many blocks it hashes.  The byte-oriented rest -- varints, the
// zero-byte rule, base58 -- is bmpow_ident_fmt.h, shared with the host test; it indexes nothing at run
// time, so a row needs no scratch memory.  The record's 45 words leave as ordinary stores in plain C++, which
// the compiler groups into eleven 16-byte stores and one 4-byte store per row.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bmpow_ident_fmt.h"
#include "bmpow_ident_kernels.h"
#include "ripemd160_dev.h"
#include "sha512_dev.h"

using namespace bm;

namespace {

// SHA-512 over 0x04||Xs||Ys||0x04||Xe||Ye (130 bytes, two blocks), then RIPEMD-160: what the address
// search's ripe_of computes, here from the keys' bytes in memory (eight aligned 16-byte loads).
BM_DEV void id_ripe_of_keys(uint32_t (&rh)[5], const uint4* __restrict__ key) {
  uint64_t k[16];  // Xs, Ys, Xe, Ye as big-endian words
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const uint4 v = key[j];
    k[2 * j] = be64(v.x, v.y);
    k[2 * j + 1] = be64(v.z, v.w);
  }
  uint64_t w[16];
  w[0] = (0x04ULL << 56) | (k[0] >> 8);
#pragma unroll
  for (int i = 1; i < 8; ++i) w[i] = (k[i - 1] << 56) | (k[i] >> 8);
  w[8] = (k[7] << 56) | (0x04ULL << 48) | (k[8] >> 16);
#pragma unroll
  for (int i = 9; i < 16; ++i) w[i] = (k[i - 1] << 48) | (k[i] >> 16);
  const uint64_t tail0 = (k[15] << 48) | (0x80ULL << 40);
  uint64_t h[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) h[i] = IV(i);
#pragma unroll 1
  for (int b = 0; b < 2; ++b) {  // one compress body for both blocks
    compress(h, w);
    w[0] = tail0;
#pragma unroll
    for (int i = 1; i < 15; ++i) w[i] = 0;
    w[15] = 130 * 8;
  }
  rmd::of_sha512_digest(rh, h);
}

// four digest words as 32 bytes in memory order
BM_DEV void id_store_be(uint32_t* __restrict__ p, const uint64_t* h) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    p[2 * i] = __builtin_bswap32(hi32(h[i]));
    p[2 * i + 1] = __builtin_bswap32(lo32(h[i]));
  }
}

// Everything from the ripe on, for both kernels: the record's five fields into rec (45 words).
BM_DEV void id_finish(const uint32_t (&rh)[5], uint64_t version, uint64_t stream, uint32_t* __restrict__ rec) {
#pragma unroll
  for (int i = 0; i < 5; ++i) rec[i] = rh[i];  // RIPEMD-160's words are the ripe's bytes in memory order
  idf::msg full, data;
  idf::put_address_data(full, version, stream, rh, 0);
  idf::put_address_data(data, version, stream, rh, idf::strip_count(version, rh));
  uint64_t h[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) h[i] = 0;
#pragma unroll 1
  for (int b = 0; b < 4; ++b) {  // data_full, its digest, the checksum's data, its digest: one compress body
    uint64_t w[16];
    if (b & 1) {
#pragma unroll
      for (int i = 0; i < 8; ++i) w[i] = h[i];
      w[8] = PAD;
#pragma unroll
      for (int i = 9; i < 15; ++i) w[i] = 0;
      w[15] = 64 * 8;
    } else {
      idf::msg m;
#pragma unroll
      for (int i = 0; i < idf::kMsgWords; ++i) m.w[i] = b == 0 ? full.w[i] : data.w[i];
      m.len = b == 0 ? full.len : data.len;
      idf::sha512_block(m, w);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) h[i] = IV(i);
    compress(h, w);
    if (b < 2) id_store_be(rec + 5 + 8 * b, h);  // key_v3 = d1[:32], tag_key = d2[:32]
    if (b == 1) id_store_be(rec + 21, h + 4);    // tag = d2[32:]
  }
  idf::put_be32(data, hi32(h[0]));  // the checksum: the first four bytes of the second digest
  uint32_t s[idf::kMaxChars / 4], field[16];
  const uint32_t nchars = idf::base58(data, s);
  idf::address_field(nchars, s, field);
#pragma unroll
  for (int i = 0; i < 16; ++i) rec[29 + i] = field[i];
}

}  // namespace

__global__ __launch_bounds__(ID_BLOCK) void id_derive_kernel(const uint4* __restrict__ keys,
                                                             const uint64_t* __restrict__ versions,
                                                             const uint64_t* __restrict__ streams, uint32_t n,
                                                             uint32_t* __restrict__ out) {
  const uint32_t k = blockIdx.x * ID_BLOCK + threadIdx.x;
  if (k >= n) return;
  uint32_t rh[5];
  id_ripe_of_keys(rh, keys + 8 * (uint64_t)k);
  id_finish(rh, versions[k], streams[k], out + ID_REC_WORDS * (uint64_t)k);
}

__global__ __launch_bounds__(ID_BLOCK) void id_from_ripe_kernel(const uint32_t* __restrict__ ripes,
                                                                const uint64_t* __restrict__ versions,
                                                                const uint64_t* __restrict__ streams, uint32_t n,
                                                                uint32_t* __restrict__ out) {
  const uint32_t k = blockIdx.x * ID_BLOCK + threadIdx.x;
  if (k >= n) return;
  uint32_t rh[5];
#pragma unroll
  for (int i = 0; i < 5; ++i) rh[i] = ripes[5 * (uint64_t)k + i];
  id_finish(rh, versions[k], streams[k], out + ID_REC_WORDS * (uint64_t)k);
}

// ---------------------------------------------------------------------------------------
// Launch wrappers (C++ linkage, used by bmpow_host_ident.hip).
// ---------------------------------------------------------------------------------------
hipError_t id_launch_derive(hipStream_t st, const uint4* keys, const uint64_t* versions, const uint64_t* streams,
                            uint32_t n, bmpow_ident_rec* out) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(id_derive_kernel, dim3((n + ID_BLOCK - 1) / ID_BLOCK), dim3(ID_BLOCK), 0, st, keys, versions,
                     streams, n, reinterpret_cast<uint32_t*>(out));
  return hipGetLastError();
}

hipError_t id_launch_from_ripe(hipStream_t st, const uint32_t* ripes, const uint64_t* versions, const uint64_t* streams,
                               uint32_t n, bmpow_ident_rec* out) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(id_from_ripe_kernel, dim3((n + ID_BLOCK - 1) / ID_BLOCK), dim3(ID_BLOCK), 0, st, ripes, versions,
                     streams, n, reinterpret_cast<uint32_t*>(out));
  return hipGetLastError();
}
