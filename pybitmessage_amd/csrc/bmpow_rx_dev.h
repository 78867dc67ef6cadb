// bmpow_rx_dev.h -- the device code the two families of signed rows share: msgs (bmpow_rx.hip) and broadcasts
// and pubkeys (bmpow_rxobj.hip).  Their kernels differ in the walk and in how they write the record; the steps
// between are the same and are here once, as inlined helpers: what goes to the curve kernels for a row (its own
// signature and key, or the dummy), the identification's key bytes, one row's share of the pack kernel, and
// sigHash.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bmpow_rx_fmt.h"
#include "bmpow_sig_kernels.h"
#include "sha512_dev.h"

namespace rxd {

// secp256k1's generator, little-endian limbs
static __device__ const uint32_t kGx[8] = {0x16F81798u, 0x59F2815Bu, 0x2DCE28D9u, 0x029BFCDBu,
                                    0xCE870B07u, 0x55A06295u, 0xF9DCBBACu, 0x79BE667Eu};
static __device__ const uint32_t kGy[8] = {0xFB10D4B8u, 0x9C47D08Fu, 0xA6855419u, 0xFD17B448u,
                                    0x0E1108A8u, 0x5DA4FBFCu, 0x26A3C465u, 0x483ADA77u};

struct PoolSrc {  // a row's plaintext (or object) in the plaintext pool, for rxf::pack_chunk_n
  const uint4* chunks;  // its slot in the pool
  uint32_t nchunks;     // of the slot, clipped to the pool
  const uint8_t* bytes;
  uint32_t len;
  __device__ __forceinline__ void load16(uint32_t k, uint32_t (&w)[4]) const {
    uint4 v = make_uint4(0, 0, 0, 0);
    if (k < nchunks) v = chunks[k];
    w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
  }
  __device__ __forceinline__ uint32_t byte(uint32_t i) const { return i < len ? bytes[i] : 0u; }
};

// sig and pt of one row: r, s and the key as they parsed (real), with nblk blocks to hash from blk on; else a
// fixed valid dummy -- the generator, r = s = 1, no blocks to hash -- so that the sets keep their shape, no
// compaction pass runs, and sg_scalar_kernel's 1 <= r, s < n holds for every lane.  The dummy's verdict is
// never read.
__device__ __forceinline__ void emit_sig(bool real, const uint32_t (&r)[8], const uint32_t (&s)[8], const uint32_t (&x)[8],
                                         const uint32_t (&y)[8], uint32_t blk, uint32_t nblk, sg_sig& sig_out,
                                         ec::ge& pt_out) {
  sg_sig sig;
  ec::ge pt;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    sig.r.d[i] = real ? r[i] : (i == 0 ? 1u : 0u);
    sig.s.d[i] = real ? s[i] : (i == 0 ? 1u : 0u);
    pt.x.d[i] = real ? x[i] : kGx[i];
    pt.y.d[i] = real ? y[i] : kGy[i];
  }
  sig.blk = blk;
  sig.nblk = real ? nblk : 0u;
  sig_out = sig;
  pt_out = pt;
}

// The identification's input: the two keys' 128 bytes as they lie at p[key_off ..) (have: all inside the row's
// bytes), zeros otherwise, as eight 16-byte chunks.
__device__ __forceinline__ void gather_keys(bool have, const uint8_t* p, uint32_t key_off, uint4* keys) {
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    uint32_t w[4] = {0, 0, 0, 0};
    if (have) {
#pragma unroll
      for (int j = 0; j < 16; ++j) w[j >> 2] |= (uint32_t)p[key_off + 16 * q + j] << (8 * (j & 3));
    }
    keys[q] = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

// One lane's share of a row in the pack kernels: chunks sub, sub + lanes, ... of the row's nblk blocks at
// pool[4 blk ..), each pre[0 .. pre_len) || source[skip .. skip + bottom) || padding.  The source lies at byte
// poff of plain, plen bytes long; nothing is read past plain_chunks or written past pool_chunks.
template <int NW>
__device__ __forceinline__ void pack_row(uint32_t sub, uint32_t lanes, uint64_t poff, uint32_t plen,
                                         const uint4* __restrict__ plain, uint64_t plain_chunks, uint32_t blk, uint32_t nblk,
                                         const uint32_t (&pre)[NW], uint32_t pre_len, uint32_t bottom, uint32_t skip,
                                         uint4* __restrict__ pool, uint64_t pool_chunks) {
  const uint64_t base = 4ull * blk;
  const uint64_t first = poff >> 4;
  PoolSrc src;
  src.len = plen;
  src.chunks = plain + first;
  const uint64_t want = ((uint64_t)src.len + 15) >> 4, room = first < plain_chunks ? plain_chunks - first : 0;
  src.nchunks = (uint32_t)(want < room ? want : room);
  src.bytes = reinterpret_cast<const uint8_t*>(plain) + poff;
  if ((uint64_t)src.nchunks * 16 < src.len) src.len = src.nchunks * 16;  // never past the pool
#pragma unroll 1
  for (uint32_t c = sub; c < 4 * nblk; c += lanes) {
    uint32_t w[4];
    rxf::pack_chunk_n<NW>(c, nblk, pre, pre_len, bottom, skip, src, w);
    if (base + c < pool_chunks) pool[base + c] = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

// sigHash = SHA512(SHA512(signature))[32:] of the have <= rxf::kMaxDer bytes at sp (one block each): out = the
// second digest's words 4 .. 7.  The caller clips have, and sp + have to the row's bytes.
__device__ __forceinline__ void sig_hash(const uint8_t* sp, uint32_t have, uint64_t (&out)[4]) {
  using namespace bm;
  uint64_t w[16], h[8];
#pragma unroll
  for (int i = 0; i < 16; ++i) w[i] = 0;
#pragma unroll
  for (int i = 0; i <= (int)rxf::kMaxDer; ++i) {
    const uint32_t b = (uint32_t)i < have ? sp[(uint32_t)i < have ? i : 0] : (uint32_t)i == have ? 0x80u : 0u;
    w[i >> 3] |= (uint64_t)b << (56 - 8 * (i & 7));
  }
  w[15] = 8ull * have;
#pragma unroll 1
  for (int pass = 0; pass < 2; ++pass) {  // one compress body for both hashes
    if (pass) {
#pragma unroll
      for (int i = 0; i < 8; ++i) w[i] = h[i];
      w[8] = PAD;
#pragma unroll
      for (int i = 9; i < 15; ++i) w[i] = 0;
      w[15] = 64 * 8;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) h[i] = IV(i);
    compress(h, w);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) out[i] = h[4 + i];
}

}  // namespace rxd
