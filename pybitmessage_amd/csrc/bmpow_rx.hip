// bmpow_rx.hip -- decrypted msgs from plaintext bytes to the inputs of the signature and identification
// kernels, and from their outputs to the final record (gfx950; include/bmpow_rx.h).
//
// Reference: processmsg, src/class_objectProcessor.py:441-452 and :488-591.  Host side: bmpow_host_rx.hip.
//
//   rx_walk_kernel   : one lane per row.  The field walk, the DER parse of the signature and the range
//                      checks of r, s and the key (bmpow_rx_fmt.h, the text the host test runs), and from
//                      them the sg_sig entry, the ec::ge key, the identification's 128 key bytes and the
//                      prefix of signedData.  A row that is rejected, or whose signature or key cannot go
//                      to the curve kernels, gets a fixed valid dummy (the generator, r = s = 1, no blocks
//                      to hash): the sets keep their shape, no compaction pass runs, and sg_scalar_kernel's
//                      1 <= r, s < n holds for every lane.  The dummy's verdict is never read.
//   rx_pack_kernel   : 16 lanes per row write prefix || plaintext[:bottom] || padding into the block pool
//                      sg_hash_kernel reads, 16 bytes per lane and pass: two aligned 16-byte loads funnelled
//                      by the prefix's length (the source is misaligned against the destination by 14, 16,
//                      18 or 22 bytes), one 16-byte store.
//   rx_finish_kernel : one lane per row.  The walk's status, the comb's verdict and the identification's
//                      ripe and address into the record, and sigHash = SHA512(SHA512(signature))[32:] of a
//                      signature that parsed (at most 72 bytes: one block each).
// Every index is checked against the row's own lengths before it is used; lanes past n do nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bmpow_rx_fmt.h"
#include "bmpow_rx_kernels.h"
#include "sha512_dev.h"

namespace {

// secp256k1's generator, little-endian limbs
__device__ const uint32_t kGx[8] = {0x16F81798u, 0x59F2815Bu, 0x2DCE28D9u, 0x029BFCDBu,
                                    0xCE870B07u, 0x55A06295u, 0xF9DCBBACu, 0x79BE667Eu};
__device__ const uint32_t kGy[8] = {0xFB10D4B8u, 0x9C47D08Fu, 0xA6855419u, 0xFD17B448u,
                                    0x0E1108A8u, 0x5DA4FBFCu, 0x26A3C465u, 0x483ADA77u};

struct PlainSrc {  // a row's plaintext for rxf::pack_chunk
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

}  // namespace

__global__ __launch_bounds__(SG_BLOCK) void rx_walk_kernel(const rx_row* __restrict__ rows,
                                                           const uint8_t* __restrict__ plain, uint32_t n,
                                                           bmpow_rx_msg_rec* __restrict__ recs, sg_sig* __restrict__ sigs,
                                                           ec::ge* __restrict__ pts, uint4* __restrict__ keys,
                                                           uint64_t* __restrict__ versions, uint64_t* __restrict__ streams,
                                                           rx_pk* __restrict__ pk, uint8_t* __restrict__ flags) {
  const uint32_t o = blockIdx.x * SG_BLOCK + threadIdx.x;
  if (o >= n) return;
  const rx_row* row = rows + o;
  const uint8_t* p = plain + row->poff;
  const uint32_t len = row->plen;
  bmpow_rx_msg_rec rec = {};
  uint32_t key_off;
  rxf::walk(row->head, row->hlen, p, len, row->to_ripe, rec, key_off);
  const bool walked = rec.status == BMPOW_RX_OK;

  uint32_t r[8], s[8], x[8], y[8];
  uint8_t flag = 0;
  if (walked) {
    if (rxf::der_parse(p + rec.sig_off, rec.sig_len, r, s)) flag |= RX_FLAG_DER;
    if (rxf::load_key(p + key_off, x, y) && (flag & RX_FLAG_DER)) flag |= RX_FLAG_REAL;
  }
  const bool real = (flag & RX_FLAG_REAL) != 0;
  sg_sig sig;
  ec::ge pt;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    sig.r.d[i] = real ? r[i] : (i == 0 ? 1u : 0u);
    sig.s.d[i] = real ? s[i] : (i == 0 ? 1u : 0u);
    pt.x.d[i] = real ? x[i] : kGx[i];
    pt.y.d[i] = real ? y[i] : kGy[i];
  }
  sig.blk = row->blk;
  sig.nblk = real ? rxf::signed_blocks(rec.prefix_len, rec.bottom) : 0u;
  sigs[o] = sig;
  pts[o] = pt;

  rx_pk k;
  k.plen = rxf::put_prefix(row->head, rec.claimed_stream, k.pre);
  k.bottom = rec.bottom;
  pk[o] = k;

  // the identification's input: the keys' bytes as they lie in the plaintext (the walk's 170-byte floor
  // keeps all 128 inside it); zeros for a row the walk rejected
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    uint32_t w[4] = {0, 0, 0, 0};
    if (walked) {
#pragma unroll
      for (int j = 0; j < 16; ++j) w[j >> 2] |= (uint32_t)p[key_off + 16 * q + j] << (8 * (j & 3));
    }
    keys[8 * (uint64_t)o + q] = make_uint4(w[0], w[1], w[2], w[3]);
  }
  versions[o] = rec.sender_version;
  streams[o] = rec.sender_stream;
  flags[o] = flag;
  recs[o] = rec;
}

__global__ __launch_bounds__(64) void rx_pack_kernel(const rx_row* __restrict__ rows, const uint4* __restrict__ plain,
                                                     uint64_t plain_chunks, const sg_sig* __restrict__ sigs,
                                                     const rx_pk* __restrict__ pk, uint32_t n, uint4* __restrict__ pool,
                                                     uint64_t pool_chunks) {
  const uint32_t o = blockIdx.x * (64 / RX_PACK_LANES) + threadIdx.x / RX_PACK_LANES;
  const uint32_t sub = threadIdx.x % RX_PACK_LANES;
  if (o >= n) return;
  const uint32_t nblk = sigs[o].nblk;
  if (nblk == 0) return;
  const uint64_t base = 4ull * sigs[o].blk;
  const rx_pk k = pk[o];
  const uint64_t first = rows[o].poff >> 4;
  PlainSrc src;
  src.len = rows[o].plen;
  src.chunks = plain + first;
  const uint64_t want = ((uint64_t)src.len + 15) >> 4, room = first < plain_chunks ? plain_chunks - first : 0;
  src.nchunks = (uint32_t)(want < room ? want : room);
  src.bytes = reinterpret_cast<const uint8_t*>(plain) + rows[o].poff;
  if ((uint64_t)src.nchunks * 16 < src.len) src.len = src.nchunks * 16;  // never past the pool
#pragma unroll 1
  for (uint32_t c = sub; c < 4 * nblk; c += RX_PACK_LANES) {
    uint32_t w[4];
    rxf::pack_chunk(c, nblk, k.pre, k.plen, k.bottom, src, w);
    if (base + c < pool_chunks) pool[base + c] = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

__global__ __launch_bounds__(SG_BLOCK) void rx_finish_kernel(const rx_row* __restrict__ rows,
                                                             const uint8_t* __restrict__ plain,
                                                             const uint8_t* __restrict__ verdict,
                                                             const uint8_t* __restrict__ flags,
                                                             const uint32_t* __restrict__ ident, uint32_t n,
                                                             uint32_t* __restrict__ recs) {
  using namespace bm;
  const uint32_t o = blockIdx.x * SG_BLOCK + threadIdx.x;
  if (o >= n) return;
  uint32_t* __restrict__ rec = recs + RX_REC_WORDS * (uint64_t)o;
  const uint8_t flag = flags[o];
  const uint32_t v = verdict[o];
  const bool walked = rec[20] == (uint32_t)BMPOW_RX_OK;
  const bool good = walked && (flag & RX_FLAG_REAL) && (v == 1 || v == 2);
  if (!walked) return;  // the walk's status stands; everything behind it is zero already
  if (!good) {
    rec[20] = (uint32_t)BMPOW_RX_BAD_SIGNATURE;
    return;
  }
  rec[51] = (rec[51] & 0xffffff00u) | v;  // digest
  const uint32_t* __restrict__ id = ident + 45 * (uint64_t)o;
#pragma unroll
  for (int i = 0; i < 5; ++i) rec[21 + i] = id[i];        // ripe
#pragma unroll
  for (int i = 0; i < 16; ++i) rec[34 + i] = id[29 + i];  // addr_len || addr
  // sigHash: the signature parsed (good implies RX_FLAG_DER), so it is 8 .. 72 bytes of the plaintext
  const uint32_t slen = rec[18] <= rxf::kMaxDer ? rec[18] : rxf::kMaxDer;
  const uint8_t* sp = plain + rows[o].poff + rec[17];
  uint64_t w[16], h[8];
#pragma unroll
  for (int i = 0; i < 16; ++i) w[i] = 0;
#pragma unroll
  for (int i = 0; i <= (int)rxf::kMaxDer; ++i) {
    const uint32_t b = (uint32_t)i < slen ? sp[(uint32_t)i < slen ? i : 0] : (uint32_t)i == slen ? 0x80u : 0u;
    w[i >> 3] |= (uint64_t)b << (56 - 8 * (i & 7));
  }
  w[15] = 8ull * slen;
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
  for (int i = 0; i < 4; ++i) {
    rec[26 + 2 * i] = __builtin_bswap32(hi32(h[4 + i]));
    rec[27 + 2 * i] = __builtin_bswap32(lo32(h[4 + i]));
  }
}

// ---------------------------------------------------------------------------------------
// Launch wrappers (C++ linkage, used by bmpow_host_rx.hip).  stride is a multiple of SG_BLOCK.
// ---------------------------------------------------------------------------------------
hipError_t rx_launch_walk(hipStream_t st, const rx_row* rows, const uint8_t* plain, uint32_t n, uint32_t stride,
                          bmpow_rx_msg_rec* recs, sg_sig* sigs, ec::ge* pts, uint4* keys, uint64_t* versions,
                          uint64_t* streams, rx_pk* pk, uint8_t* flags) {
  if (n == 0) return hipSuccess;
  if (n > stride || stride % SG_BLOCK) return hipErrorInvalidValue;
  hipLaunchKernelGGL(rx_walk_kernel, dim3(stride / SG_BLOCK), dim3(SG_BLOCK), 0, st, rows, plain, n, recs, sigs, pts, keys,
                     versions, streams, pk, flags);
  return hipGetLastError();
}

hipError_t rx_launch_pack(hipStream_t st, const rx_row* rows, const uint4* plain, uint64_t plain_chunks,
                          const sg_sig* sigs, const rx_pk* pk, uint32_t n, uint4* pool, uint64_t pool_chunks) {
  if (n == 0) return hipSuccess;
  const uint32_t per = 64 / RX_PACK_LANES;
  hipLaunchKernelGGL(rx_pack_kernel, dim3((n + per - 1) / per), dim3(64), 0, st, rows, plain, plain_chunks, sigs, pk, n,
                     pool, pool_chunks);
  return hipGetLastError();
}

hipError_t rx_launch_finish(hipStream_t st, const rx_row* rows, const uint8_t* plain, const uint8_t* verdict,
                            const uint8_t* flags, const bmpow_ident_rec* ident, uint32_t n, bmpow_rx_msg_rec* recs) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(rx_finish_kernel, dim3((n + SG_BLOCK - 1) / SG_BLOCK), dim3(SG_BLOCK), 0, st, rows, plain, verdict,
                     flags, reinterpret_cast<const uint32_t*>(ident), n, reinterpret_cast<uint32_t*>(recs));
  return hipGetLastError();
}
