// bmpow_rx.hip -- decrypted msgs from plaintext bytes to the inputs of the signature and identification
// kernels, and from their outputs to the final record (gfx950; include/bmpow_rx.h).
//
// Reference: processmsg, src/class_objectProcessor.py:441-452 and :488-591.  Host side: bmpow_host_rx.hip, through bmpow_host_rows.h.
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

#include "bmpow_rx_dev.h"
#include "bmpow_rx_kernels.h"

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
  rxd::emit_sig(real, r, s, x, y, row->blk, rxf::signed_blocks(rec.prefix_len, rec.bottom), sigs[o], pts[o]);

  rx_pk k;
  k.plen = rxf::put_prefix(row->head, rec.claimed_stream, k.pre);
  k.bottom = rec.bottom;
  pk[o] = k;

  // the identification's input: the keys' bytes as they lie in the plaintext (the walk's 170-byte floor
  // keeps all 128 inside it); zeros for a row the walk rejected
  rxd::gather_keys(walked, p, key_off, keys + 8 * (uint64_t)o);
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
  const rx_pk k = pk[o];
  rxd::pack_row<6>(sub, RX_PACK_LANES, rows[o].poff, rows[o].plen, plain, plain_chunks, sigs[o].blk, nblk, k.pre, k.plen,
                   k.bottom, 0u, pool, pool_chunks);
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
  uint64_t h[4];
  rxd::sig_hash(sp, slen, h);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    rec[26 + 2 * i] = __builtin_bswap32(hi32(h[i]));
    rec[27 + 2 * i] = __builtin_bswap32(lo32(h[i]));
  }
}

// ---------------------------------------------------------------------------------------
// Launch wrappers (C++ linkage, the msg family's in bmpow_host_rx.h).  stride is a multiple of SG_BLOCK.
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
