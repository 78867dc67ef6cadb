// bmpow_tx.hip -- outgoing objects from head and body bytes to the inputs of the signing and seal kernels,
// and from their outputs to the payload's initialHash and the final record (gfx950; include/bmpow_tx.h).
//
// Reference: sendMsg, src/class_singleWorker.py:1224-1276; sendBroadcast :641-681; the pubkeys :342-378 and
// :420-465.  Host side: bmpow_host_tx.hip.  Between these kernels run, unchanged, sg_hash_kernel,
// sd_comb_kernel, sd_sign_kernel and, for the sealed rows, sd_digits_kernel, ec_prep_kernel,
// sd_shared_kernel and sl_seal_kernel.
//
//   tx_pack_kernel   : 16 lanes per row write head || body || padding into the block pool sg_hash_kernel
//                      reads, 16 bytes per lane and pass, and the row's blk / nblk into its sg_sig entry:
//                      the device's counterpart of the host's pad_blocks.
//   tx_tail_kernel   : one lane per row.  r || s as sd_sign_kernel left them become canonical DER behind a
//                      one-byte varint right behind the body in the row's seal slot (bmpow_tx_fmt.h, the text
//                      the host test runs); the seal's row gets its plaintext length, the record the
//                      signature.  r and s are read from device memory and never reach the host.
//   tx_finish_kernel : one lane per row.  SHA-512 over head || blob (sealed) or head || body || tail
//                      (clear), read from the row struct and the slot; the payload's length, the status
//                      and initialHash into the record.
// Every index is checked against the pool's size before it is used; lanes past n do nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bmpow_tx_fmt.h"
#include "bmpow_tx_kernels.h"
#include "sha512_dev.h"

__global__ __launch_bounds__(64) void tx_pack_kernel(const tx_row* __restrict__ rows, const uint8_t* __restrict__ pool,
                                                     uint64_t pool_bytes, uint32_t n, uint4* __restrict__ hpool,
                                                     uint64_t hpool_chunks, sg_sig* __restrict__ sigs) {
  const uint32_t o = blockIdx.x * (64 / TX_PACK_LANES) + threadIdx.x / TX_PACK_LANES;
  const uint32_t sub = threadIdx.x % TX_PACK_LANES;
  if (o >= n) return;
  const tx_row* row = rows + o;
  const uint32_t head_len = row->head_len, body_len = row->body_len;
  const uint64_t slot = 16ull * row->off16;
  uint32_t nblk = txf::signed_blocks(head_len + body_len);
  const uint64_t base = 4ull * row->blk;
  if (slot + txf::body_at() + body_len > pool_bytes || base + 4ull * nblk > hpool_chunks) nblk = 0;  // never
  if (sub == 0) {
    sigs[o].blk = row->blk;
    sigs[o].nblk = nblk;
  }
  const uint8_t* body = pool + slot + txf::body_at();
#pragma unroll 1
  for (uint32_t c = sub; c < 4 * nblk; c += TX_PACK_LANES) {
    uint32_t w[4];
    txf::pack_chunk(c, nblk, row->head, head_len, body, body_len, w);
    hpool[base + c] = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

__global__ __launch_bounds__(TX_BLOCK) void tx_tail_kernel(const tx_row* __restrict__ rows, const sn::sc* __restrict__ rs,
                                                           const uint8_t* __restrict__ ok, uint32_t n, uint32_t stride,
                                                           uint8_t* pool, uint64_t pool_bytes, sl_row* __restrict__ sl,
                                                           bmpow_tx_rec* __restrict__ recs) {
  const uint32_t o = blockIdx.x * TX_BLOCK + threadIdx.x;
  if (o >= n) return;
  const tx_row* row = rows + o;
  const uint32_t body_len = row->body_len;
  const uint64_t slot = 16ull * row->off16;
  bmpow_tx_rec* rec = recs + o;
  uint32_t* rw = reinterpret_cast<uint32_t*>(rec);
#pragma unroll
  for (int i = 0; i < (int)(sizeof(bmpow_tx_rec) / 4); ++i) rw[i] = 0;
  rec->kind = row->kind;
  rec->digest = row->digest;
  uint32_t sig_len = 0;
  if (ok[o] && slot + txf::tail_at(body_len) + txf::kTailMax <= pool_bytes) {
    uint32_t r[8], s[8];
    const sn::sc R = rs[o], S = rs[(size_t)stride + o];
#pragma unroll
    for (int i = 0; i < 8; ++i) r[i] = R.d[7 - i], s[i] = S.d[7 - i];
    uint8_t* p = pool + slot;
    sig_len = txf::put_tail(p, body_len, r, s);
    const uint8_t* sig = p + txf::tail_at(body_len) + 1;
    for (uint32_t i = 0; i < sig_len; ++i) rec->sig[i] = sig[i];
  }
  rec->sig_len = (uint8_t)sig_len;
  rec->plain_len = sig_len ? body_len + 1 + sig_len : 0;
  // a row without a signature still goes through the seal (the sets keep their shape): its body alone
  sl[o] = sl_row{row->off16, sig_len ? body_len + 1 + sig_len : body_len};
}

__global__ __launch_bounds__(TX_BLOCK) void tx_finish_kernel(const tx_row* __restrict__ rows,
                                                             const uint32_t* __restrict__ blob_len, uint32_t ns,
                                                             const uint8_t* __restrict__ pool, uint64_t pool_bytes,
                                                             uint32_t n, bmpow_tx_rec* __restrict__ recs) {
  using namespace bm;
  const uint32_t o = blockIdx.x * TX_BLOCK + threadIdx.x;
  if (o >= n) return;
  const tx_row* row = rows + o;
  bmpow_tx_rec* rec = recs + o;
  if (rec->sig_len == 0) {
    rec->status = BMPOW_TX_NO_SIGNATURE;
    return;
  }
  const uint64_t slot = 16ull * row->off16;
  const bool sealed = row->kind == BMPOW_TX_SEALED;
  const uint32_t src_len = sealed ? (o < ns ? blob_len[o] : 0u) : rec->plain_len;
  const uint64_t src_at = slot + (sealed ? 0u : txf::body_at());
  if (src_len == 0 || src_at + src_len > pool_bytes) {  // the second never
    rec->status = BMPOW_TX_BAD_RECIPIENT;
    return;
  }
  const uint32_t head_len = row->head_len, len = head_len + src_len;
  rec->obj_len = len;
  if (8ull + len > txf::kMaxObject) {
    rec->status = BMPOW_TX_TOO_LARGE;
    return;
  }
  const uint8_t* src = pool + src_at;
  const uint32_t nblk = txf::payload_blocks(len);
  uint64_t h[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) h[i] = IV(i);
#pragma unroll 1
  for (uint32_t b = 0; b < nblk; ++b) {
    uint64_t w[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) w[k] = txf::msg_word(16 * b + k, row->head, head_len, src, src_len);
    if (b == nblk - 1) w[15] = 8ull * len;
    compress(h, w);
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint64_t t = __builtin_bswap64(h[i]);
    __builtin_memcpy(rec->initial_hash + 8 * i, &t, 8);
  }
  rec->status = BMPOW_TX_OK;
}

// ---------------------------------------------------------------------------------------
// Launch wrappers (C++ linkage, used by bmpow_host_tx.hip).  stride is a multiple of TX_BLOCK.
// ---------------------------------------------------------------------------------------
hipError_t tx_launch_pack(hipStream_t st, const tx_row* rows, const uint8_t* pool, uint64_t pool_bytes, uint32_t n,
                          uint4* hpool, uint64_t hpool_chunks, sg_sig* sigs) {
  if (n == 0) return hipSuccess;
  if (!rows || !pool || !hpool || !sigs) return hipErrorInvalidValue;
  const uint32_t per = 64 / TX_PACK_LANES;
  hipLaunchKernelGGL(tx_pack_kernel, dim3((n + per - 1) / per), dim3(64), 0, st, rows, pool, pool_bytes, n, hpool,
                     hpool_chunks, sigs);
  return hipGetLastError();
}

hipError_t tx_launch_tail(hipStream_t st, const tx_row* rows, const sn::sc* rs, const uint8_t* ok, uint32_t n,
                          uint32_t stride, uint8_t* pool, uint64_t pool_bytes, sl_row* sl, bmpow_tx_rec* recs) {
  if (n == 0) return hipSuccess;
  if (n > stride || stride % TX_BLOCK || !rows || !rs || !ok || !pool || !sl || !recs) return hipErrorInvalidValue;
  hipLaunchKernelGGL(tx_tail_kernel, dim3(stride / TX_BLOCK), dim3(TX_BLOCK), 0, st, rows, rs, ok, n, stride, pool,
                     pool_bytes, sl, recs);
  return hipGetLastError();
}

hipError_t tx_launch_finish(hipStream_t st, const tx_row* rows, const uint32_t* blob_len, uint32_t ns, const uint8_t* pool,
                            uint64_t pool_bytes, uint32_t n, bmpow_tx_rec* recs) {
  if (n == 0) return hipSuccess;
  if (ns > n || (ns && !blob_len) || !rows || !pool || !recs) return hipErrorInvalidValue;
  hipLaunchKernelGGL(tx_finish_kernel, dim3((n + TX_BLOCK - 1) / TX_BLOCK), dim3(TX_BLOCK), 0, st, rows, blob_len, ns, pool,
                     pool_bytes, n, recs);
  return hipGetLastError();
}
