// bmpow_rxobj.hip -- broadcasts and pubkeys from their bytes to the inputs of the signature and
// identification kernels, and from their outputs to the final record (gfx950; include/bmpow_rx.h).
//
// Reference: processbroadcast (src/class_objectProcessor.py:756-926), decryptAndCheckPubkeyPayload
// (src/protocol.py:412-518), processpubkey (:276-408).  Host side: bmpow_host_rxobj.hip.  The same three
// steps as bmpow_rx.hip takes for msgs, over rows of three kinds (BMPOW_RXO_KIND_*):
//
//   rxo_walk_kernel   : one lane per row, branching on its kind.  The field walk (bmpow_rx_fmt.h, the text
//                       the host test runs), the DER parse and the range checks of r, s and the key, and from
//                       them the sg_sig entry, the ec::ge key, the identification's 128 key bytes and the
//                       prefix of signedData (the object's bytes 8 .. payload_off, up to 62 of them).  A row
//                       that has no signature to check (a v2 pubkey), that the walk refuses, or whose
//                       signature or key cannot go to the curve kernels gets the msgs' dummy (the generator,
//                       r = s = 1, no blocks to hash), so the sets keep their shape.
//   rxo_pack_kernel   : 16 lanes per row write prefix || source[skip : skip + bottom] || padding into the block
//                       pool sg_hash_kernel reads: two aligned 16-byte loads funnelled by (skip - prefix
//                       length) mod 16, one 16-byte store.  skip is 8 for a clear pubkey, whose signed bytes
//                       start at the object's byte 8, and 0 for a decrypted payload.
//   rxo_finish_kernel : one lane per row.  A broadcast's ripe (v4) or tag (v5) against the expected ripe or
//                       the tag in the object -- the reference makes that comparison before it reads the
//                       encoding, so it overrides what the walk found behind it --, an encrypted pubkey's
//                       ripe after its signature, the comb's verdict, the address, and a broadcast's sigHash.
// Every index is checked against the row's own lengths before it is used; lanes past n do nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bmpow_rx_dev.h"
#include "bmpow_rxobj_kernels.h"

__global__ __launch_bounds__(SG_BLOCK) void rxo_walk_kernel(const rxo_row* __restrict__ rows,
                                                            const uint8_t* __restrict__ plain, uint32_t n,
                                                            bmpow_rx_obj_rec* __restrict__ recs, sg_sig* __restrict__ sigs,
                                                            ec::ge* __restrict__ pts, uint4* __restrict__ keys,
                                                            uint64_t* __restrict__ versions, uint64_t* __restrict__ streams,
                                                            rxo_pk* __restrict__ pk, uint8_t* __restrict__ flags) {
  const uint32_t o = blockIdx.x * SG_BLOCK + threadIdx.x;
  if (o >= n) return;
  const rxo_row* row = rows + o;
  const uint8_t* p = plain + row->poff;
  const uint32_t len = row->plen;
  const uint32_t hlen = row->hlen <= rxf::kObjHeadBytes ? row->hlen : rxf::kObjHeadBytes;
  bmpow_rx_obj_rec rec = {};
  rxf::obj_walk w;
  rxf::walk_object(row->kind, row->head, hlen, p, len, rec, w);

  uint32_t r[8], s[8], x[8], y[8];
  uint8_t flag = 0;
  if (w.sig) {  // the signature's slice and the keys lie inside the source: the walk clipped the one and saw the other
    if (rxf::der_parse(p + rec.sig_off, rec.sig_len, r, s)) flag |= RXO_FLAG_DER;
    if (rxf::load_key(p + w.key_off, x, y) && (flag & RXO_FLAG_DER)) flag |= RXO_FLAG_REAL;
  }
  const bool real = (flag & RXO_FLAG_REAL) != 0;
  rxd::emit_sig(real, r, s, x, y, row->blk, rxf::signed_blocks(rec.prefix_len, rec.bottom), sigs[o], pts[o]);

  rxo_pk k;
  rxf::put_prefix_obj(row->head, rec.payload_off <= hlen ? rec.payload_off : hlen, k.pre);
  k.plen = rec.prefix_len;
  k.bottom = rec.bottom;
  k.skip = w.skip;
  k.pad = 0;
  pk[o] = k;

  // the identification's input: the keys' bytes as they lie in the source (w.keys: all 128 inside it)
  rxd::gather_keys(w.keys, p, w.key_off, keys + 8 * (uint64_t)o);
  versions[o] = rec.sender_version;
  streams[o] = rec.sender_stream;
  flags[o] = flag;
  // field by field: the record's byte arrays (zero until the finish kernel) never become a stack copy
  bmpow_rx_obj_rec* __restrict__ d = recs + o;
  d->object_version = rec.object_version, d->object_stream = rec.object_stream;
  d->sender_version = rec.sender_version, d->sender_stream = rec.sender_stream;
  d->ntpb = rec.ntpb, d->extra = rec.extra, d->encoding = rec.encoding;
  d->payload_off = rec.payload_off, d->tag_off = rec.tag_off, d->end_of_pubkey = rec.end_of_pubkey;
  d->msg_off = rec.msg_off, d->msg_len = rec.msg_len, d->sig_off = rec.sig_off, d->sig_len = rec.sig_len;
  d->bottom = rec.bottom, d->status = rec.status;
  uint32_t* __restrict__ words = reinterpret_cast<uint32_t*>(d);
#pragma unroll
  for (int i = RXO_REC_RIPE_WORD; i < RXO_REC_BEHAVIOUR_WORD; ++i) words[i] = 0;  // ripe, sig_hash, addr_len, addr
  words[RXO_REC_BEHAVIOUR_WORD] = (uint32_t)rec.behaviour[0] | (uint32_t)rec.behaviour[1] << 8 |
                                  (uint32_t)rec.behaviour[2] << 16 | (uint32_t)rec.behaviour[3] << 24;
  words[RXO_REC_BEHAVIOUR_WORD + 1] = (uint32_t)rec.prefix_len << 8 | (uint32_t)rec.kind << 16 |  // digest 0
                                      (uint32_t)rec.keys_hashed << 24;
}

__global__ __launch_bounds__(64) void rxo_pack_kernel(const rxo_row* __restrict__ rows, const uint4* __restrict__ plain,
                                                      uint64_t plain_chunks, const sg_sig* __restrict__ sigs,
                                                      const rxo_pk* __restrict__ pk, uint32_t n, uint4* __restrict__ pool,
                                                      uint64_t pool_chunks) {
  const uint32_t o = blockIdx.x * (64 / RXO_PACK_LANES) + threadIdx.x / RXO_PACK_LANES;
  const uint32_t sub = threadIdx.x % RXO_PACK_LANES;
  if (o >= n) return;
  const uint32_t nblk = sigs[o].nblk;
  if (nblk == 0) return;
  const rxo_pk k = pk[o];
  rxd::pack_row<(int)rxf::kObjPrefixWords>(sub, RXO_PACK_LANES, rows[o].poff, rows[o].plen, plain, plain_chunks,
                                           sigs[o].blk, nblk, k.pre, k.plen, k.bottom, k.skip, pool, pool_chunks);
}

__global__ __launch_bounds__(SG_BLOCK) void rxo_finish_kernel(const rxo_row* __restrict__ rows,
                                                              const uint8_t* __restrict__ plain,
                                                              const uint8_t* __restrict__ verdict,
                                                              const uint8_t* __restrict__ flags,
                                                              const bmpow_ident_rec* __restrict__ ident, uint32_t n,
                                                              bmpow_rx_obj_rec* __restrict__ recs) {
  using namespace bm;
  const uint32_t o = blockIdx.x * SG_BLOCK + threadIdx.x;
  if (o >= n) return;
  bmpow_rx_obj_rec* __restrict__ rec = recs + o;
  const rxo_row* __restrict__ row = rows + o;
  const bmpow_ident_rec* __restrict__ id = ident + o;
  if (!rec->keys_hashed) return;  // the walk's status stands; nothing was hashed for this row
  const uint32_t kind = rec->kind;
  const uint8_t flag = flags[o];
  const uint32_t v = verdict[o];
  const bool good = (flag & RXO_FLAG_REAL) && (v == 1 || v == 2);
  uint32_t diff = 0;
  if (kind == BMPOW_RXO_KIND_BROADCAST) {
    if (rec->object_version == 4) {
      for (int i = 0; i < 20; ++i) diff |= (uint32_t)(id->ripe[i] ^ row->expect[i]);
    } else {
      // keys_hashed: the tag lies whole in the head, tag_off + 32 == payload_off <= 70
      const uint32_t t = rec->tag_off <= rxf::kObjHeadBytes - 32 ? rec->tag_off : rxf::kObjHeadBytes - 32;
      for (int i = 0; i < 32; ++i) diff |= (uint32_t)(id->tag[i] ^ row->head[t + i]);
    }
    if (diff) {  // :882 / :893 return before anything behind the keys is read
      rec->status = rec->object_version == 4 ? BMPOW_RXO_WRONG_RIPE : BMPOW_RXO_WRONG_TAG;
      rec->encoding = 0;
      rec->msg_off = rec->msg_len = rec->sig_off = rec->sig_len = rec->bottom = 0;
      return;
    }
  }
  if (rec->status != BMPOW_RXO_OK) return;
  const bool signed_kind = kind != BMPOW_RXO_KIND_PUBKEY || rec->object_version == 3;
  if (signed_kind && !good) {
    rec->status = BMPOW_RXO_BAD_SIGNATURE;
    return;
  }
  if (kind == BMPOW_RXO_KIND_PUBKEY_V4) {  // protocol.py:497, behind the signature
    for (int i = 0; i < 20; ++i) diff |= (uint32_t)(id->ripe[i] ^ row->expect[i]);
    if (diff) {
      rec->status = BMPOW_RXO_WRONG_RIPE;
      return;
    }
  }
  rec->digest = signed_kind ? (uint8_t)v : (uint8_t)0;
  for (int i = 0; i < 20; ++i) rec->ripe[i] = id->ripe[i];
  rec->addr_len = id->addr_len;
  for (int i = 0; i < 63; ++i) rec->addr[i] = id->addr[i];
  if (kind != BMPOW_RXO_KIND_BROADCAST) return;
  // sigHash: the signature parsed (good implies RXO_FLAG_DER), so it is 8 .. 72 bytes of the plaintext
  const uint32_t slen = rec->sig_len <= rxf::kMaxDer ? rec->sig_len : rxf::kMaxDer;
  const uint32_t soff = (uint64_t)rec->sig_off + slen <= row->plen ? rec->sig_off : 0u;
  const uint8_t* sp = plain + row->poff + soff;
  const uint32_t have = (uint64_t)soff + slen <= row->plen ? slen : 0u;
  uint64_t h[4];
  rxd::sig_hash(sp, have, h);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t hi = hi32(h[i]), lo = lo32(h[i]);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      rec->sig_hash[8 * i + j] = (uint8_t)(hi >> (24 - 8 * j));
      rec->sig_hash[8 * i + 4 + j] = (uint8_t)(lo >> (24 - 8 * j));
    }
  }
}

// ---------------------------------------------------------------------------------------
// Launch wrappers (C++ linkage, the object family's in bmpow_host_rxobj.hip).  stride is a multiple of SG_BLOCK.
// ---------------------------------------------------------------------------------------
hipError_t rxo_launch_walk(hipStream_t st, const rxo_row* rows, const uint8_t* plain, uint32_t n, uint32_t stride,
                           bmpow_rx_obj_rec* recs, sg_sig* sigs, ec::ge* pts, uint4* keys, uint64_t* versions,
                           uint64_t* streams, rxo_pk* pk, uint8_t* flags) {
  if (n == 0) return hipSuccess;
  if (n > stride || stride % SG_BLOCK) return hipErrorInvalidValue;
  hipLaunchKernelGGL(rxo_walk_kernel, dim3(stride / SG_BLOCK), dim3(SG_BLOCK), 0, st, rows, plain, n, recs, sigs, pts, keys,
                     versions, streams, pk, flags);
  return hipGetLastError();
}

hipError_t rxo_launch_pack(hipStream_t st, const rxo_row* rows, const uint4* plain, uint64_t plain_chunks,
                           const sg_sig* sigs, const rxo_pk* pk, uint32_t n, uint4* pool, uint64_t pool_chunks) {
  if (n == 0) return hipSuccess;
  const uint32_t per = 64 / RXO_PACK_LANES;
  hipLaunchKernelGGL(rxo_pack_kernel, dim3((n + per - 1) / per), dim3(64), 0, st, rows, plain, plain_chunks, sigs, pk, n,
                     pool, pool_chunks);
  return hipGetLastError();
}

hipError_t rxo_launch_finish(hipStream_t st, const rxo_row* rows, const uint8_t* plain, const uint8_t* verdict,
                             const uint8_t* flags, const bmpow_ident_rec* ident, uint32_t n, bmpow_rx_obj_rec* recs) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(rxo_finish_kernel, dim3((n + SG_BLOCK - 1) / SG_BLOCK), dim3(SG_BLOCK), 0, st, rows, plain, verdict,
                     flags, ident, n, recs);
  return hipGetLastError();
}
