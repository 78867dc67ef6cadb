// bmpow_rx_fmt.h -- the byte-oriented half of the msg processing: addresses.decodeVarint, the field walk
// of processmsg (src/class_objectProcessor.py:441-452, :488-561), the strict DER parse of the signature,
// the prefix of signedData (:562-564) and the packing of signedData into padded SHA blocks, written once
// for the device (bmpow_rx.hip), for the host-only entry point (bmpow_rx_walk_msg, bmpow_host_rx.hip) and
// for the stand-alone test program (tests/native/rx_sim.cpp builds this header with g++).  Behind the msgs'
// part: the walks of processbroadcast, decryptAndCheckPubkeyPayload and processpubkey and their prefix of up
// to 62 bytes (bmpow_rxobj.hip, bmpow_rx_walk_object in bmpow_host_rxobj.hip, tests/native/rxobj_sim.cpp).
//
// Positions are 64-bit and saturate: a length varint may be 2^64 - 1, and a slice that starts or ends past
// the plaintext is cut at its end as Python cuts it.  Bytes are read one at a time through a plain pointer
// (global memory on the device); whatever is assembled from them lives in arrays indexed by compile-time
// constants after unrolling.
#pragma once
#include <stdint.h>

#include "../../include/bmpow_rx.h"
#include "scalar_dev.h"

#if defined(__HIPCC__)
#define RX_HD __host__ __device__ __forceinline__
#else
#define RX_HD inline
#endif
#if defined(__clang__)
#define RX_UNROLL _Pragma("unroll")
#else
#define RX_UNROLL
#endif

namespace rxf {

constexpr uint32_t kHeadBytes = 38;  // data[:38]: nonce, time, type, and two varints of at most 9 bytes
constexpr uint32_t kMinPlain = 170;  // :500
constexpr uint32_t kMaxDer = 72;     // 30 46 02 21 00 r[32] 02 21 00 s[32]: the longest canonical signature

struct varint {
  uint64_t v;
  uint32_t n;  // bytes it takes; 0 for decodeVarint(b'')
  bool ok;     // false where the reference raises varintDecodeError
};

RX_HD uint64_t sat_add(uint64_t a, uint64_t b) { return a + b < a ? ~0ull : a + b; }
RX_HD uint64_t min64(uint64_t a, uint64_t b) { return a < b ? a : b; }

// decodeVarint(data[pos:pos + 9 or 10]): the window is never shorter than the longest varint, so only the
// end of the data cuts one short
RX_HD varint get_varint(const uint8_t* p, uint64_t len, uint64_t pos) {
  varint r = {0, 0, true};
  if (pos >= len) return r;
  const uint32_t first = p[pos];
  if (first < 253) {
    r.v = first;
    r.n = 1;
    return r;
  }
  const uint32_t size = first == 253 ? 2u : first == 254 ? 4u : 8u;
  if (len - pos < 1 + size) {
    r.ok = false;
    return r;
  }
  uint64_t v = 0;
  for (uint32_t i = 0; i < size; ++i) v = (v << 8) | p[pos + 1 + i];
  r.v = v;
  r.n = 1 + size;
  r.ok = v >= (first == 253 ? 253ull : first == 254 ? 65536ull : 4294967296ull);
  return r;
}

// data[pos:pos + want] as (offset, length) within a plaintext of len bytes
RX_HD void slice(uint64_t len, uint64_t pos, uint64_t want, uint32_t& off, uint32_t& got) {
  const uint64_t a = min64(pos, len), b = min64(sat_add(pos, want), len);
  off = (uint32_t)a;
  got = (uint32_t)(b - a);
}

// The walk.  head: the object's first hlen <= 38 bytes; p, len: the plaintext (len <= 2^31).  rec must be
// zeroed; status is left at the first returning line, BMPOW_RX_OK where the walk reaches :566.  key_off:
// where the two 64-byte keys start (set from :510 on).
RX_HD void walk(const uint8_t* head, uint32_t hlen, const uint8_t* p, uint64_t len, const uint8_t* to_ripe,
                bmpow_rx_msg_rec& rec, uint32_t& key_off) {
  key_off = 0;
  rec.status = BMPOW_RX_MSG_VERSION;
  const varint mv = get_varint(head, hlen, 20);
  if (!mv.ok || mv.v != 1) return;
  const varint claimed = get_varint(head, hlen, 20 + mv.n);
  if (!claimed.ok) return;
  rec.claimed_stream = claimed.v;
  rec.prefix_len = (uint8_t)(13 + (claimed.v < 253 ? 1 : claimed.v < 65536 ? 3 : claimed.v < 4294967296ull ? 5 : 9));
  rec.status = BMPOW_RX_VARINT;
  const varint ver = get_varint(p, len, 0);
  if (!ver.ok) return;
  rec.sender_version = ver.v;
  if (ver.v == 0 || ver.v > 4 || len < kMinPlain) {
    rec.status = ver.v == 0 ? BMPOW_RX_SENDER_VERSION_0 : ver.v > 4 ? BMPOW_RX_SENDER_VERSION_HIGH : BMPOW_RX_TOO_SHORT;
    return;
  }
  uint64_t pos = ver.n;
  const varint stream = get_varint(p, len, pos);
  if (!stream.ok) return;
  rec.sender_stream = stream.v;
  if (stream.v == 0) {
    rec.status = BMPOW_RX_SENDER_STREAM_0;
    return;
  }
  pos += stream.n;  // at most 18 + 4 + 128 + 18 = 168 < 170 <= len from here to the end of the keys' varints
  RX_UNROLL
  for (int i = 0; i < 4; ++i) rec.behaviour[i] = p[pos + i];
  pos += 4;
  key_off = (uint32_t)pos;
  pos += 128;
  if (ver.v >= 3) {
    const varint ntpb = get_varint(p, len, pos);
    if (!ntpb.ok) return;
    rec.ntpb = ntpb.v;
    pos += ntpb.n;
    const varint extra = get_varint(p, len, pos);
    if (!extra.ok) return;
    rec.extra = extra.v;
    pos += extra.n;
  }
  rec.end_of_pubkey = (uint32_t)pos;
  bool mine = len - pos >= 20;  // a toRipe slice cut short is not the 20 bytes it is compared with
  if (mine) {
    uint32_t diff = 0;
    for (int i = 0; i < 20; ++i) diff |= (uint32_t)(p[pos + i] ^ to_ripe[i]);
    mine = diff == 0;
  }
  if (!mine) {
    rec.status = BMPOW_RX_WRONG_TO_RIPE;
    return;
  }
  pos += 20;
  const varint enc = get_varint(p, len, pos);
  if (!enc.ok) return;
  rec.encoding = enc.v;
  pos += enc.n;
  const varint mlen = get_varint(p, len, pos);
  if (!mlen.ok) return;
  pos += mlen.n;
  slice(len, pos, mlen.v, rec.msg_off, rec.msg_len);
  pos = sat_add(pos, mlen.v);
  const varint alen = get_varint(p, len, pos);
  if (!alen.ok) return;
  pos = sat_add(pos, alen.n);
  slice(len, pos, alen.v, rec.ack_off, rec.ack_len);
  pos = sat_add(pos, alen.v);
  rec.bottom = (uint32_t)min64(pos, len);
  const varint slen = get_varint(p, len, pos);
  if (!slen.ok) return;
  pos = sat_add(pos, slen.n);
  slice(len, pos, slen.v, rec.sig_off, rec.sig_len);
  rec.status = BMPOW_RX_OK;
}

// 32 big-endian bytes at v[0 .. l), l <= 32, right-aligned, as 8 little-endian limbs
RX_HD void limbs_from_be(const uint8_t* v, uint32_t l, uint32_t (&d)[8]) {
  RX_UNROLL
  for (int i = 0; i < 8; ++i) d[i] = 0;
  RX_UNROLL
  for (int k = 0; k < 32; ++k) {  // byte k from the least significant end
    const uint32_t b = (uint32_t)k < l ? v[l - 1 - k] : 0u;
    d[k >> 2] |= b << (8 * (k & 3));
  }
}

RX_HD bool scalar_in_range(const uint32_t (&d)[8]) {  // 1 <= d < n
  sn::sc a, t;
  RX_UNROLL
  for (int i = 0; i < 8; ++i) a.d[i] = d[i];
  return !sn::is_zero(a) && !sn::cond_sub_n(t, a);
}

RX_HD bool coord_in_range(const uint32_t (&d)[8]) {  // d < p = 2^256 - 2^32 - 977
  bool all_ones = true;
  RX_UNROLL
  for (int i = 7; i >= 2; --i) all_ones = all_ones && d[i] == 0xFFFFFFFFu;
  if (!all_ones) return true;
  if (d[1] != 0xFFFFFFFEu) return d[1] < 0xFFFFFFFEu;
  return d[0] < 0xFFFFFC2Fu;
}

// One DER INTEGER at p[pos ..): minimal, non-negative, at most 32 value bytes (the rules of bmpow_sig_parse)
RX_HD bool der_int(const uint8_t* p, uint32_t len, uint32_t& pos, uint32_t (&out)[8]) {
  if (len - pos < 2 || p[pos] != 0x02) return false;
  uint32_t l = p[pos + 1];
  if (l == 0 || l >= 0x80 || len - pos - 2 < l) return false;
  const uint8_t* v = p + pos + 2;
  if (v[0] & 0x80) return false;
  if (l > 1 && v[0] == 0 && !(v[1] & 0x80)) return false;
  pos += 2 + l;
  if (v[0] == 0) ++v, --l;
  if (l > 32) return false;
  limbs_from_be(v, l, out);
  return true;
}

// exactly one canonical SEQUENCE { INTEGER r, INTEGER s } with 1 <= r, s < n
RX_HD bool der_parse(const uint8_t* p, uint32_t len, uint32_t (&r)[8], uint32_t (&s)[8]) {
  if (len < 8 || len > kMaxDer || p[0] != 0x30 || p[1] >= 0x80 || (uint32_t)p[1] != len - 2) return false;
  uint32_t pos = 2;
  if (!der_int(p, len, pos, r) || !der_int(p, len, pos, s) || pos != len) return false;
  return scalar_in_range(r) && scalar_in_range(s);
}

// X || Y (64 big-endian bytes) as limbs; false for a coordinate that is not below p
RX_HD bool load_key(const uint8_t* p, uint32_t (&x)[8], uint32_t (&y)[8]) {
  limbs_from_be(p, 32, x);
  limbs_from_be(p + 32, 32, y);
  return coord_in_range(x) && coord_in_range(y);
}

// data[8:20] || varint(1) || varint(claimed_stream) as 24 bytes in memory order (little-endian words), zero
// behind its 14, 16, 18 or 22 bytes; the result is that length
RX_HD uint32_t put_prefix(const uint8_t* head, uint64_t claimed, uint32_t (&pre)[6]) {
  const uint32_t nv = claimed < 253 ? 0u : claimed < 65536 ? 2u : claimed < 4294967296ull ? 4u : 8u;
  RX_UNROLL
  for (int i = 0; i < 6; ++i) pre[i] = 0;
  RX_UNROLL
  for (int i = 0; i < 12; ++i) pre[i >> 2] |= (uint32_t)head[8 + i] << (8 * (i & 3));
  pre[3] |= 1u;  // byte 12: encodeVarint(1)
  const uint32_t first = nv == 0 ? (uint32_t)claimed : nv == 2 ? 253u : nv == 4 ? 254u : 255u;
  pre[3] |= first << 8;  // byte 13
  RX_UNROLL
  for (int i = 1; i <= 8; ++i) {  // value byte i of nv, most significant first, at byte 13 + i
    const uint32_t b = (uint32_t)i <= nv ? (uint32_t)(claimed >> (8 * (nv - (uint32_t)i))) & 0xffu : 0u;
    pre[(13 + i) >> 2] |= b << (8 * ((13 + i) & 3));
  }
  return 14 + nv;
}

RX_HD uint32_t signed_blocks(uint32_t prefix_len, uint32_t bottom) {  // ceil((len + 9) / 64)
  return (uint32_t)(((uint64_t)prefix_len + bottom + 9 + 63) / 64);
}
// what the host reserves before the walk has run: no prefix is longer than 22 bytes, bottom <= len
RX_HD uint32_t signed_blocks_bound(uint64_t plain_len) { return (uint32_t)((22 + plain_len + 9 + 63) / 64); }

template <int NW>
RX_HD uint32_t word_at(const uint32_t (&pre)[NW], uint32_t q) {  // no run-time index: one select per word
  uint32_t w = 0;
  RX_UNROLL
  for (int i = 0; i < NW; ++i) w = q == (uint32_t)i ? pre[i] : w;
  return w;
}

// Chunk c (16 bytes, four words in memory order) of the padded signed data
//     prefix[:plen] || source[skip : skip + bottom] || 0x80 || zeros || the bit length as 8 big-endian bytes
// of nblk 64-byte blocks; the prefix is NW words.  src.load16(k, w) gives bytes [16 k, 16 k + 16) of the
// source as four words (zero past its storage), src.byte(i) one byte.  A chunk that lies within the source is
// two aligned 16-byte loads funnelled by (skip - plen) mod 16; only the chunks at either end go byte by byte.
template <int NW, class Src>
RX_HD void pack_chunk_n(uint32_t c, uint32_t nblk, const uint32_t (&pre)[NW], uint32_t plen, uint32_t bottom, uint32_t skip,
                        const Src& src, uint32_t (&out)[4]) {
  const uint64_t q0 = 16ull * c, len = (uint64_t)plen + bottom, total = 64ull * nblk;
  if (q0 >= plen && q0 + 16 <= len) {
    const uint64_t a = q0 - plen + skip;
    const uint32_t k = (uint32_t)(a >> 4), sh = (uint32_t)a & 15u, ws = sh >> 2, bs = 8 * (sh & 3u);
    uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t lo[4], hi[4] = {0, 0, 0, 0};
    src.load16(k, lo);
    if (sh) src.load16(k + 1, hi);
    RX_UNROLL
    for (int i = 0; i < 4; ++i) w[i] = lo[i], w[4 + i] = hi[i];
    uint32_t t[5];
    RX_UNROLL
    for (int i = 0; i < 5; ++i)
      t[i] = ws == 0 ? w[i] : ws == 1 ? w[i + 1 < 8 ? i + 1 : 7] : ws == 2 ? w[i + 2 < 8 ? i + 2 : 7] : w[i + 3 < 8 ? i + 3 : 7];
    RX_UNROLL
    for (int i = 0; i < 4; ++i) out[i] = bs ? (t[i] >> bs) | (t[i + 1] << ((32 - bs) & 31)) : t[i];
    return;
  }
  const uint64_t bits = 8 * len;
  RX_UNROLL
  for (int i = 0; i < 4; ++i) out[i] = 0;
  RX_UNROLL
  for (int j = 0; j < 16; ++j) {
    const uint64_t q = q0 + j;
    uint32_t b = 0;
    if (q < plen) b = (word_at(pre, (uint32_t)q >> 2) >> (8 * ((uint32_t)q & 3))) & 0xffu;
    else if (q < len) b = src.byte((uint32_t)(q - plen) + skip);
    else if (q == len) b = 0x80u;
    else if (q + 8 >= total) b = (uint32_t)(bits >> (8 * (total - 1 - q))) & 0xffu;
    out[j >> 2] |= b << (8 * (j & 3));
  }
}

// the msgs' instantiation: six words of prefix (14 .. 22 bytes), the plaintext from its first byte
template <class Src>
RX_HD void pack_chunk(uint32_t c, uint32_t nblk, const uint32_t (&pre)[6], uint32_t plen, uint32_t bottom, const Src& src,
                      uint32_t (&out)[4]) {
  pack_chunk_n<6>(c, nblk, pre, plen, bottom, 0u, src, out);
}

// ---------------------------------------------------------------------------------------
// Broadcasts and pubkeys (bmpow_rxobj.hip, bmpow_rx_walk_object): processbroadcast
// (src/class_objectProcessor.py:756-926), decryptAndCheckPubkeyPayload (src/protocol.py:412-518) and
// processpubkey (:276-408).  rec must be zeroed but for its kind.
// ---------------------------------------------------------------------------------------
constexpr uint32_t kObjHeadBytes = 70;    // data[:70]: nonce, time, type, two varints of at most 9 bytes, a tag
constexpr uint32_t kObjPrefixWords = 16;  // obj[8:payload_off]: at most 62 bytes
constexpr uint32_t kV2Min = 146;          // :293
constexpr uint32_t kV3Min = 170;          // :346

struct obj_walk {
  uint32_t key_off;  // where the two 64-byte keys start in the source
  uint32_t skip;     // where the signed bytes start in the source (8 for a clear pubkey)
  bool keys;         // the keys lie whole in the source and go to the identification
  bool sig;          // the walk got through and there is a signature to check
};

RX_HD void clipped4(const uint8_t* p, uint64_t len, uint64_t pos, uint8_t (&out)[4]) {
  RX_UNROLL
  for (int i = 0; i < 4; ++i) out[i] = pos + i < len ? p[pos + i] : (uint8_t)0;
}

// The header of a broadcast: :756-769 and the tag of :808.  status is OK where the walk goes on.
RX_HD void walk_broadcast_header(const uint8_t* head, uint32_t hlen, bmpow_rx_obj_rec& rec) {
  rec.status = BMPOW_RXO_VARINT;
  const varint bv = get_varint(head, hlen, 20);
  if (!bv.ok) return;
  rec.object_version = bv.v;
  if (bv.v < 4 || bv.v > 5) {
    rec.status = BMPOW_RXO_BC_VERSION;
    return;
  }
  const varint st = get_varint(head, hlen, 20 + bv.n);
  if (!st.ok) return;
  rec.object_stream = st.v;
  const uint32_t pos = 20 + bv.n + st.n;  // <= hlen: bv was read there
  rec.tag_off = pos;
  rec.payload_off = bv.v == 5 ? (uint32_t)min64(pos + 32, hlen) : pos;
  rec.prefix_len = (uint8_t)(rec.payload_off - 8);
  rec.status = BMPOW_RXO_OK;
}

RX_HD void walk_broadcast(const uint8_t* head, uint32_t hlen, const uint8_t* p, uint64_t len, bmpow_rx_obj_rec& rec,
                          obj_walk& w) {
  walk_broadcast_header(head, hlen, rec);
  if (rec.status != BMPOW_RXO_OK) return;
  rec.status = BMPOW_RXO_VARINT;
  const bool v4 = rec.object_version == 4;
  const varint ver = get_varint(p, len, 0);
  if (!ver.ok) return;
  rec.sender_version = ver.v;
  if (v4 ? (ver.v < 2 || ver.v > 3) : ver.v < 4) {
    rec.status = BMPOW_RXO_SENDER_VERSION;
    return;
  }
  uint64_t pos = ver.n;
  const varint stream = get_varint(p, len, pos);
  if (!stream.ok) return;
  rec.sender_stream = stream.v;
  if (stream.v != rec.object_stream) {
    rec.status = BMPOW_RXO_STREAM_MISMATCH;
    return;
  }
  pos += stream.n;
  clipped4(p, len, pos, rec.behaviour);
  pos += 4;
  w.key_off = (uint32_t)pos;  // at most 22
  pos += 128;
  if (ver.v >= 3) {
    const varint ntpb = get_varint(p, len, pos);
    if (!ntpb.ok) return;
    rec.ntpb = ntpb.v;
    pos += ntpb.n;
    const varint extra = get_varint(p, len, pos);
    if (!extra.ok) return;
    rec.extra = extra.v;
    pos += extra.n;
  }
  rec.end_of_pubkey = (uint32_t)min64(pos, len);
  // :882 / :893.  Keys cut short by the end of the plaintext hash to another ripe and another tag, and a tag
  // cut short by the end of the object equals no 32 bytes: those are decided here; whole ones on the device.
  if (len < (uint64_t)w.key_off + 128 || (!v4 && rec.payload_off - rec.tag_off != 32)) {
    rec.status = v4 ? BMPOW_RXO_WRONG_RIPE : BMPOW_RXO_WRONG_TAG;
    return;
  }
  w.keys = true;
  rec.keys_hashed = 1;
  const varint enc = get_varint(p, len, pos);
  if (!enc.ok) return;
  rec.encoding = enc.v;
  if (enc.v == 0) {
    rec.status = BMPOW_RXO_ENCODING_0;
    return;
  }
  pos += enc.n;
  const varint mlen = get_varint(p, len, pos);
  if (!mlen.ok) return;
  pos += mlen.n;
  slice(len, pos, mlen.v, rec.msg_off, rec.msg_len);
  pos = sat_add(pos, mlen.v);
  rec.bottom = (uint32_t)min64(pos, len);
  const varint slen = get_varint(p, len, pos);
  if (!slen.ok) return;
  pos = sat_add(pos, slen.n);
  slice(len, pos, slen.v, rec.sig_off, rec.sig_len);
  rec.status = BMPOW_RXO_OK;
  w.sig = true;
}

// The header of an encrypted pubkey: protocol.py:412-439
RX_HD void walk_pubkey_v4_header(const uint8_t* head, uint32_t hlen, bmpow_rx_obj_rec& rec) {
  rec.status = BMPOW_RXO_VARINT;
  const varint ver = get_varint(head, hlen, 20);
  if (!ver.ok) return;
  rec.object_version = ver.v;
  const varint st = get_varint(head, hlen, 20 + ver.n);
  if (!st.ok) return;
  rec.object_stream = st.v;
  rec.tag_off = (uint32_t)min64(20 + ver.n + st.n, hlen);
  rec.payload_off = (uint32_t)min64(rec.tag_off + 32, hlen);
  rec.prefix_len = (uint8_t)(rec.payload_off > 8 ? rec.payload_off - 8 : 0);
  rec.status = BMPOW_RXO_OK;
}

RX_HD void walk_pubkey_v4(const uint8_t* head, uint32_t hlen, const uint8_t* p, uint64_t len, bmpow_rx_obj_rec& rec,
                          obj_walk& w) {
  walk_pubkey_v4_header(head, hlen, rec);
  if (rec.status != BMPOW_RXO_OK) return;
  rec.status = BMPOW_RXO_VARINT;
  rec.sender_version = rec.object_version;
  rec.sender_stream = rec.object_stream;
  clipped4(p, len, 0, rec.behaviour);
  w.key_off = 4;
  uint64_t pos = 132;
  const varint ntpb = get_varint(p, len, pos);
  if (!ntpb.ok) return;
  rec.ntpb = ntpb.v;
  pos += ntpb.n;
  const varint extra = get_varint(p, len, pos);
  if (!extra.ok) return;
  rec.extra = extra.v;
  pos += extra.n;
  rec.end_of_pubkey = rec.bottom = (uint32_t)min64(pos, len);
  const varint slen = get_varint(p, len, pos);
  if (!slen.ok) return;
  pos += slen.n;
  slice(len, pos, slen.v, rec.sig_off, rec.sig_len);
  if (len < 132) {  // a key cut short is no key: verify says False (protocol.py:484)
    rec.status = BMPOW_RXO_BAD_SIGNATURE;
    return;
  }
  w.keys = w.sig = true;
  rec.keys_hashed = 1;
  rec.status = BMPOW_RXO_OK;
}

// A clear pubkey, p the object itself: :276-308 (version 2) and :345-368 (version 3)
RX_HD void walk_pubkey(const uint8_t* p, uint64_t len, bmpow_rx_obj_rec& rec, obj_walk& w) {
  rec.status = BMPOW_RXO_VARINT;
  const varint ver = get_varint(p, len, 20);
  if (!ver.ok) return;
  const varint st = get_varint(p, len, 20 + ver.n);
  if (!st.ok) return;
  rec.object_version = rec.sender_version = ver.v;
  rec.object_stream = rec.sender_stream = st.v;
  uint64_t pos = 20 + ver.n + st.n;
  rec.payload_off = (uint32_t)min64(pos, len);
  if (ver.v < 2 || ver.v > 3) {
    rec.status = ver.v == 0 ? BMPOW_RXO_ADDRESS_VERSION_0 : ver.v == 4 ? BMPOW_RXO_NEEDS_DECRYPTION : BMPOW_RXO_ADDRESS_VERSION;
    return;
  }
  if (len < (ver.v == 2 ? kV2Min : kV3Min)) {
    rec.status = BMPOW_RXO_TOO_SHORT;
    return;
  }
  clipped4(p, len, pos, rec.behaviour);
  pos += 4;
  w.key_off = (uint32_t)pos;  // at most 42
  if (ver.v == 2) {
    if (len - (pos + 64) < 64) {  // pos + 64 <= 106 < 146 <= len
      rec.status = BMPOW_RXO_KEY_SHORT;
      return;
    }
    rec.end_of_pubkey = (uint32_t)pos + 128;
    w.keys = true;
    rec.keys_hashed = 1;
    rec.status = BMPOW_RXO_OK;
    return;
  }
  pos += 128;  // at most 170 <= len
  const varint ntpb = get_varint(p, len, pos);
  if (!ntpb.ok) return;
  rec.ntpb = ntpb.v;
  pos += ntpb.n;
  const varint extra = get_varint(p, len, pos);
  if (!extra.ok) return;
  rec.extra = extra.v;
  pos += extra.n;  // a varint that was read lies inside: pos <= len
  rec.end_of_pubkey = (uint32_t)pos;
  rec.bottom = (uint32_t)pos - 8;
  w.skip = 8;
  const varint slen = get_varint(p, len, pos);
  if (!slen.ok) return;
  pos += slen.n;
  slice(len, pos, slen.v, rec.sig_off, rec.sig_len);
  w.keys = w.sig = true;
  rec.keys_hashed = 1;
  rec.status = BMPOW_RXO_OK;
}

// one row of any kind; kind is one of BMPOW_RXO_KIND_*
RX_HD void walk_object(uint32_t kind, const uint8_t* head, uint32_t hlen, const uint8_t* p, uint64_t len,
                       bmpow_rx_obj_rec& rec, obj_walk& w) {
  w.key_off = w.skip = 0;
  w.keys = w.sig = false;
  rec.kind = (uint8_t)kind;
  if (kind == BMPOW_RXO_KIND_BROADCAST) walk_broadcast(head, hlen, p, len, rec, w);
  else if (kind == BMPOW_RXO_KIND_PUBKEY_V4) walk_pubkey_v4(head, hlen, p, len, rec, w);
  else walk_pubkey(p, len, rec, w);
}

// obj[8:payload_off] as 64 bytes in memory order, zero behind its prefix_len bytes; head holds hlen >=
// payload_off bytes
RX_HD void put_prefix_obj(const uint8_t* head, uint32_t payload_off, uint32_t (&pre)[kObjPrefixWords]) {
  RX_UNROLL
  for (int i = 0; i < (int)kObjPrefixWords; ++i) pre[i] = 0;
  RX_UNROLL
  for (int i = 0; i < 62; ++i) {
    const uint32_t b = 8u + (uint32_t)i < payload_off ? head[8 + i] : 0u;
    pre[i >> 2] |= b << (8 * (i & 3));
  }
}

// what the host reserves for a row before the walk has run: no prefix is longer than 62 bytes
RX_HD uint32_t signed_blocks_bound_obj(uint64_t source_len) { return (uint32_t)((62 + source_len + 9 + 63) / 64); }

}  // namespace rxf
