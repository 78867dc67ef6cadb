// bmpow_tx_fmt.h -- the byte-oriented half of the assembly of outgoing objects (bmpow_tx.hip): where a row's
// pieces lie in its slot, the packing of head || body into padded SHA blocks, the canonical DER of (r, s),
// the tail varint(len(sig)) || sig behind the body, and the big-endian words of the payload the final
// SHA-512 reads -- written once for the device, for the host unit (bmpow_tx_layout_row, bmpow_host_tx.hip)
// and for the stand-alone test program (tests/native/tx_sim.cpp builds this header with g++).
//
// A row's slot is the seal's (bmpow_seal_rows.h): the body at SL_PLAIN_AT, the tail right behind it, so
// that body || tail is the plaintext sl_seal_kernel reads; a clear row's payload is the head and those same
// bytes.  The slot is sized for the longest tail (73 bytes), whatever the signature's length turns out to be.
//
// Bytes go through plain pointers (global memory on the device) with byte stores or memcpy; whatever is
// assembled from them lives in arrays indexed by compile-time constants after unrolling.
#pragma once
#include <stdint.h>

#include "bmpow_seal_plan.h"  // SL_PLAIN_AT, seal_slot_bytes

#if defined(__HIPCC__)
#define TX_HD __host__ __device__ __forceinline__
#else
#define TX_HD inline
#endif
#if defined(__clang__)
#define TX_UNROLL _Pragma("unroll")
#else
#define TX_UNROLL
#endif

namespace txf {

constexpr uint32_t kHeadMin = 12;  // time, type, two one-byte varints
constexpr uint32_t kHeadMax = 62;  // two nine-byte varints and a tag
constexpr uint32_t kMaxDer = 72;   // 30 46 02 21 00 r[32] 02 21 00 s[32]
constexpr uint32_t kTailMax = 1 + kMaxDer;
constexpr uint32_t kMaxBody = 1u << 18;    // a longer body cannot fit an object
constexpr uint32_t kMaxObject = 1u << 18;  // nonce included

TX_HD uint32_t body_at() { return SL_PLAIN_AT; }
TX_HD uint32_t tail_at(uint32_t body_len) { return SL_PLAIN_AT + body_len; }
TX_HD uint32_t signed_blocks(uint32_t signed_len) { return (signed_len + 9 + 63) / 64; }
// host only: the slot of a row, whatever its kind and its signature's length
inline uint64_t slot_bytes(uint64_t body_len) { return bmseal::seal_slot_bytes(body_len + kTailMax); }

// Chunk c (16 bytes) of  head || body || 0x80 || zeros || bit length  in nblk 64-byte blocks, as four words
// in memory order.  c < 4 nblk, nblk == signed_blocks(head_len + body_len).
TX_HD void pack_chunk(uint32_t c, uint32_t nblk, const uint8_t* head, uint32_t head_len, const uint8_t* body,
                      uint32_t body_len, uint32_t (&w)[4]) {
  const uint32_t at = 16 * c, signed_len = head_len + body_len, total = 64 * nblk;
  if (at >= head_len && at + 16 <= signed_len) {  // wholly inside the body
    __builtin_memcpy(w, body + (at - head_len), 16);
    return;
  }
  const uint64_t bits = (uint64_t)signed_len * 8;
  TX_UNROLL
  for (int q = 0; q < 4; ++q) w[q] = 0;
  TX_UNROLL
  for (int j = 0; j < 16; ++j) {
    const uint32_t i = at + (uint32_t)j;
    uint32_t b = 0;
    if (i < head_len) b = head[i];
    else if (i < signed_len) b = body[i - head_len];
    else if (i == signed_len) b = 0x80;
    else if (i + 8 >= total) b = (uint32_t)(bits >> (8 * (total - 1 - i))) & 0xffu;
    w[j >> 2] |= b << (8 * (j & 3));
  }
}

// leading zero bytes of the 256-bit v (big-endian words, the top word first; not zero): 0 .. 31, and
// whether the first byte that is kept has its top bit set
TX_HD uint32_t lead_zero_bytes(const uint32_t (&v)[8], bool& top_set) {
  uint32_t z = 0;
  bool run = true;
  top_set = false;
  TX_UNROLL
  for (int i = 0; i < 8; ++i) {
    const uint32_t lz = v[i] == 0 ? 32u : (uint32_t)__builtin_clz(v[i]);
    if (run && v[i] != 0) top_set = (lz & 7u) == 0;
    z += run ? lz >> 3 : 0u;
    run = run && v[i] == 0;
  }
  return z < 31 ? z : 31;
}

// a DER INTEGER of v: minimal, a 0x00 in front of a set top bit; returns its length, 3 .. 35
TX_HD uint32_t der_int(uint8_t* dst, const uint32_t (&v)[8]) {
  bool top;
  const uint32_t skip = lead_zero_bytes(v, top), pad = top ? 1u : 0u, l = 32 - skip + pad;
  dst[0] = 0x02;
  dst[1] = (uint8_t)l;
  if (pad) dst[2] = 0;
  uint8_t* p = dst + 2 + pad;
  TX_UNROLL
  for (int i = 0; i < 32; ++i)
    if ((uint32_t)i >= skip) p[(uint32_t)i - skip] = (uint8_t)(v[i / 4] >> (24 - 8 * (i % 4)));
  return 2 + l;
}

// SEQUENCE { INTEGER r, INTEGER s }, the bytes of the host's bmpow_sig_der; r, s not zero; returns 8 .. 72
TX_HD uint32_t put_sig(uint8_t* dst, const uint32_t (&r)[8], const uint32_t (&s)[8]) {
  const uint32_t lr = der_int(dst + 2, r), ls = der_int(dst + 2 + lr, s);
  dst[0] = 0x30;
  dst[1] = (uint8_t)(lr + ls);  // at most 70: short form
  return 2 + lr + ls;
}

// varint(len(sig)) || sig behind the body in the row's slot; returns len(sig).  The plaintext the seal reads
// is then body_len + 1 + len(sig) bytes at SL_PLAIN_AT.
TX_HD uint32_t put_tail(uint8_t* slot, uint32_t body_len, const uint32_t (&r)[8], const uint32_t (&s)[8]) {
  uint8_t* p = slot + tail_at(body_len);
  const uint32_t n = put_sig(p + 1, r, s);
  p[0] = (uint8_t)n;  // below 253: a one-byte varint
  return n;
}

// Big-endian 64-bit word k of  head || src || 0x80 || zeros  (the SHA-512 message of a payload without its
// length field).
TX_HD uint64_t msg_word(uint32_t k, const uint8_t* head, uint32_t head_len, const uint8_t* src, uint32_t src_len) {
  const uint32_t at = 8 * k, len = head_len + src_len;
  if (at >= head_len && at + 8 <= len) {
    uint64_t t;
    __builtin_memcpy(&t, src + (at - head_len), 8);
    return __builtin_bswap64(t);
  }
  if (at > len) return 0;
  uint64_t w = 0;
  TX_UNROLL
  for (int j = 0; j < 8; ++j) {
    const uint32_t i = at + (uint32_t)j;
    const uint32_t b = i < head_len ? head[i] : i < len ? src[i - head_len] : i == len ? 0x80u : 0u;
    w = w << 8 | b;
  }
  return w;
}

TX_HD uint32_t payload_blocks(uint32_t len) { return (len + 17 + 127) / 128; }  // SHA-512's 128-byte blocks

}  // namespace txf
