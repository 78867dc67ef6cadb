// bmpow_ident_fmt.h -- the byte-oriented half of the sender identification: addresses.encodeVarint, the
// leading-zero rule of addresses.encodeAddress and its base58 conversion (src/addresses.py:66-79,
// :146-180), written once for the device (bmpow_ident.hip) and for the host (tests/native/ident_sim.cpp
// builds this header with g++ and runs it against the fixture).
//
// Everything lives in fixed-size word arrays whose indices are compile-time constants after unrolling,
// so on the device a row stays in registers: a byte string of at most 48 bytes is six big-endian
// 64-bit words (SHA-512's own word order, no byte swap on the way into a block), and a byte lands at a
// run-time position through one select per word.  No table is indexed at run time; the base58 alphabet
// is arithmetic on the digit.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define ID_HD __host__ __device__ __forceinline__
#else
#define ID_HD inline
#endif
#if defined(__clang__)
#define ID_UNROLL _Pragma("unroll")
#else
#define ID_UNROLL
#endif

namespace idf {

constexpr int kMsgWords = 6;       // 48 bytes: varint(version) 9 + varint(stream) 9 + ripe 20 + checksum 4 = 42
constexpr int kMaxChars = 60;      // twelve chunks of five digits; 42 bytes need at most 58
constexpr uint32_t kChunk = 656356768u;  // 58^5, the largest power of 58 below 2^32

struct msg {  // bytes [0, len) of the string in w, big-endian within each word; zero from len on
  uint64_t w[kMsgWords];
  uint32_t len;
};

ID_HD void clear(msg& m) {
  ID_UNROLL
  for (int i = 0; i < kMsgWords; ++i) m.w[i] = 0;
  m.len = 0;
}

// b at position pos (< 48), which must still be zero
ID_HD void or_byte(msg& m, uint32_t pos, uint32_t b) {
  const uint32_t q = pos >> 3;
  const uint64_t v = (uint64_t)(b & 0xffu) << (56 - 8 * (pos & 7));
  ID_UNROLL
  for (int i = 0; i < kMsgWords; ++i) m.w[i] |= (q == (uint32_t)i) ? v : 0;
}

ID_HD void put_byte(msg& m, uint32_t b) {
  or_byte(m, m.len, b);
  m.len += 1;
}

// addresses.encodeVarint: 1, 3, 5 or 9 bytes, the shortest form
ID_HD void put_varint(msg& m, uint64_t v) {
  const uint32_t n = v < 253 ? 0u : v < 65536 ? 2u : v < 4294967296ULL ? 4u : 8u;  // value bytes behind the first
  put_byte(m, n == 0 ? (uint32_t)v : n == 2 ? 253u : n == 4 ? 254u : 255u);
  ID_UNROLL
  for (int i = 7; i >= 0; --i)
    if ((uint32_t)i < n) put_byte(m, (uint32_t)(v >> (8 * i)));
}

// byte i of a ripe kept as RIPEMD-160 leaves it: five little-endian words
ID_HD uint32_t ripe_byte(const uint32_t (&r)[5], int i) { return (r[i >> 2] >> (8 * (i & 3))) & 0xffu; }

// How many leading bytes of the ripe encodeAddress drops: versions 2 and 3 at most two zero bytes,
// version 4 every zero byte (all 20 of a zero ripe), any other version none.
ID_HD uint32_t strip_count(uint64_t version, const uint32_t (&r)[5]) {
  uint32_t z = 0;
  bool run = true;
  ID_UNROLL
  for (int i = 0; i < 20; ++i) {
    run = run && ripe_byte(r, i) == 0;
    z += run ? 1u : 0u;
  }
  if (version == 2 || version == 3) return z < 2 ? z : 2u;
  return version == 4 ? z : 0u;
}

// varint(version) || varint(stream) || ripe[skip:]
ID_HD void put_address_data(msg& m, uint64_t version, uint64_t stream, const uint32_t (&r)[5], uint32_t skip) {
  clear(m);
  put_varint(m, version);
  put_varint(m, stream);
  ID_UNROLL
  for (int i = 0; i < 20; ++i)
    if ((uint32_t)i >= skip) put_byte(m, ripe_byte(r, i));
}

ID_HD void put_be32(msg& m, uint32_t v) {
  ID_UNROLL
  for (int i = 3; i >= 0; --i) put_byte(m, v >> (8 * i));
}

// The string as its one padded SHA-512 block (len <= 111 always holds here).
ID_HD void sha512_block(const msg& m, uint64_t (&w)[16]) {
  msg t = m;
  or_byte(t, t.len, 0x80);
  ID_UNROLL
  for (int i = 0; i < kMsgWords; ++i) w[i] = t.w[i];
  ID_UNROLL
  for (int i = kMsgWords; i < 15; ++i) w[i] = 0;
  w[15] = 8ull * m.len;
}

ID_HD uint32_t base58_char(uint32_t d) {  // '1'-'9' 'A'-'H' 'J'-'N' 'P'-'Z' 'a'-'k' 'm'-'z'
  return d + (d < 9 ? 49u : d < 17 ? 56u : d < 22 ? 57u : d < 33 ? 58u : d < 44 ? 64u : 65u);
}

// encodeBase58(int(hexlify(string), 16)) of a string of at most 42 bytes: the characters come back
// left-aligned in s, four per word with the first in the top byte, zero behind the last; the result is
// their number (1 .. 58).  Leading zero bytes vanish as they do in the reference's integer, and the
// value 0 is '1'.
ID_HD uint32_t base58(const msg& m, uint32_t (&s)[kMaxChars / 4]) {
  // the string as an integer: right-aligned in 12 words, most significant first
  uint64_t w[kMsgWords];
  ID_UNROLL
  for (int i = 0; i < kMsgWords; ++i) w[i] = m.w[i];
  const uint32_t drop = 8 * kMsgWords - m.len;  // bytes to shift out on the right (>= 6)
  const uint32_t dw = drop >> 3, db = 8 * (drop & 7);
  ID_UNROLL
  for (int step = 4; step >= 1; step >>= 1) {
    const bool on = (dw & (uint32_t)step) != 0;
    ID_UNROLL
    for (int i = kMsgWords - 1; i >= 0; --i) {
      const uint64_t from = i - step >= 0 ? w[i - step >= 0 ? i - step : 0] : 0;
      w[i] = on ? from : w[i];
    }
  }
  ID_UNROLL
  for (int i = kMsgWords - 1; i >= 0; --i) {
    const uint64_t above = i > 0 ? w[i > 0 ? i - 1 : 0] : 0;
    w[i] = db ? (w[i] >> db) | (above << ((64 - db) & 63)) : w[i];
  }
  uint32_t limb[12];
  ID_UNROLL
  for (int i = 0; i < kMsgWords; ++i) {
    limb[2 * i] = (uint32_t)(w[i] >> 32);
    limb[2 * i + 1] = (uint32_t)w[i];
  }
  // twelve long divisions by 58^5; D > 2^29, so before pass k the value is below 2^(336 - 29 k) and
  // only its low ceil((336 - 29 k) / 32) limbs can be non-zero
  uint32_t chunk[kMaxChars / 5];
  ID_UNROLL
  for (int k = 0; k < kMaxChars / 5; ++k) {
    const int live = (336 - 29 * k + 31) / 32;
    uint32_t rem = 0;
    ID_UNROLL
    for (int i = 12 - live; i < 12; ++i) {
      const uint64_t x = ((uint64_t)rem << 32) | limb[i];
      const uint32_t q = (uint32_t)(x / kChunk);
      rem = (uint32_t)(x - (uint64_t)q * kChunk);
      limb[i] = q;
    }
    chunk[k] = rem;
  }
  // 60 digits, most significant first, as characters; lz counts the leading zero digits
  uint32_t lz = 0;
  bool run = true;
  ID_UNROLL
  for (int i = 0; i < kMaxChars / 4; ++i) s[i] = 0;
  ID_UNROLL
  for (int k = kMaxChars / 5 - 1; k >= 0; --k) {
    uint32_t c = chunk[k], d[5];
    ID_UNROLL
    for (int i = 0; i < 5; ++i) {
      d[i] = c % 58u;
      c /= 58u;
    }
    ID_UNROLL
    for (int i = 4; i >= 0; --i) {
      const int p = kMaxChars - 1 - (5 * k + i);  // position from the left
      run = run && d[i] == 0;
      lz += run ? 1u : 0u;
      s[p >> 2] |= base58_char(d[i]) << (24 - 8 * (p & 3));
    }
  }
  if (lz == kMaxChars) lz = kMaxChars - 1;  // the value 0: one '1'
  // left-align: shift the character string left by lz bytes
  const uint32_t sw = lz >> 2, sb = 8 * (lz & 3);
  ID_UNROLL
  for (int step = 8; step >= 1; step >>= 1) {
    const bool on = (sw & (uint32_t)step) != 0;
    ID_UNROLL
    for (int i = 0; i < kMaxChars / 4; ++i) {
      const uint32_t from = i + step < kMaxChars / 4 ? s[i + step < kMaxChars / 4 ? i + step : 0] : 0;
      s[i] = on ? from : s[i];
    }
  }
  ID_UNROLL
  for (int i = 0; i < kMaxChars / 4; ++i) {
    const uint32_t below = i + 1 < kMaxChars / 4 ? s[i + 1 < kMaxChars / 4 ? i + 1 : 0] : 0;
    s[i] = sb ? (s[i] << sb) | (below >> ((32 - sb) & 31)) : s[i];
  }
  return kMaxChars - lz;
}

// addr_len || addr[63] of bmpow_ident_rec as sixteen words in memory order (little-endian words)
ID_HD void address_field(uint32_t nchars, const uint32_t (&s)[kMaxChars / 4], uint32_t (&out)[16]) {
  ID_UNROLL
  for (int i = 0; i < 16; ++i) {
    const uint32_t hi = i == 0 ? nchars : s[i > 0 ? i - 1 : 0];   // its low byte leads this word
    const uint32_t lo = i < kMaxChars / 4 ? s[i < kMaxChars / 4 ? i : 0] : 0;
    const uint32_t be = (hi << 24) | (lo >> 8);
    out[i] = (be >> 24) | ((be >> 8) & 0xff00u) | ((be << 8) & 0xff0000u) | (be << 24);
  }
}

}  // namespace idf
