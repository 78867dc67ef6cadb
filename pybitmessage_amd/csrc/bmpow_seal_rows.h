// bmpow_seal_rows.h -- one lane's work in the seal kernels (bmpow_seal.hip): the ECIES blob of one row and
// raw AES-256-CBC of one message, as plain functions over a byte slot and table pointers, so that
// tests/native/seal_sim.cpp runs the very same code on the host against libcrypto.
//
// A row works in place in its own 16-byte-aligned slot of the set's pool.
//   seal: the host put the plaintext at slot + SL_PLAIN_AT.  The lane writes the head (22 + xl + yl bytes,
//     at most 86) at the slot's start, then block by block the ciphertext behind it -- block b is read from
//     SL_PLAIN_AT + 16 b and written to head + 16 b .. head + 16 b + 16 <= SL_PLAIN_AT + 16 (b + 1): never
//     over a block still to be read -- then the SHA-256 padding of the inner HMAC hash behind the
//     ciphertext, hashes the slot's 64-byte blocks, and writes the MAC over the padding.
//   cbc: block b is read and written at 16 b.
// The head is a multiple of 2 bytes, so the ciphertext and the MAC are stored 2-byte aligned.  All
// accesses to the slot go through byte stores or memcpy, which alias everything: the hash's loads come
// after the ciphertext's stores in program order and must stay there.  No register array is indexed by
// a run-time value.
#pragma once
#include <stdint.h>

#include "aes256_dev.h"
#include "bmpow_seal_plan.h"  // SL_PLAIN_AT and the slot's size
#include "sha256_dev.h"

namespace sl {

BM_DEV void load16(uint32_t (&w)[4], const uint8_t* p) {  // 16-byte aligned; big-endian words
  __builtin_memcpy(w, __builtin_assume_aligned(p, 16), 16);
#pragma unroll
  for (int i = 0; i < 4; ++i) w[i] = __builtin_bswap32(w[i]);
}
BM_DEV void store16(uint8_t* p, const uint32_t (&w)[4]) {  // 16-byte aligned
  uint32_t t[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) t[i] = __builtin_bswap32(w[i]);
  __builtin_memcpy(__builtin_assume_aligned(p, 16), t, 16);
}
BM_DEV void store4_a2(uint8_t* p, uint32_t be) {  // 2-byte aligned
  const uint32_t t = __builtin_bswap32(be);
  __builtin_memcpy(__builtin_assume_aligned(p, 2), &t, 4);
}

// leading zero bytes of the 32-byte big-endian integer v (v[0] the top word): 0 .. 32
BM_DEV uint32_t lead_zero_bytes(const uint32_t (&v)[8]) {
  uint32_t z = 0;
  bool run = true;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint32_t here = v[i] == 0 ? 4u : (uint32_t)__builtin_clz(v[i]) >> 3;
    z += run ? here : 0u;
    run = run && v[i] == 0;
  }
  return z;
}

// v without its first `skip` bytes, at dst
BM_DEV void put_coord(uint8_t* dst, const uint32_t (&v)[8], uint32_t skip) {
#pragma unroll
  for (int i = 0; i < 32; ++i)
    if ((uint32_t)i >= skip) dst[(uint32_t)i - skip] = (uint8_t)(v[i / 4] >> (24 - 8 * (i % 4)));
}

// the last plaintext block: `rem` bytes of p (from the top of p[0]) kept, PKCS#7's 16 - rem behind them
BM_DEV void pkcs7_pad(uint32_t (&p)[4], uint32_t rem) {
  const uint32_t padw = (16u - rem) * 0x01010101u;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t keep = rem > 4u * j ? (rem - 4u * j >= 4u ? 4u : rem - 4u * j) : 0u;
    const uint32_t mask = keep == 4u ? 0xffffffffu : (keep == 0u ? 0u : ~(0xffffffffu >> (8u * keep)));
    p[j] = (p[j] & mask) | (padw & ~mask);
  }
}

// The blob of bmpow_ecies_seal (include/bmpow_send.h) into slot; returns its length.  ke, km, iv, X, Y are
// big-endian words, the top word first.
BM_DEV uint32_t seal_row(uint8_t* slot, uint32_t len, const uint32_t (&ke)[8], const uint32_t (&km)[8],
                         const uint32_t (&iv)[4], const uint32_t (&X)[8], const uint32_t (&Y)[8], const uint32_t* te0) {
  const uint32_t xs = lead_zero_bytes(X), ys = lead_zero_bytes(Y);
  const uint32_t xl = 32 - xs, yl = 32 - ys, head = 22 + xl + yl;
#pragma unroll
  for (int i = 0; i < 16; ++i) slot[i] = (uint8_t)(iv[i / 4] >> (24 - 8 * (i % 4)));
  slot[16] = 0x02, slot[17] = 0xCA;  // secp256k1 in pyelliptic's numbering: 714
  slot[18] = 0, slot[19] = (uint8_t)xl;
  put_coord(slot + 20, X, xs);
  slot[20 + xl] = 0, slot[21 + xl] = (uint8_t)yl;
  put_coord(slot + 22 + xl, Y, ys);

  const uint32_t nfull = len / 16, rem = len % 16, clen = 16 * (nfull + 1);
  {
    uint32_t rk[60], c[4], p[4];
    aes::expand_key(rk, ke, te0);
#pragma unroll
    for (int i = 0; i < 4; ++i) c[i] = iv[i];
    const uint8_t* src = slot + SL_PLAIN_AT;
    uint8_t* dst = slot + head;
    for (uint32_t b = 0; b <= nfull; ++b) {
      load16(p, src + 16 * (size_t)b);
      if (b == nfull) pkcs7_pad(p, rem);
#pragma unroll
      for (int i = 0; i < 4; ++i) c[i] ^= p[i];
      aes::encrypt_block(c, rk, te0);
#pragma unroll
      for (int i = 0; i < 4; ++i) store4_a2(dst + 16 * (size_t)b + 4 * i, c[i]);
    }
  }

  // the inner hash's tail: 0x80, zeros, the bit length of (K ^ ipad) || maced bytes
  const uint32_t maced = head + clen, nblk = (maced + 9 + 63) / 64, total = nblk * 64;
  slot[maced] = 0x80;
  for (uint32_t i = maced + 1; i < total - 8; ++i) slot[i] = 0;
  const uint64_t bits = (uint64_t)(64 + maced) * 8;
#pragma unroll
  for (int j = 0; j < 8; ++j) slot[total - 8 + j] = (uint8_t)(bits >> (56 - 8 * j));

  uint32_t hi[8], ho[8];
  s256::hmac_key_states(hi, ho, km);
  for (uint32_t b = 0; b < nblk; ++b) {
    uint32_t w[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      uint32_t t[4];
      load16(t, slot + 64 * (size_t)b + 16 * q);
#pragma unroll
      for (int i = 0; i < 4; ++i) w[4 * q + i] = t[i];
    }
    s256::compress(hi, w);
  }
  s256::hmac_outer(ho, hi);
#pragma unroll
  for (int i = 0; i < 8; ++i) store4_a2(slot + maced + 4 * i, ho[i]);
  return maced + 32;
}

// AES-256-CBC with PKCS#7 padding of slot[0 .. len) in place; returns 16 (len / 16 + 1).
BM_DEV uint32_t cbc_encrypt_row(uint8_t* slot, uint32_t len, const uint32_t (&key)[8], const uint32_t (&iv)[4],
                                const uint32_t* te0) {
  const uint32_t nfull = len / 16, rem = len % 16;
  uint32_t rk[60], c[4], p[4];
  aes::expand_key(rk, key, te0);
#pragma unroll
  for (int i = 0; i < 4; ++i) c[i] = iv[i];
  for (uint32_t b = 0; b <= nfull; ++b) {
    load16(p, slot + 16 * (size_t)b);
    if (b == nfull) pkcs7_pad(p, rem);
#pragma unroll
    for (int i = 0; i < 4; ++i) c[i] ^= p[i];
    aes::encrypt_block(c, rk, te0);
    store16(slot + 16 * (size_t)b, c);
  }
  return 16 * (nfull + 1);
}

// The other way, len a positive multiple of 16 (the host's check).  Returns the plaintext's length, or
// -1 for padding EVP_DecryptFinal_ex refuses: the last byte not in 1 .. 16, or the pad bytes not all it.
BM_DEV int32_t cbc_decrypt_row(uint8_t* slot, uint32_t len, const uint32_t (&key)[8], const uint32_t (&iv)[4],
                               const aes::DecTab& l) {
  uint32_t dk[60], prev[4], ct[4], p[4];
  aes::expand_dec_key(dk, key, l);
#pragma unroll
  for (int i = 0; i < 4; ++i) prev[i] = iv[i], p[i] = 0;
  const uint32_t nblk = len / 16;
  for (uint32_t b = 0; b < nblk; ++b) {
    load16(ct, slot + 16 * (size_t)b);
#pragma unroll
    for (int i = 0; i < 4; ++i) p[i] = ct[i];
    aes::decrypt_block(p, dk, l);
#pragma unroll
    for (int i = 0; i < 4; ++i) p[i] ^= prev[i], prev[i] = ct[i];
    store16(slot + 16 * (size_t)b, p);
  }
  const uint32_t pad = p[3] & 0xffu;
  bool good = pad >= 1 && pad <= 16;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const uint32_t byte = (p[k / 4] >> (24 - 8 * (k % 4))) & 0xffu;
    if ((uint32_t)k >= 16u - pad && byte != pad) good = false;
  }
  return good ? (int32_t)(len - pad) : -1;
}

}  // namespace sl
