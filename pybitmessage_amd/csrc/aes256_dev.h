// aes256_dev.h -- gfx950 AES-256 (FIPS-197) for the ECIES seal and the raw CBC call (bmpow_seal.hip).
//
// The reference encrypts a blob's body with pyelliptic's Cipher(key_e, iv, 1, 'aes-256-cbc')
// (src/pyelliptic/ecc.py:474-476, cipher.py) and opens it with the same cipher the other way (:499-501).
// In the style of sha256_dev.h: 32-bit big-endian words, rotates as v_alignbit_b32, rounds unrolled with
// compile-time indices so the state and the 60 round-key words stay in VGPRs.
//
// Tables.  One forward table te0[x] = S[x] . (02, 01, 01, 03) and one inverse table td0[x] =
// Si[x] . (0e, 09, 0d, 0b), 256 words each; the other three columns of each are byte rotations of it
// (Te1 = ror 8, Te2 = ror 16, Te3 = ror 24), one v_alignbit each.  The S-box of the last round and of
// the key schedule is byte 1 of te0[x] (its multiplier is 01); the inverse S-box has no such column and
// is a byte table of its own.  They are generated at compile time from the field arithmetic (no typed-in
// constants beside FIPS-197's polynomial and affine map; static_asserts pin known entries), lie in
// constant memory, and a block copies them into LDS cooperatively at kernel entry (fill_enc / fill_dec).
// Layout: the plain one, entry x at word x.  By the LDS's banking ((a / 4) mod 32 over 32-lane groups)
// random indices conflict about 3-4 ways on it; the conflict-free layout (entry * 32 + lane % 32, 32 KB
// per table) was not taken because the seal kernel is a small part of the call it serves (DESIGN.md,
// send side).  The tables are indexed by secret bytes: not constant-time, see DESIGN.md.
//
// The functions take the tables as pointers, so tests/native/seal_sim.cpp runs the same code on the host.
#pragma once
#include <stdint.h>

#ifndef BM_DEV
#define BM_DEV __device__ __forceinline__
#endif

namespace aes {

constexpr uint8_t xtime(uint8_t a) { return (uint8_t)((a << 1) ^ ((a & 0x80) ? 0x1b : 0)); }
constexpr uint8_t gmul(uint8_t a, uint8_t b) {
  uint8_t r = 0;
  for (int i = 0; i < 8; ++i) {
    if (b & 1) r ^= a;
    a = xtime(a);
    b >>= 1;
  }
  return r;
}
constexpr uint8_t rotl8(uint8_t x, int n) { return (uint8_t)((x << n) | (x >> (8 - n))); }

struct Tables {
  uint32_t te0[256];
  uint32_t td0[256];
  uint8_t si[256];
};

constexpr Tables make_tables() {
  Tables t{};
  uint8_t sb[256] = {};
  // S[x] = affine(x^-1): p runs over the powers of 3, q over those of 3^-1 (FIPS-197 5.1.1)
  uint8_t p = 1, q = 1;
  do {
    p = (uint8_t)(p ^ xtime(p));
    q = gmul(q, 0xf6);  // 3^-1
    sb[p] = (uint8_t)(q ^ rotl8(q, 1) ^ rotl8(q, 2) ^ rotl8(q, 3) ^ rotl8(q, 4) ^ 0x63);
  } while (p != 1);
  sb[0] = 0x63;
  for (int x = 0; x < 256; ++x) {
    const uint8_t s = sb[x];
    t.te0[x] = (uint32_t)xtime(s) << 24 | (uint32_t)s << 16 | (uint32_t)s << 8 | (uint8_t)(xtime(s) ^ s);
    t.si[s] = (uint8_t)x;
  }
  for (int x = 0; x < 256; ++x) {
    const uint8_t s = t.si[x];
    t.td0[x] = (uint32_t)gmul(s, 14) << 24 | (uint32_t)gmul(s, 9) << 16 | (uint32_t)gmul(s, 13) << 8 | gmul(s, 11);
  }
  return t;
}

inline constexpr Tables kTables = make_tables();
// FIPS-197 figure 7 / 14 and the first entries of the usual Te0 / Td0
static_assert(kTables.te0[0x00] == 0xc66363a5u && kTables.te0[0x01] == 0xf87c7c84u && kTables.te0[0xff] == 0x2c16163au, "Te0");
static_assert(kTables.td0[0x00] == 0x51f4a750u && kTables.td0[0x01] == 0x7e416553u, "Td0");
static_assert(kTables.si[0x00] == 0x52 && kTables.si[0x63] == 0x00 && kTables.si[0xff] == 0x7d, "inverse S-box");

struct EncTab {  // what encryption and the key schedule read
  uint32_t te0[256];
};
struct DecTab {  // decryption: the key schedule's S-box comes from te0
  uint32_t te0[256];
  uint32_t td0[256];
  uint8_t si[256];
};

// Thread tid of nthr copies its share; the caller synchronises the block afterwards.
BM_DEV void fill_enc(EncTab& l, uint32_t tid, uint32_t nthr) {
  static constexpr Tables t = make_tables();
  for (uint32_t i = tid; i < 256; i += nthr) l.te0[i] = t.te0[i];
}
BM_DEV void fill_dec(DecTab& l, uint32_t tid, uint32_t nthr) {
  static constexpr Tables t = make_tables();
  for (uint32_t i = tid; i < 256; i += nthr) {
    l.te0[i] = t.te0[i];
    l.td0[i] = t.td0[i];
    l.si[i] = t.si[i];
  }
}

template <int N>
BM_DEV uint32_t ror(uint32_t x) {
  static_assert(N > 0 && N < 32, "rotate");
#if defined(__AMDGCN__)
  return __builtin_amdgcn_alignbit(x, x, N);
#else
  return (x >> N) | (x << (32 - N));
#endif
}

BM_DEV uint32_t b3(uint32_t w) { return w >> 24; }
BM_DEV uint32_t b2(uint32_t w) { return (w >> 16) & 0xffu; }
BM_DEV uint32_t b1(uint32_t w) { return (w >> 8) & 0xffu; }
BM_DEV uint32_t b0(uint32_t w) { return w & 0xffu; }

// S[a] S[b] S[c] S[d] as one word (a the top byte), from te0's 01 columns
BM_DEV uint32_t sbox4(const uint32_t* te0, uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
  return ((te0[a] & 0x00ff0000u) << 8) | (te0[b] & 0x00ff0000u) | (te0[c] & 0x0000ff00u) | ((te0[d] >> 8) & 0xffu);
}

constexpr uint32_t rcon(int i) { return i <= 8 ? 1u << (i - 1) : (i == 9 ? 0x1bu : 0x36u); }

// FIPS-197 5.2 with Nk = 8: rk[0..8) is the key as big-endian words, rk[8..60) follows.
template <int I>
BM_DEV void expand_from(uint32_t (&rk)[60], const uint32_t* te0) {
  if constexpr (I < 60) {
    uint32_t t = rk[I - 1];
    if constexpr (I % 8 == 0) {
      t = ror<24>(t);  // RotWord
      t = sbox4(te0, b3(t), b2(t), b1(t), b0(t)) ^ (rcon(I / 8) << 24);
    } else if constexpr (I % 8 == 4) {
      t = sbox4(te0, b3(t), b2(t), b1(t), b0(t));
    }
    rk[I] = rk[I - 8] ^ t;
    expand_from<I + 1>(rk, te0);
  }
}

BM_DEV void expand_key(uint32_t (&rk)[60], const uint32_t (&key)[8], const uint32_t* te0) {
#pragma unroll
  for (int i = 0; i < 8; ++i) rk[i] = key[i];
  expand_from<8>(rk, te0);
}

// InvMixColumns of one word: td0 of the S-box of each byte (td0[S[x]] = x . (0e, 09, 0d, 0b))
BM_DEV uint32_t inv_mix(uint32_t w, const uint32_t* te0, const uint32_t* td0) {
  const uint32_t a = (te0[b3(w)] >> 8) & 0xffu, b = (te0[b2(w)] >> 8) & 0xffu;
  const uint32_t c = (te0[b1(w)] >> 8) & 0xffu, d = (te0[b0(w)] >> 8) & 0xffu;
  return td0[a] ^ ror<8>(td0[b]) ^ ror<16>(td0[c]) ^ ror<24>(td0[d]);
}

// The equivalent inverse cipher's keys (FIPS-197 5.3.5): the rounds in reverse order, InvMixColumns on
// rounds 1..13.
template <int R>
BM_DEV void dec_keys_from(uint32_t (&dk)[60], const uint32_t (&ek)[60], const uint32_t* te0, const uint32_t* td0) {
  if constexpr (R <= 14) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if constexpr (R == 0 || R == 14) dk[4 * R + i] = ek[4 * (14 - R) + i];
      else dk[4 * R + i] = inv_mix(ek[4 * (14 - R) + i], te0, td0);
    }
    dec_keys_from<R + 1>(dk, ek, te0, td0);
  }
}

BM_DEV void expand_dec_key(uint32_t (&dk)[60], const uint32_t (&key)[8], const DecTab& l) {
  uint32_t ek[60];
  expand_key(ek, key, l.te0);
  dec_keys_from<0>(dk, ek, l.te0, l.td0);
}

template <int R>
BM_DEV void enc_rounds(uint32_t (&s)[4], const uint32_t (&rk)[60], const uint32_t* te0) {
  if constexpr (R < 14) {
    const uint32_t t0 = te0[b3(s[0])] ^ ror<8>(te0[b2(s[1])]) ^ ror<16>(te0[b1(s[2])]) ^ ror<24>(te0[b0(s[3])]) ^ rk[4 * R];
    const uint32_t t1 = te0[b3(s[1])] ^ ror<8>(te0[b2(s[2])]) ^ ror<16>(te0[b1(s[3])]) ^ ror<24>(te0[b0(s[0])]) ^ rk[4 * R + 1];
    const uint32_t t2 = te0[b3(s[2])] ^ ror<8>(te0[b2(s[3])]) ^ ror<16>(te0[b1(s[0])]) ^ ror<24>(te0[b0(s[1])]) ^ rk[4 * R + 2];
    const uint32_t t3 = te0[b3(s[3])] ^ ror<8>(te0[b2(s[0])]) ^ ror<16>(te0[b1(s[1])]) ^ ror<24>(te0[b0(s[2])]) ^ rk[4 * R + 3];
    s[0] = t0, s[1] = t1, s[2] = t2, s[3] = t3;
    enc_rounds<R + 1>(s, rk, te0);
  }
}

// One block, in place: s = the 16 bytes as four big-endian words.
BM_DEV void encrypt_block(uint32_t (&s)[4], const uint32_t (&rk)[60], const uint32_t* te0) {
#pragma unroll
  for (int i = 0; i < 4; ++i) s[i] ^= rk[i];
  enc_rounds<1>(s, rk, te0);
  const uint32_t t0 = sbox4(te0, b3(s[0]), b2(s[1]), b1(s[2]), b0(s[3])) ^ rk[56];
  const uint32_t t1 = sbox4(te0, b3(s[1]), b2(s[2]), b1(s[3]), b0(s[0])) ^ rk[57];
  const uint32_t t2 = sbox4(te0, b3(s[2]), b2(s[3]), b1(s[0]), b0(s[1])) ^ rk[58];
  const uint32_t t3 = sbox4(te0, b3(s[3]), b2(s[0]), b1(s[1]), b0(s[2])) ^ rk[59];
  s[0] = t0, s[1] = t1, s[2] = t2, s[3] = t3;
}

template <int R>
BM_DEV void dec_rounds(uint32_t (&s)[4], const uint32_t (&dk)[60], const uint32_t* td0) {
  if constexpr (R < 14) {
    const uint32_t t0 = td0[b3(s[0])] ^ ror<8>(td0[b2(s[3])]) ^ ror<16>(td0[b1(s[2])]) ^ ror<24>(td0[b0(s[1])]) ^ dk[4 * R];
    const uint32_t t1 = td0[b3(s[1])] ^ ror<8>(td0[b2(s[0])]) ^ ror<16>(td0[b1(s[3])]) ^ ror<24>(td0[b0(s[2])]) ^ dk[4 * R + 1];
    const uint32_t t2 = td0[b3(s[2])] ^ ror<8>(td0[b2(s[1])]) ^ ror<16>(td0[b1(s[0])]) ^ ror<24>(td0[b0(s[3])]) ^ dk[4 * R + 2];
    const uint32_t t3 = td0[b3(s[3])] ^ ror<8>(td0[b2(s[2])]) ^ ror<16>(td0[b1(s[1])]) ^ ror<24>(td0[b0(s[0])]) ^ dk[4 * R + 3];
    s[0] = t0, s[1] = t1, s[2] = t2, s[3] = t3;
    dec_rounds<R + 1>(s, dk, td0);
  }
}

BM_DEV uint32_t isbox4(const uint8_t* si, uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
  return (uint32_t)si[a] << 24 | (uint32_t)si[b] << 16 | (uint32_t)si[c] << 8 | si[d];
}

// One block, in place, with expand_dec_key's keys.
BM_DEV void decrypt_block(uint32_t (&s)[4], const uint32_t (&dk)[60], const DecTab& l) {
#pragma unroll
  for (int i = 0; i < 4; ++i) s[i] ^= dk[i];
  dec_rounds<1>(s, dk, l.td0);
  const uint32_t t0 = isbox4(l.si, b3(s[0]), b2(s[3]), b1(s[2]), b0(s[1])) ^ dk[56];
  const uint32_t t1 = isbox4(l.si, b3(s[1]), b2(s[0]), b1(s[3]), b0(s[2])) ^ dk[57];
  const uint32_t t2 = isbox4(l.si, b3(s[2]), b2(s[1]), b1(s[0]), b0(s[3])) ^ dk[58];
  const uint32_t t3 = isbox4(l.si, b3(s[3]), b2(s[2]), b1(s[1]), b0(s[0])) ^ dk[59];
  s[0] = t0, s[1] = t1, s[2] = t2, s[3] = t3;
}

}  // namespace aes
