// sha256_dev.h -- gfx950 SHA-256 and HMAC-SHA256 for the ECIES MAC check (bmpow_ecies.hip).
//
// The reference authenticates a received blob with hmac_sha256(key_m, data[:-32])
// (src/pyelliptic/ecc.py:498, hash.py) where key_m is the second half of SHA512(shared x): 32 bytes,
// so the HMAC key block is key_m || 32 zero bytes and
//   HMAC = SHA256((K ^ opad) || SHA256((K ^ ipad) || data)).
// In the style of sha512_dev.h: 32-bit words, rotates as v_alignbit_b32, Ch / Maj / XOR3 as one
// v_bitop3_b32, rounds fully unrolled with compile-time indices so state and schedule stay in VGPRs.
#pragma once
#include <stdint.h>

#ifndef BM_DEV
#define BM_DEV __device__ __forceinline__
#endif

namespace s256 {

// FIPS 180-4 4.2.2 / 5.3.3
constexpr uint32_t K(int t) {
  constexpr uint32_t k[64] = {
      0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u,
      0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u,
      0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
      0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u,
      0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
      0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
      0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,
      0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
  return k[t];
}

constexpr uint32_t IV(int i) {
  constexpr uint32_t iv[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au,
                              0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
  return iv[i];
}

template <int N>
BM_DEV uint32_t rotr(uint32_t x) {
  static_assert(N > 0 && N < 32, "rotate");
  return __builtin_amdgcn_alignbit(x, x, N);
}

// LUT bits: S0 = 0xF0, S1 = 0xCC, S2 = 0xAA (as sha512_dev.h)
BM_DEV uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96); }
BM_DEV uint32_t Ch(uint32_t e, uint32_t f, uint32_t g) { return __builtin_amdgcn_bitop3_b32(e, f, g, 0xCA); }
BM_DEV uint32_t Maj(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_bitop3_b32(a, b, c, 0xE8); }
BM_DEV uint32_t Sig0(uint32_t a) { return xor3(rotr<2>(a), rotr<13>(a), rotr<22>(a)); }
BM_DEV uint32_t Sig1(uint32_t e) { return xor3(rotr<6>(e), rotr<11>(e), rotr<25>(e)); }
BM_DEV uint32_t sig0(uint32_t w) { return xor3(rotr<7>(w), rotr<18>(w), w >> 3); }
BM_DEV uint32_t sig1(uint32_t w) { return xor3(rotr<17>(w), rotr<19>(w), w >> 10); }

// State slot of a at round T is (-T) & 7, as in sha512_dev.h: every index is a compile-time constant.
template <int T>
BM_DEV void round_step(uint32_t (&s)[8], uint32_t (&w)[16]) {
  constexpr int A = (8 - (T & 7)) & 7;
  constexpr int B = (A + 1) & 7, C = (A + 2) & 7, D = (A + 3) & 7;
  constexpr int E = (A + 4) & 7, F = (A + 5) & 7, G = (A + 6) & 7, H = (A + 7) & 7;
  if constexpr (T >= 16)
    w[T & 15] = w[(T - 7) & 15] + sig0(w[(T - 15) & 15]) + w[(T - 16) & 15] + sig1(w[(T - 2) & 15]);
  const uint32_t t1 = s[H] + Sig1(s[E]) + Ch(s[E], s[F], s[G]) + (K(T) + w[T & 15]);
  s[D] += t1;
  s[H] = t1 + Sig0(s[A]) + Maj(s[A], s[B], s[C]);
}

template <int T, int END>
BM_DEV void rounds(uint32_t (&s)[8], uint32_t (&w)[16]) {
  if constexpr (T < END) {
    round_step<T>(s, w);
    rounds<T + 1, END>(s, w);
  }
}

// One compression of the 64-byte block w (big-endian words; clobbered) into the chaining state h.
BM_DEV void compress(uint32_t (&h)[8], uint32_t (&w)[16]) {
  uint32_t s[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) s[i] = h[i];
  rounds<0, 64>(s, w);
#pragma unroll
  for (int i = 0; i < 8; ++i) h[i] += s[i];
}

BM_DEV void init(uint32_t (&h)[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) h[i] = IV(i);
}

// The two keyed states of HMAC-SHA256 for a 32-byte key (8 big-endian words): the chaining state after
// the block (K ^ ipad) and after (K ^ opad).
BM_DEV void hmac_key_states(uint32_t (&hi)[8], uint32_t (&ho)[8], const uint32_t (&key)[8]) {
  uint32_t w[16];
#pragma unroll
  for (int i = 0; i < 8; ++i) w[i] = key[i] ^ 0x36363636u;
#pragma unroll
  for (int i = 8; i < 16; ++i) w[i] = 0x36363636u;
  init(hi);
  compress(hi, w);
#pragma unroll
  for (int i = 0; i < 8; ++i) w[i] = key[i] ^ 0x5c5c5c5cu;
#pragma unroll
  for (int i = 8; i < 16; ++i) w[i] = 0x5c5c5c5cu;
  init(ho);
  compress(ho, w);
}

// The outer hash: SHA256 of (K ^ opad) || inner digest, from the keyed outer state ho.  The message is
// 64 + 32 bytes: one more block, inner || 0x80 || zeros || 768 (bits).
BM_DEV void hmac_outer(uint32_t (&ho)[8], const uint32_t (&inner)[8]) {
  uint32_t w[16];
#pragma unroll
  for (int i = 0; i < 8; ++i) w[i] = inner[i];
  w[8] = 0x80000000u;
#pragma unroll
  for (int i = 9; i < 15; ++i) w[i] = 0;
  w[15] = 96 * 8;
  compress(ho, w);
}

// The inner hash's data blocks, pre-padded by the host (bmpow_host_ecies.hip pad_mac_blocks): data ||
// 0x80 || zeros || the bit length of 64 + len(data), so nblk = ceil((len + 9) / 64) and the padding
// depends only on the data length, never on the key.  blocks: nblk * 4 uint4, bytes as they lie in the
// message (each 32-bit lane is byte-swapped into a big-endian word here).  The caller's nblk comes
// from the host-validated length; the lane reads exactly its own nblk blocks.
BM_DEV void hmac_inner(uint32_t (&hi)[8], const uint4* __restrict__ blocks, uint32_t nblk) {
  for (uint32_t b = 0; b < nblk; ++b) {
    uint32_t w[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint4 v = blocks[(size_t)b * 4 + q];
      w[4 * q + 0] = __builtin_bswap32(v.x);
      w[4 * q + 1] = __builtin_bswap32(v.y);
      w[4 * q + 2] = __builtin_bswap32(v.z);
      w[4 * q + 3] = __builtin_bswap32(v.w);
    }
    compress(hi, w);
  }
}

}  // namespace s256
