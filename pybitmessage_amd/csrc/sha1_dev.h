// sha1_dev.h -- gfx950 SHA-1 for the signature verification (bmpow_sig.hip), written from
// FIPS 180-4 (6.1.2, 4.1.1, 4.2.1, 5.3.1).
//
// The reference's verify tries every signature under SHA-1 first (src/highlevelcrypto.py:88-108,
// digest_alg "sha1", then "sha256").  SHA-1 pads as SHA-256 does (64-byte blocks, 0x80, a 64-bit
// big-endian bit length), so one padded block feeds both compressions.  In the style of
// sha256_dev.h: rotates as v_alignbit_b32, Ch / Parity / Maj as one v_bitop3_b32, the 80 rounds
// unrolled with compile-time indices over a 16-word schedule ring.
#pragma once
#include <stdint.h>

#ifndef BM_DEV
#define BM_DEV __device__ __forceinline__
#endif

namespace s1 {

constexpr uint32_t IV(int i) {
  constexpr uint32_t iv[5] = {0x67452301u, 0xefcdab89u, 0x98badcfeu, 0x10325476u, 0xc3d2e1f0u};
  return iv[i];
}

constexpr uint32_t K(int t) { return t < 20 ? 0x5a827999u : t < 40 ? 0x6ed9eba1u : t < 60 ? 0x8f1bbcdcu : 0xca62c1d6u; }

template <int N>
BM_DEV uint32_t rotl(uint32_t x) {
  static_assert(N > 0 && N < 32, "rotate");
  return __builtin_amdgcn_alignbit(x, x, 32 - N);
}

// LUT bits: S0 = 0xF0, S1 = 0xCC, S2 = 0xAA (as sha256_dev.h)
template <int T>
BM_DEV uint32_t f(uint32_t b, uint32_t c, uint32_t d) {
  if constexpr (T < 20) return __builtin_amdgcn_bitop3_b32(b, c, d, 0xCA);                 // Ch
  else if constexpr (T >= 40 && T < 60) return __builtin_amdgcn_bitop3_b32(b, c, d, 0xE8);  // Maj
  else return __builtin_amdgcn_bitop3_b32(b, c, d, 0x96);                                   // Parity
}

// State slot of a at round T is (-T) mod 5: every index is a compile-time constant.
template <int T>
BM_DEV void round_step(uint32_t (&s)[5], uint32_t (&w)[16]) {
  constexpr int A = (5 - (T % 5)) % 5;
  constexpr int B = (A + 1) % 5, C = (A + 2) % 5, D = (A + 3) % 5, E = (A + 4) % 5;
  if constexpr (T >= 16) {
    const uint32_t x = __builtin_amdgcn_bitop3_b32(w[(T - 3) & 15], w[(T - 8) & 15], w[(T - 14) & 15], 0x96) ^ w[T & 15];
    w[T & 15] = rotl<1>(x);
  }
  // T = ROTL5(a) + f(b, c, d) + e + K + W; the new a takes e's slot, b becomes ROTL30(b) in place
  s[E] = rotl<5>(s[A]) + f<T>(s[B], s[C], s[D]) + s[E] + (K(T) + w[T & 15]);
  s[B] = rotl<30>(s[B]);
}

template <int T, int END>
BM_DEV void rounds(uint32_t (&s)[5], uint32_t (&w)[16]) {
  if constexpr (T < END) {
    round_step<T>(s, w);
    rounds<T + 1, END>(s, w);
  }
}

// One compression of the 64-byte block w (big-endian words; clobbered) into the chaining state h.
BM_DEV void compress(uint32_t (&h)[5], uint32_t (&w)[16]) {
  uint32_t s[5];
#pragma unroll
  for (int i = 0; i < 5; ++i) s[i] = h[i];
  rounds<0, 80>(s, w);
#pragma unroll
  for (int i = 0; i < 5; ++i) h[i] += s[i];
}

BM_DEV void init(uint32_t (&h)[5]) {
#pragma unroll
  for (int i = 0; i < 5; ++i) h[i] = IV(i);
}

}  // namespace s1
