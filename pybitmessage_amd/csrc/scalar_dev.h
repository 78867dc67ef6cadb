// scalar_dev.h -- arithmetic modulo the group order n of secp256k1 for the signature verification
// (bmpow_sig.hip): the scalars of the ECDSA equation, w = s^-1, u1 = e w, u2 = r w (mod n), and the
// recoding of u2 into the signed odd digits of the variable-base ladder (secp256k1_var_dev.h).
//
// A scalar is 8 little-endian 32-bit limbs.  Products are 8 x 8 limbs by operand scanning
// (a 32 x 32 product plus two 32-bit addends never leaves 64 bits); the 512-bit product folds back by
// 2^256 = c (mod n), c = 2^256 - n = 0x1_45512319_50B75FC4_402DA173_2FC9BEBF (129 bits): three
// folds (512 -> 386 -> 260 -> 257 bits), a last one for the carry bit and one conditional
// subtraction leave the canonical residue.  Inputs may be any value below 2^256 (a digest is not
// reduced before it is used); every result is below n.
//
// The inversion is Fermat's a^(n-2).  n - 2 is 127 one bits, a zero, and the 128 bits
// 0xBAAEDCE6AF48A03BBFD25E8CD036413F: a^(2^127 - 1) by an addition chain (126 squarings, 10 products),
// then square-and-multiply over the low half, whose bits are the same for every lane (no divergence):
// 255 squarings and 79 products in all (a squaring is a product here), in rolled loops.
//
// Plain C++ (uint32 / uint64 only), as modinv_dev.h: the same source compiles for gfx950 and for the
// host, where tests/test_sig.py checks it against Python integers.
#pragma once
#include <stdint.h>

// host and device: the host unit (bmpow_host_sig.hip) range-checks r and s with the same code
#if defined(__HIPCC__)
#define SN_HD __host__ __device__ __forceinline__
#else
#define SN_HD static inline
#endif

namespace sn {

struct sc {
  uint32_t d[8];
};

constexpr uint32_t N(int i) {
  constexpr uint32_t n[8] = {0xD0364141u, 0xBFD25E8Cu, 0xAF48A03Bu, 0xBAAEDCE6u,
                             0xFFFFFFFEu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
  return n[i];
}

// 2^256 - n, 5 limbs
constexpr uint32_t C(int i) {
  constexpr uint32_t c[5] = {0x2FC9BEBFu, 0x402DA173u, 0x50B75FC4u, 0x45512319u, 1u};
  return c[i];
}

// the low 128 bits of n - 2
constexpr uint32_t ELOW(int i) {
  constexpr uint32_t e[4] = {0xD036413Fu, 0xBFD25E8Cu, 0xAF48A03Bu, 0xBAAEDCE6u};
  return e[i];
}

SN_HD void set(sc& r, uint32_t v) {
  r.d[0] = v;
#pragma unroll
  for (int i = 1; i < 8; ++i) r.d[i] = 0;
}

SN_HD bool is_zero(const sc& a) {
  uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) o |= a.d[i];
  return o == 0;
}

// r = a - n and true when a >= n; r = a and false otherwise (a < 2^256)
SN_HD bool cond_sub_n(sc& r, const sc& a) {
  uint32_t u[8];
  uint64_t bw = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint64_t t = (uint64_t)a.d[i] - N(i) - bw;
    u[i] = (uint32_t)t;
    bw = (t >> 32) & 1u;
  }
  const bool ge_n = bw == 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) r.d[i] = ge_n ? u[i] : a.d[i];
  return ge_n;
}

// r = n - a for 0 < a < n
SN_HD void neg(sc& r, const sc& a) {
  uint64_t bw = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint64_t t = (uint64_t)N(i) - a.d[i] - bw;
    r.d[i] = (uint32_t)t;
    bw = (t >> 32) & 1u;
  }
}

// r = a + b mod n for a, b < n
SN_HD void add(sc& r, const sc& a, const sc& b) {
  uint32_t t[8], u[8];
  uint64_t c = 0, bw = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    c += (uint64_t)a.d[i] + b.d[i];
    t[i] = (uint32_t)c;
    c >>= 32;
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint64_t v = (uint64_t)t[i] - N(i) - bw;
    u[i] = (uint32_t)v;
    bw = (v >> 32) & 1u;
  }
  // a + b < 2 n < 2^257: with a carry out of 256 bits the sum is above n and t - n wraps to it
  const bool sub = c != 0 || bw == 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) r.d[i] = sub ? u[i] : t[i];
}

// o[0 .. ON) = lo[0 .. 8) + hi[0 .. HN) * c; the caller's bound on the value fits ON limbs
template <int HN, int ON>
SN_HD void fold(uint32_t (&o)[ON], const uint32_t* lo, const uint32_t* hi) {
#pragma unroll
  for (int i = 0; i < ON; ++i) o[i] = i < 8 ? lo[i] : 0u;
#pragma unroll
  for (int i = 0; i < HN; ++i) {
    uint64_t carry = 0;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      if (i + j < ON) {
        const uint64_t t = (uint64_t)hi[i] * C(j) + o[i + j] + carry;
        o[i + j] = (uint32_t)t;
        carry = t >> 32;
      }
    }
#pragma unroll
    for (int k = i + 5; k < ON; ++k) {
      const uint64_t t = (uint64_t)o[k] + carry;
      o[k] = (uint32_t)t;
      carry = t >> 32;
    }
  }
}

// r = p mod n for a 512-bit p (16 limbs)
SN_HD void reduce512(sc& r, const uint32_t (&p)[16]) {
  uint32_t t1[13], t2[9], t3[9], t4[9];
  fold<8, 13>(t1, p, p + 8);     // < 2^256 + 2^256 c < 2^386
  fold<5, 9>(t2, t1, t1 + 8);    // the high part is < 2^130: < 2^256 + 2^259
  fold<1, 9>(t3, t2, t2 + 8);    // the high part is < 16: < 2^256 + 2^133, so t3[8] is 0 or 1
  fold<1, 9>(t4, t3, t3 + 8);    // and when it is 1 the rest is < 2^133: no carry now
  sc v;
#pragma unroll
  for (int i = 0; i < 8; ++i) v.d[i] = t4[i];
  cond_sub_n(r, v);  // v < 2^256 < 2 n
}

// r = a b mod n (a, b < 2^256)
SN_HD void mul(sc& r, const sc& a, const sc& b) {
  uint32_t p[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) p[i] = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    uint64_t carry = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint64_t t = (uint64_t)a.d[i] * b.d[j] + p[i + j] + carry;
      p[i + j] = (uint32_t)t;
      carry = t >> 32;
    }
    p[i + 8] = (uint32_t)carry;
  }
  reduce512(r, p);
}

// r = a^(2^k) b
SN_HD void sqr_n_mul(sc& r, const sc& a, int k, const sc& b) {
  sc t = a;
#pragma unroll 1
  for (int i = 0; i < k; ++i) mul(t, t, t);
  mul(r, t, b);
}

// r = a^-1 mod n (a = 0 mod n gives 0)
SN_HD void inv(sc& r, const sc& a) {
  sc x1, x2, x3, x6, x12, x24, x48, x96, t, one;
  // x_k = a^(2^k - 1); x1 = a mod n
  set(one, 1);
  mul(x1, a, one);
  sqr_n_mul(x2, x1, 1, x1);
  sqr_n_mul(x3, x2, 1, x1);
  sqr_n_mul(x6, x3, 3, x3);
  sqr_n_mul(x12, x6, 6, x6);
  sqr_n_mul(x24, x12, 12, x12);
  sqr_n_mul(x48, x24, 24, x24);
  sqr_n_mul(x96, x48, 48, x48);
  sqr_n_mul(t, x96, 24, x24);  // x120
  sqr_n_mul(t, t, 6, x6);      // x126
  sqr_n_mul(t, t, 1, x1);      // x127
  mul(t, t, t);                // the zero bit 128
#pragma unroll 1
  for (int i = 127; i >= 0; --i) {
    mul(t, t, t);
    if ((ELOW(i >> 5) >> (i & 31)) & 1u) mul(t, t, x1);
  }
  r = t;
}

// The ladder's digits of an ODD k < 2^256: k = sum d_i 16^i over 64 odd digits |d_i| <= 15.  The
// regular recoding d_i = (k mod 32) - 16, k <- (k - d_i) / 16 (bmpow_host_ecies.hip recode_key) never
// carries: k - d_i clears the low five bits and sets bit 4, so the next k is (k >> 4) | 1 and digit i
// reads bits [4 i, 4 i + 5) of the scalar alone; the last digit is what is left, (k >> 252) | 1.
SN_HD int recode_digit(const sc& k, int i) {
  const int b = 4 * i, w = b >> 5, s = b & 31;
  uint32_t v = k.d[w] >> s;
  if (s > 27 && w + 1 < 8) v |= k.d[w + 1] << (32 - s);
  if (i == 63) return (int)((v & 15u) | 1u);
  return (int)((v & 31u) | 1u) - 16;
}

// u made odd for the ladder: u itself, or n - u (flip = true) when u is even; 0 < u < n
SN_HD bool make_odd(sc& r, const sc& u) {
  sc m;
  neg(m, u);
  const bool flip = (u.d[0] & 1u) == 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) r.d[i] = flip ? m.d[i] : u.d[i];
  return flip;
}

}  // namespace sn
