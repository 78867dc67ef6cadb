// secp256k1_var_dev.h -- variable-base scalar multiplication on secp256k1 for the ECIES trial
// decryption (bmpow_ecies.hip), on top of the field and group arithmetic of secp256k1_dev.h.
//
// The reference tries a received msg against a private key k with ECDH_compute_key
// (src/pyelliptic/ecc.py:243): x(k R) for the message's ephemeral point R.  Here one lane holds one
// object's R and computes x(k R) for the key of its wave:
//   * per object, once (var_table): the odd multiples R, 3R, ..., 15R in affine coordinates, laid out
//     [entry][object] so a wave's loads of one entry are contiguous, reused by every key;
//   * per key, once, on the host (bmpow_host_ecies.hip recode_key): k made odd (x(k R) = x((n - k) R),
//     and n is odd), then recoded into 64 signed odd digits d_i in {+-1, ..., +-15},
//     k = sum d_i 16^i (regular recoding: every window adds, none is skipped);
//   * per pair (var_mult_x): acc = d_63 R, then 63 times acc = 16 acc + d_i R -- 252 doublings and 63
//     mixed additions (about 2,450 field multiplications) and one inversion for x = X / Z^2.
// With one key per wave the digits are wave-uniform; the ladder itself is branch-free in the digit
// (the entry is an address, the sign a select), so a per-lane digit string runs the same code
// (bmpow_ecdh).  The additions take gej_add_ge's complete path: an accumulator equal to plus or minus
// the table entry doubles or goes to infinity as it must.
#pragma once
#include "secp256k1_dev.h"

namespace ec {

constexpr int kVarEntries = 8;   // R, 3R, ..., 15R
constexpr int kVarDigits = 64;   // signed odd base-16 digits of a 256-bit odd scalar

// r = -a (weakly reduced a: 0 - a borrows and adds p back, fe_sub)
BM_DEV void fe_neg(fe& r, const fe& a) {
  fe z;
  fe_set(z, 0);
  fe_sub(r, z, a);
}

// y^2 = x^3 + 7 for canonical or weakly reduced x, y
BM_DEV bool ge_on_curve(const ge& p) {
  fe l, r, t;
  fe_sqr(l, p.y);
  fe_sqr(r, p.x);
  fe_mul(r, r, p.x);
  fe_set(t, 7);
  fe_add(r, r, t);
  fe_sub(t, l, r);
  return fe_is_zero(t);
}

// The generator: what a lane works on when its object's point is not on the curve, so every lane's
// arithmetic is defined (the object is reported through its ok flag and never matched).
BM_DEV void ge_set_generator(ge& g) {
  constexpr uint32_t gx[8] = {0x16F81798u, 0x59F2815Bu, 0x2DCE28D9u, 0x029BFCDBu,
                              0xCE870B07u, 0x55A06295u, 0xF9DCBBACu, 0x79BE667Eu};
  constexpr uint32_t gy[8] = {0xFB10D4B8u, 0x9C47D08Fu, 0xA6855419u, 0xFD17B448u,
                              0x0E1108A8u, 0x5DA4FBFCu, 0x26A3C465u, 0x483ADA77u};
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    g.x.d[i] = gx[i];
    g.y.d[i] = gy[i];
  }
}

// tab[e * stride + o] = (2e + 1) R in affine coordinates (weakly reduced), e < kVarEntries, for the
// on-curve point R of object o.
//
// 2R = (X2, Y2, C) in Jacobian coordinates.  On the isomorphic curve phi(x, y) = (C^2 x, C^3 y) the
// point 2R is the AFFINE point (X2, Y2) (the addition formulas of a = 0 never use b), so the chain
// R + 2R + 2R + ... runs as seven mixed additions there, and a point (X, Y, Z) of it is (X, Y, C Z) on
// the curve itself.  One inversion (of the product of the eight C Z_e) then makes all entries affine.
// R has the group's prime order n, so no two of R, 2R, ..., 15R meet or cancel and R has no point of
// order 2 under it: the chain never reaches the additions' special cases.
BM_DEV void var_table(ge* __restrict__ tab, size_t stride, size_t o, const ge& R) {
  gej a, d;
  a.x = R.x;
  a.y = R.y;
  fe_set(a.z, 1);
  a.inf = false;
  gej_double(d, a);
  const fe C = d.z;
  fe c2, c3;
  fe_sqr(c2, C);
  fe_mul(c3, c2, C);
  ge q2;
  q2.x = d.x;
  q2.y = d.y;
  fe_mul(a.x, R.x, c2);
  fe_mul(a.y, R.y, c3);
  fe zt[kVarEntries], pre[kVarEntries];  // C Z_e and their running products
  zt[0] = C;
  pre[0] = C;
  tab[o] = ge{a.x, a.y};  // Jacobian X, Y for now; made affine below
#pragma unroll 1
  for (int e = 1; e < kVarEntries; ++e) {
    gej_add_ge(a, a, q2);
    tab[(size_t)e * stride + o] = ge{a.x, a.y};
    fe_mul(zt[e], a.z, C);
    fe_mul(pre[e], pre[e - 1], zt[e]);
  }
  fe inv;
  fe_inv(inv, pre[kVarEntries - 1]);
#pragma unroll 1
  for (int e = kVarEntries - 1; e >= 0; --e) {
    fe zi = inv;  // (C Z_0 ... C Z_e)^-1
    if (e > 0) {
      fe_mul(zi, inv, pre[e - 1]);
      fe_mul(inv, inv, zt[e]);
    }
    fe zi2, zi3;
    fe_sqr(zi2, zi);
    fe_mul(zi3, zi2, zi);
    ge j = tab[(size_t)e * stride + o], r;
    fe_mul(r.x, j.x, zi2);
    fe_mul(r.y, j.y, zi3);
    tab[(size_t)e * stride + o] = r;
  }
}

// The table entry of digit d (odd, |d| <= 15), negated for d < 0.
BM_DEV void var_entry(ge& q, const ge* __restrict__ tab, size_t stride, size_t o, int d) {
  const int m = d < 0 ? -d : d;
  q = tab[(size_t)((m - 1) >> 1) * stride + o];
  fe ny;
  fe_neg(ny, q.y);
#pragma unroll
  for (int i = 0; i < 8; ++i) q.y.d[i] = d < 0 ? ny.d[i] : q.y.d[i];
}

// k R in Jacobian coordinates for the digit string dig[0], dig[dstride], ..., 64 digits of k (least
// significant first; int32 or int8 each), and object o's table.
template <class D>
BM_DEV void var_mult_jac(gej& acc, const ge* __restrict__ tab, size_t stride, size_t o, const D* __restrict__ dig,
                         size_t dstride) {
  ge q;
  var_entry(q, tab, stride, o, dig[(kVarDigits - 1) * dstride]);
  acc.x = q.x;
  acc.y = q.y;
  fe_set(acc.z, 1);
  acc.inf = false;
#pragma unroll 1
  for (int i = kVarDigits - 2; i >= 0; --i) {
    var_entry(q, tab, stride, o, dig[i * dstride]);  // issued ahead of the four doublings that hide its latency
#pragma unroll 1
    for (int j = 0; j < 4; ++j) gej_double(acc, acc);
    gej_add_ge(acc, acc, q);
  }
}

// x(k R), canonical, for the digit string dig[0 .. 64) of k (least significant first) and object o's
// table; false when k R is the point at infinity (no scalar in [1, n) gives it).
BM_DEV bool var_mult_x(fe& x, const ge* __restrict__ tab, size_t stride, size_t o, const int32_t* __restrict__ dig) {
  gej acc;
  var_mult_jac(acc, tab, stride, o, dig, 1);
  if (acc.inf) {
    fe_set(x, 0);
    return false;
  }
  fe zi;
  fe_inv(zi, acc.z);
  fe_sqr(zi, zi);
  fe_mul(x, acc.x, zi);
  fe_normalize(x, x);
  return true;
}

}  // namespace ec
