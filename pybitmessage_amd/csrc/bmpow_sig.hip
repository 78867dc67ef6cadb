// bmpow_sig.hip -- batched ECDSA signature verification of received objects (gfx950).
//
// Reference: highlevelcrypto.verify (src/highlevelcrypto.py:88-108) checks every received v3 / v4
// pubkey, every decrypted msg and every broadcast with pyelliptic.ECC.verify
// (src/pyelliptic/ecc.py:387-440), first under SHA-1 and then, unless that passed, under SHA-256: for
// the key Q, the signature (r, s) and the digest e
//     w = s^-1,  u1 = e w,  u2 = r w  (mod n),  R = u1 G + u2 Q,  valid iff R != inf and x(R) mod n = r.
// Both tries share u2 Q, the expensive half.  Host side: bmpow_host_sig.hip.
//
// One lane per signature, the phases as separate kernels so that no phase's register allocation
// carries another's state (as bmpow_ecies.hip keeps its ladder apart from its MAC):
//   sg_hash_kernel   : SHA-1 and SHA-256 of the message, each host-padded block read once;
//   sg_scalar_kernel : w, u1 (per digest), u2 and u2's signed odd digits (scalar_dev.h);
//   ec_prep_kernel   : (bmpow_ecies.hip) the on-curve check and the table Q, 3Q, ..., 15Q;
//   sg_ladder_kernel : T = u2 Q by the signed-window ladder, left in Jacobian coordinates;
//   sg_comb_kernel   : R = T + u1 G by 16 mixed additions of 16-bit-comb entries, per digest, and the
//                      test X = r Z^2 or (r + n) Z^2 -- no inversion mod p anywhere.
// The inputs are attacker-chosen: every addition takes gej_add_ge's complete path (doubling and
// cancellation included).  Every loop bound comes from a host-validated length, a lane reads exactly
// its own nblk blocks of the pool, and lanes past n do nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bmpow_sig_kernels.h"
#include "secp256k1_var_dev.h"
#include "sha1_dev.h"
#include "sha256_dev.h"

using ec::fe;
using ec::ge;
using ec::gej;
using sn::sc;

static_assert(SG_DIGITS == ec::kVarDigits, "digit layout");

__global__ __launch_bounds__(SG_BLOCK) void sg_hash_kernel(const sg_sig* __restrict__ sigs,
                                                           const uint4* __restrict__ pool, uint32_t n, uint32_t stride,
                                                           sc* __restrict__ e) {
  const uint32_t o = blockIdx.x * SG_BLOCK + threadIdx.x;
  if (o >= n) return;
  const uint32_t blk = sigs[o].blk, nblk = sigs[o].nblk;
  const uint4* __restrict__ blocks = pool + (size_t)blk * 4;
  uint32_t h1[5], h2[8];
  s1::init(h1);
  s256::init(h2);
  for (uint32_t b = 0; b < nblk; ++b) {
    uint32_t w[16], v[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint4 x = blocks[(size_t)b * 4 + q];
      w[4 * q + 0] = __builtin_bswap32(x.x);
      w[4 * q + 1] = __builtin_bswap32(x.y);
      w[4 * q + 2] = __builtin_bswap32(x.z);
      w[4 * q + 3] = __builtin_bswap32(x.w);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = w[i];
    s1::compress(h1, v);
    s256::compress(h2, w);
  }
  // the digests as integers: the first word is the most significant; SHA-1's 160 bits zero-extended
  sc e1, e2;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    e1.d[i] = i < 5 ? h1[4 - i] : 0u;
    e2.d[i] = h2[7 - i];
  }
  e[o] = e1;
  e[(size_t)stride + o] = e2;
}

__global__ __launch_bounds__(SG_BLOCK) void sg_scalar_kernel(const sg_sig* __restrict__ sigs, const sc* __restrict__ e,
                                                             uint32_t n, uint32_t stride, int nhash,
                                                             sg_kw* __restrict__ u1, int8_t* __restrict__ dig,
                                                             uint8_t* __restrict__ flip) {
  const uint32_t o = blockIdx.x * SG_BLOCK + threadIdx.x;
  if (o >= n) return;
  sc w, u2, k;
  sn::inv(w, sigs[o].s);
  sn::mul(u2, sigs[o].r, w);  // 1 <= r, s < n and n is prime: never 0
  flip[o] = sn::make_odd(k, u2) ? 1 : 0;
#pragma unroll
  for (int i = 0; i < SG_DIGITS; ++i) dig[(size_t)i * stride + o] = (int8_t)sn::recode_digit(k, i);
#pragma unroll 1
  for (int h = 0; h < nhash; ++h) {
    sc u;
    sn::mul(u, e[(size_t)h * stride + o], w);
    sg_kw kw;
#pragma unroll
    for (int j = 0; j < 4; ++j) kw.w[j] = ((uint64_t)u.d[7 - 2 * j] << 32) | u.d[6 - 2 * j];
    u1[(size_t)h * stride + o] = kw;
  }
}

__global__ __launch_bounds__(SG_BLOCK) void sg_ladder_kernel(const ge* __restrict__ tab, uint32_t n, uint32_t stride,
                                                             const int8_t* __restrict__ dig,
                                                             const uint8_t* __restrict__ flip, sg_pt* __restrict__ T,
                                                             uint8_t* __restrict__ tinf) {
  const uint32_t o = blockIdx.x * SG_BLOCK + threadIdx.x;
  if (o >= n) return;
  gej acc;
  ec::var_mult_jac(acc, tab, stride, o, dig + o, stride);
  // the digits were those of n - u2 when u2 is even: u2 Q = -((n - u2) Q).  Unlike the x-only ECDH
  // the sign matters here.
  fe ny;
  ec::fe_neg(ny, acc.y);
  const bool f = flip[o] != 0;
  sg_pt t;
  t.x = acc.x;
  t.z = acc.z;
#pragma unroll
  for (int i = 0; i < 8; ++i) t.y.d[i] = f ? ny.d[i] : acc.y.d[i];
  T[o] = t;
  tinf[o] = acc.inf ? 1 : 0;
}

// acc += k G for the scalar kw (4 big-endian words), by the 16-bit comb: a zero window is skipped, every
// other one is a complete addition
BM_DEV void comb_add(gej& acc, const ge* __restrict__ table, const sg_kw& kw) {
  using C = ec::comb<ec::kCombSmall>;
  uint64_t s[4] = {kw.w[3], kw.w[2], kw.w[1], kw.w[0]};
#pragma unroll 1
  for (int i = 0; i < C::kWindows; ++i) {
    const uint32_t v = (uint32_t)s[0] & C::kMask;
    ec::shr256_window<ec::kCombSmall>(s);
    if (v) {
      const ge q = table[((size_t)i << ec::kCombSmall) | v];
      ec::gej_add_ge(acc, acc, q);
    }
  }
}

// x(R) mod n == r without an inversion: x(R) = X / Z^2 is r, or r + n when that is still below p
BM_DEV bool x_is_r(const gej& R, const fe& r, const fe& rn, bool has_rn) {
  if (R.inf) return false;
  fe z2, t, d;
  ec::fe_sqr(z2, R.z);
  ec::fe_mul(t, r, z2);
  ec::fe_sub(d, R.x, t);
  if (ec::fe_is_zero(d)) return true;
  ec::fe_mul(t, rn, z2);
  ec::fe_sub(d, R.x, t);
  return has_rn && ec::fe_is_zero(d);
}

__global__ __launch_bounds__(SG_BLOCK) void sg_comb_kernel(const ge* __restrict__ table, const sg_sig* __restrict__ sigs,
                                                           const sg_kw* __restrict__ u1, const sg_pt* __restrict__ T,
                                                           const uint8_t* __restrict__ tinf,
                                                           const uint32_t* __restrict__ ok, uint32_t n, uint32_t stride,
                                                           int nhash, uint8_t* __restrict__ verdict) {
  const uint32_t o = blockIdx.x * SG_BLOCK + threadIdx.x;
  if (o >= n) return;
  // r and r + n as field elements; r + n counts only when it is below p (p - n is about 2^128.4)
  fe r, rn;
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    r.d[i] = sigs[o].r.d[i];
    c += (uint64_t)r.d[i] + sn::N(i);
    rn.d[i] = (uint32_t)c;
    c >>= 32;
  }
  fe rnn;
  ec::fe_normalize(rnn, rn);
  uint32_t same = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) same |= rnn.d[i] ^ rn.d[i];
  const bool has_rn = c == 0 && same == 0;  // no carry out of 256 bits and already canonical: r + n < p
  uint8_t v = 0;
#pragma unroll 1
  for (int h = 0; h < nhash && v == 0; ++h) {
    const sg_pt t = T[o];
    gej acc;
    acc.x = t.x;
    acc.y = t.y;
    acc.z = t.z;
    acc.inf = tinf[o] != 0;
    comb_add(acc, table, u1[(size_t)h * stride + o]);
    if (x_is_r(acc, r, rn, has_rn)) v = (uint8_t)(h + 1);
  }
  verdict[o] = ok[o] ? v : 0;
}

// ---------------------------------------------------------------------------------------
// Launch wrappers (C++ linkage, used by bmpow_host_sig.hip).  stride is a multiple of SG_BLOCK.
// ---------------------------------------------------------------------------------------
static bool sg_shape_ok(uint32_t n, uint32_t stride, int nhash) {
  return n <= stride && stride % SG_BLOCK == 0 && (nhash == 1 || nhash == 2);
}

hipError_t sg_launch_hash(hipStream_t st, const sg_sig* sigs, const uint4* pool, uint32_t n, uint32_t stride, sc* e) {
  if (n == 0) return hipSuccess;
  if (!sg_shape_ok(n, stride, 2)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sg_hash_kernel, dim3(stride / SG_BLOCK), dim3(SG_BLOCK), 0, st, sigs, pool, n, stride, e);
  return hipGetLastError();
}

hipError_t sg_launch_scalars(hipStream_t st, const sg_sig* sigs, const sc* e, uint32_t n, uint32_t stride, int nhash,
                             sg_kw* u1, int8_t* dig, uint8_t* flip) {
  if (n == 0) return hipSuccess;
  if (!sg_shape_ok(n, stride, nhash)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sg_scalar_kernel, dim3(stride / SG_BLOCK), dim3(SG_BLOCK), 0, st, sigs, e, n, stride, nhash, u1, dig,
                     flip);
  return hipGetLastError();
}

hipError_t sg_launch_ladder(hipStream_t st, const ge* tab, uint32_t n, uint32_t stride, const int8_t* dig,
                            const uint8_t* flip, sg_pt* T, uint8_t* tinf) {
  if (n == 0) return hipSuccess;
  if (!sg_shape_ok(n, stride, 1)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sg_ladder_kernel, dim3(stride / SG_BLOCK), dim3(SG_BLOCK), 0, st, tab, n, stride, dig, flip, T, tinf);
  return hipGetLastError();
}

hipError_t sg_launch_comb(hipStream_t st, const ge* table, const sg_sig* sigs, const sg_kw* u1, const sg_pt* T,
                          const uint8_t* tinf, const uint32_t* ok, uint32_t n, uint32_t stride, int nhash,
                          uint8_t* verdict) {
  if (n == 0) return hipSuccess;
  if (!sg_shape_ok(n, stride, nhash)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sg_comb_kernel, dim3(stride / SG_BLOCK), dim3(SG_BLOCK), 0, st, table, sigs, u1, T, tinf, ok, n,
                     stride, nhash, verdict);
  return hipGetLastError();
}
