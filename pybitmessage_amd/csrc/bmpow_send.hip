// bmpow_send.hip -- batched ECDSA signing and ECIES key agreement of outgoing objects (gfx950).
//
// Reference: highlevelcrypto.sign / encrypt / pointMult (src/highlevelcrypto.py:54-85, :111-146), one
// pyelliptic call per outgoing object (src/class_singleWorker.py:1224-1234):
//     sign:     r = x(k G) mod n,  s = (e + r d) / k mod n           (ECC.sign, src/pyelliptic/ecc.py:319-385)
//     encrypt:  R = t G,  key = SHA512(x(t Q)),  key_e = key[:32], key_m = key[32:]
//                                                               (ECC.raw_encrypt, :462-482)
// The receive side's arithmetic composed the other way round (bmpow_sig.hip, bmpow_ecies.hip).  The AES
// and HMAC pass is bmpow_seal.hip's kernel behind these, or libcrypto on the host.  Host side:
// bmpow_host_send.hip.
//
// One lane per row, the phases as separate kernels so that no phase's register allocation carries
// another's state:
//   sg_hash_kernel   : (bmpow_sig.hip) SHA-1 and SHA-256 of the message;
//   sd_comb_kernel   : k G by 16 mixed additions of 16-bit-comb entries from infinity, one inversion of Z:
//                      the public key of bmpow_ec_pubkeys, the signature's k G, the ephemeral R;
//   sd_sign_kernel   : r = x mod n, k^-1 (Fermat, a fixed exponent), s;
//   sd_digits_kernel : the ephemeral key's signed odd digits;
//   ec_prep_kernel   : (bmpow_ecies.hip) the on-curve check of the recipient key and its table;
//   sd_shared_kernel : t Q by the signed-window ladder with per-lane digits, x = X / Z^2, SHA-512.
// The scalars are the host's own (range-checked there: 1 <= k < n), the recipient keys are not: the
// ladder's additions take gej_add_ge's complete path, and a refused key's lane works on G.  Lanes past n
// do nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sha512_dev.h"

#include "bmpow_send_kernels.h"
#include "secp256k1_var_dev.h"

using ec::fe;
using ec::ge;
using ec::gej;
using sn::sc;

static_assert(SG_DIGITS == ec::kVarDigits, "digit layout");

BM_DEV void kw_to_sc(sc& r, const sg_kw& kw) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    r.d[7 - 2 * j] = (uint32_t)(kw.w[j] >> 32);
    r.d[6 - 2 * j] = (uint32_t)kw.w[j];
  }
}

__global__ __launch_bounds__(SD_BLOCK) void sd_comb_kernel(const ge* __restrict__ table, const sg_kw* __restrict__ kw,
                                                           uint32_t n, ge* __restrict__ pt) {
  const uint32_t o = blockIdx.x * SD_BLOCK + threadIdx.x;
  if (o >= n) return;
  using C = ec::comb<ec::kCombSmall>;
  const sg_kw k = kw[o];
  uint64_t s[4] = {k.w[3], k.w[2], k.w[1], k.w[0]};
  gej acc;
  ec::fe_set(acc.x, 0);
  ec::fe_set(acc.y, 0);
  ec::fe_set(acc.z, 0);
  acc.inf = true;
  // a zero window is skipped (one in 65,536), every other one is a complete addition: for k < n the
  // partial sum never meets plus or minus the entry (scalar_mult_base_jac), so the cases cost nothing
#pragma unroll 1
  for (int i = 0; i < C::kWindows; ++i) {
    const uint32_t v = (uint32_t)s[0] & C::kMask;
    ec::shr256_window<ec::kCombSmall>(s);
    if (v) {
      const ge q = table[((size_t)i << ec::kCombSmall) | v];
      ec::gej_add_ge(acc, acc, q);
    }
  }
  ge r;
  ec::fe_set(r.x, 0);
  ec::fe_set(r.y, 0);
  if (!acc.inf) ec::gej_to_ge(r, acc);  // 1 <= k < n: always
  pt[o] = r;
}

__global__ __launch_bounds__(SD_BLOCK) void sd_sign_kernel(const ge* __restrict__ pt, const sg_kw* __restrict__ kw,
                                                           const sc* __restrict__ d, const sc* __restrict__ e,
                                                           uint32_t n, uint32_t stride, sc* __restrict__ rs,
                                                           uint8_t* __restrict__ ok) {
  const uint32_t o = blockIdx.x * SD_BLOCK + threadIdx.x;
  if (o >= n) return;
  // r = x mod n: x < p < 2 n, one conditional subtraction
  sc x, r, k, ki, one, em, t, s;
#pragma unroll
  for (int i = 0; i < 8; ++i) x.d[i] = pt[o].x.d[i];
  sn::cond_sub_n(r, x);
  kw_to_sc(k, kw[o]);
  sn::inv(ki, k);
  sn::set(one, 1);
  sn::mul(em, e[o], one);  // e mod n
  sn::mul(t, r, d[o]);
  sn::add(t, t, em);
  sn::mul(s, ki, t);
  rs[o] = r;
  rs[(size_t)stride + o] = s;
  ok[o] = !sn::is_zero(r) && !sn::is_zero(s) ? 1 : 0;
}

__global__ __launch_bounds__(SD_BLOCK) void sd_digits_kernel(const sg_kw* __restrict__ kw, uint32_t n, uint32_t stride,
                                                             int8_t* __restrict__ dig) {
  const uint32_t o = blockIdx.x * SD_BLOCK + threadIdx.x;
  if (o >= n) return;
  sc u, k;
  kw_to_sc(u, kw[o]);
  sn::make_odd(k, u);  // n - t for an even t: x(t Q) = x((n - t) Q), as recode_key drops the sign
#pragma unroll
  for (int i = 0; i < SG_DIGITS; ++i) dig[(size_t)i * stride + o] = (int8_t)sn::recode_digit(k, i);
}

__global__ __launch_bounds__(SD_BLOCK) void sd_shared_kernel(const ge* __restrict__ tab, uint32_t n, uint32_t stride,
                                                             const int8_t* __restrict__ dig,
                                                             uint64_t* __restrict__ kout) {
  const uint32_t o = blockIdx.x * SD_BLOCK + threadIdx.x;
  if (o >= n) return;
  gej acc;
  ec::var_mult_jac(acc, tab, stride, o, dig + o, stride);
  fe x, zi;
  ec::fe_set(x, 0);
  if (!acc.inf) {  // the table's point has the order n and 1 <= t < n: always
    ec::fe_inv(zi, acc.z);
    ec::fe_sqr(zi, zi);
    ec::fe_mul(x, acc.x, zi);
    ec::fe_normalize(x, x);
  }
  // SHA512 of the 32-byte big-endian x: one block, x || 0x80 || zeros || 256
  uint64_t xw[4], w[16], h[8];
  ec::fe_to_be64(xw, x);
#pragma unroll
  for (int i = 0; i < 4; ++i) w[i] = xw[i];
  w[4] = bm::PAD;
#pragma unroll
  for (int i = 5; i < 15; ++i) w[i] = 0;
  w[15] = 32 * 8;
#pragma unroll
  for (int i = 0; i < 8; ++i) h[i] = bm::IV(i);
  bm::compress(h, w);
#pragma unroll
  for (int i = 0; i < 8; ++i) kout[(size_t)i * stride + o] = h[i];
}

// ---------------------------------------------------------------------------------------
// Launch wrappers (C++ linkage, used by bmpow_host_send.hip).  stride is a multiple of SD_BLOCK.
// ---------------------------------------------------------------------------------------
static bool sd_shape_ok(uint32_t n, uint32_t stride) { return n <= stride && stride % SD_BLOCK == 0; }

hipError_t sd_launch_comb(hipStream_t st, const ge* table, const sg_kw* kw, uint32_t n, uint32_t stride, ge* pt) {
  if (n == 0) return hipSuccess;
  if (!sd_shape_ok(n, stride)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sd_comb_kernel, dim3(stride / SD_BLOCK), dim3(SD_BLOCK), 0, st, table, kw, n, pt);
  return hipGetLastError();
}

hipError_t sd_launch_sign(hipStream_t st, const ge* pt, const sg_kw* kw, const sc* d, const sc* e, uint32_t n,
                          uint32_t stride, sc* rs, uint8_t* ok) {
  if (n == 0) return hipSuccess;
  if (!sd_shape_ok(n, stride)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sd_sign_kernel, dim3(stride / SD_BLOCK), dim3(SD_BLOCK), 0, st, pt, kw, d, e, n, stride, rs, ok);
  return hipGetLastError();
}

hipError_t sd_launch_digits(hipStream_t st, const sg_kw* kw, uint32_t n, uint32_t stride, int8_t* dig) {
  if (n == 0) return hipSuccess;
  if (!sd_shape_ok(n, stride)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sd_digits_kernel, dim3(stride / SD_BLOCK), dim3(SD_BLOCK), 0, st, kw, n, stride, dig);
  return hipGetLastError();
}

hipError_t sd_launch_shared(hipStream_t st, const ge* tab, uint32_t n, uint32_t stride, const int8_t* dig,
                            uint64_t* kout) {
  if (n == 0) return hipSuccess;
  if (!sd_shape_ok(n, stride)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sd_shared_kernel, dim3(stride / SD_BLOCK), dim3(SD_BLOCK), 0, st, tab, n, stride, dig, kout);
  return hipGetLastError();
}
