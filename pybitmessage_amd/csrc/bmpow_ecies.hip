// bmpow_ecies.hip -- batched ECIES trial decryption of received msgs and broadcasts (gfx950).
//
// Reference: class_objectProcessor.processmsg tries every msg that passed the PoW check against every
// private key the user holds (src/class_objectProcessor.py:459-477; broadcasts :779-790), each try
// one pyelliptic.ECC.decrypt (src/pyelliptic/ecc.py:484-501):
//     key = SHA512(x(k R)),  key_e = key[:32],  key_m = key[32:]
//     the key matches iff HMAC_SHA256(key_m, data[:-32]) == data[-32:]
// Almost every try fails, so the batch computes only the verdict (and key_e of the matching pair); the
// AES pass of the few matches is a call of its own (bmpow_aes256_cbc, bmpow_seal.hip).  Host side:
// bmpow_host_ecies.hip.
//
// Three kernels, one lane per object, 64 objects and ONE key per wave:
//   ec_prep_kernel : per object, once: the on-curve check and the table of odd multiples of R;
//   ec_keys_kernel : per (object, key): the signed-window ladder (the key's digits are wave-uniform, so
//                    the wave never diverges), x = X / Z^2, one SHA-512 block -> key_e, key_m;
//   ec_mac_kernel  : per (object, key): HMAC-SHA256 over the object's host-padded blocks, compare, and
//                    an atomicMin of the key index into match[object].
// and, for rows that each name their own key (a v5 broadcast's tag, a needed v4 pubkey's address:
// bmpow_host_rxobjopen.hip), ec_rowkeys_kernel: ec_keys_kernel's work with per-lane digits, one key per row.
// The two phases stay apart: the ladder costs every lane the same (~2,700 field multiplications), the
// MAC follows the object's length, and the host sorts the objects by block count so a wave's lanes
// iterate alike (as the verification pool does).  Every loop bound comes from a host-validated length
// and a lane reads exactly its own nblk blocks of the pool.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sha512_dev.h"

#include "bmpow_ecies_kernels.h"
#include "secp256k1_var_dev.h"
#include "sha256_dev.h"

using ec::fe;
using ec::ge;

static_assert(EC_ENTRIES == ec::kVarEntries && EC_DIGITS == ec::kVarDigits, "table / digit layout");

__global__ __launch_bounds__(EC_BLOCK) void ec_prep_kernel(const ge* __restrict__ pts, uint32_t n, uint32_t stride,
                                                           ge* __restrict__ tab, uint32_t* __restrict__ ok) {
  const uint32_t o = blockIdx.x * EC_BLOCK + threadIdx.x;
  if (o >= n) return;
  ge R = pts[o];
  const bool on = ec::ge_on_curve(R);
  ok[o] = on ? 1u : 0u;
  if (!on) ec::ge_set_generator(R);
  ec::var_table(tab, stride, o, R);
}

// SHA512 of the 32-byte big-endian x: one block, x || 0x80 || zeros || 256
BM_DEV void sha512_of_x(uint64_t (&h)[8], const fe& x) {
  uint64_t xw[4], w[16];
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
}

__global__ __launch_bounds__(EC_BLOCK) void ec_keys_kernel(const ge* __restrict__ tab, uint32_t n, uint32_t stride,
                                                           const int32_t* __restrict__ dig, uint32_t nkeys,
                                                           uint64_t* __restrict__ kout) {
  const uint32_t o = blockIdx.x * EC_BLOCK + threadIdx.x;
  const uint32_t k = blockIdx.y;  // wave-uniform: the digit loads are scalar
  if (o >= n) return;
  fe x;
  ec::var_mult_x(x, tab, stride, o, dig + (size_t)k * EC_DIGITS);
  uint64_t h[8];
  sha512_of_x(h, x);
  const size_t plane = (size_t)nkeys * stride, at = (size_t)k * stride + o;
#pragma unroll
  for (int w = 0; w < 8; ++w) kout[w * plane + at] = h[w];
}

__global__ __launch_bounds__(EC_BLOCK) void ec_raw_kernel(const ge* __restrict__ tab, uint32_t n, uint32_t stride,
                                                          const int32_t* __restrict__ dig, fe* __restrict__ x_out,
                                                          uint32_t* __restrict__ ok) {
  const uint32_t o = blockIdx.x * EC_BLOCK + threadIdx.x;
  if (o >= n) return;
  fe x;
  const bool finite = ec::var_mult_x(x, tab, stride, o, dig + (size_t)o * EC_DIGITS);
  x_out[o] = x;
  if (!finite) ok[o] = 0;
}

// One key per ROW: lane o runs the ladder over its own table with the digits of key kidx[o] of the table of
// recoded keys (a v5 broadcast's key is the one filed under its tag, a v4 pubkey's the one of the address that
// is awaited under its tag), then the SHA-512 block, into kout in ec_keys_kernel's layout for nkeys == 1
// (plane = stride), so that ec_mac_kernel and ec_gather_kernel take it as they stand.  The digit is a per-lane
// load (as in ec_raw_kernel); the ladder is branch-free in it, so the wave does not diverge.  A lane whose index
// is not in the table refuses its row (ok[o] = 0: the MAC kernel skips it) and reads no digit at all.
__global__ __launch_bounds__(EC_BLOCK) void ec_rowkeys_kernel(const ge* __restrict__ tab, uint32_t n, uint32_t stride,
                                                              const int32_t* __restrict__ dig, uint32_t ntab,
                                                              const int32_t* __restrict__ kidx,
                                                              uint64_t* __restrict__ kout, uint32_t* __restrict__ ok) {
  const uint32_t o = blockIdx.x * EC_BLOCK + threadIdx.x;
  if (o >= n) return;
  const int32_t k = kidx[o];
  if (k < 0 || (uint32_t)k >= ntab) {
    ok[o] = 0;
#pragma unroll
    for (int w = 0; w < 8; ++w) kout[(size_t)w * stride + o] = 0;
    return;
  }
  fe x;
  const bool finite = ec::var_mult_x(x, tab, stride, o, dig + (size_t)k * EC_DIGITS);
  uint64_t h[8];
  sha512_of_x(h, x);
#pragma unroll
  for (int w = 0; w < 8; ++w) kout[(size_t)w * stride + o] = h[w];
  if (!finite) ok[o] = 0;
}

__global__ __launch_bounds__(EC_BLOCK) void ec_mac_kernel(const uint64_t* __restrict__ kout, uint32_t n, uint32_t stride,
                                                          uint32_t nkeys, const ec_obj* __restrict__ objs,
                                                          const uint4* __restrict__ pool,
                                                          const uint32_t* __restrict__ ok, int key0,
                                                          int* __restrict__ match) {
  const uint32_t o = blockIdx.x * EC_BLOCK + threadIdx.x;
  const uint32_t k = blockIdx.y;
  if (o >= n || !ok[o]) return;
  const size_t plane = (size_t)nkeys * stride, at = (size_t)k * stride + o;
  uint32_t key[8];
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const uint64_t v = kout[(size_t)(4 + w) * plane + at];
    key[2 * w] = (uint32_t)(v >> 32);
    key[2 * w + 1] = (uint32_t)v;
  }
  const ec_obj ob = objs[o];
  uint32_t hi[8], ho[8];
  s256::hmac_key_states(hi, ho, key);
  s256::hmac_inner(hi, pool + (size_t)ob.blk * 4, ob.nblk);
  s256::hmac_outer(ho, hi);
  uint32_t diff = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) diff |= ho[i] ^ ob.mac[i];
  if (diff == 0) atomicMin(match + o, key0 + (int)k);
}

__global__ __launch_bounds__(EC_BLOCK) void ec_gather_kernel(const uint64_t* __restrict__ kout, uint32_t n,
                                                             uint32_t stride, uint32_t nkeys, int key0,
                                                             const int* __restrict__ match,
                                                             uint64_t* __restrict__ key_e) {
  const uint32_t o = blockIdx.x * EC_BLOCK + threadIdx.x;
  if (o >= n) return;
  const int m = match[o];
  if (m < key0 || m >= key0 + (int)nkeys) return;
  const size_t plane = (size_t)nkeys * stride, at = (size_t)(m - key0) * stride + o;
#pragma unroll
  for (int w = 0; w < 4; ++w) key_e[(size_t)4 * o + w] = kout[(size_t)w * plane + at];
}

// ---------------------------------------------------------------------------------------
// Launch wrappers (C++ linkage, used by bmpow_host_ecies.hip).  stride is a multiple of EC_BLOCK.
// ---------------------------------------------------------------------------------------
static bool ec_shape_ok(uint32_t n, uint32_t stride) { return n <= stride && stride % EC_BLOCK == 0; }

hipError_t ec_launch_prep(hipStream_t st, const ge* pts, uint32_t n, uint32_t stride, ge* tab, uint32_t* ok) {
  if (n == 0) return hipSuccess;
  if (!ec_shape_ok(n, stride)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ec_prep_kernel, dim3(stride / EC_BLOCK), dim3(EC_BLOCK), 0, st, pts, n, stride, tab, ok);
  return hipGetLastError();
}

hipError_t ec_launch_keys(hipStream_t st, const ge* tab, uint32_t n, uint32_t stride, const int32_t* dig, uint32_t nkeys,
                          uint64_t* kout) {
  if (n == 0 || nkeys == 0) return hipSuccess;
  if (!ec_shape_ok(n, stride) || nkeys > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ec_keys_kernel, dim3(stride / EC_BLOCK, nkeys), dim3(EC_BLOCK), 0, st, tab, n, stride, dig, nkeys,
                     kout);
  return hipGetLastError();
}

hipError_t ec_launch_raw(hipStream_t st, const ge* tab, uint32_t n, uint32_t stride, const int32_t* dig, fe* x_out,
                         uint32_t* ok) {
  if (n == 0) return hipSuccess;
  if (!ec_shape_ok(n, stride)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ec_raw_kernel, dim3(stride / EC_BLOCK), dim3(EC_BLOCK), 0, st, tab, n, stride, dig, x_out, ok);
  return hipGetLastError();
}

hipError_t ec_launch_rowkeys(hipStream_t st, const ge* tab, uint32_t first, uint32_t n, uint32_t stride,
                             const int32_t* dig, uint32_t ntab, const int32_t* kidx, uint64_t* kout, uint32_t* ok) {
  if (n == 0) return hipSuccess;
  if (!ec_shape_ok(n, stride) || first > stride - n || !tab || !dig || !kidx || !kout || !ok) return hipErrorInvalidValue;
  // rows first .. first + n of the set: every per-row array is entered at `first`, the strides stay the set's
  hipLaunchKernelGGL(ec_rowkeys_kernel, dim3((n + EC_BLOCK - 1) / EC_BLOCK), dim3(EC_BLOCK), 0, st, tab + first, n, stride,
                     dig, ntab, kidx, kout + first, ok + first);
  return hipGetLastError();
}

hipError_t ec_launch_mac(hipStream_t st, const uint64_t* kout, uint32_t n, uint32_t stride, uint32_t nkeys,
                         const ec_obj* objs, const uint4* pool, const uint32_t* ok, int key0, int* match) {
  if (n == 0 || nkeys == 0) return hipSuccess;
  if (!ec_shape_ok(n, stride) || nkeys > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ec_mac_kernel, dim3(stride / EC_BLOCK, nkeys), dim3(EC_BLOCK), 0, st, kout, n, stride, nkeys, objs,
                     pool, ok, key0, match);
  return hipGetLastError();
}

hipError_t ec_launch_gather(hipStream_t st, const uint64_t* kout, uint32_t n, uint32_t stride, uint32_t nkeys, int key0,
                            const int* match, uint64_t* key_e) {
  if (n == 0 || nkeys == 0) return hipSuccess;
  if (!ec_shape_ok(n, stride)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ec_gather_kernel, dim3(stride / EC_BLOCK), dim3(EC_BLOCK), 0, st, kout, n, stride, nkeys, key0, match,
                     key_e);
  return hipGetLastError();
}
