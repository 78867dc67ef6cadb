// bmpow_ecies_kernels.h -- device data layout and launch wrappers of the ECIES trial decryption
// (bmpow_ecies.hip), shared with its host unit (bmpow_host_ecies.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "secp256k1_dev.h"

constexpr uint32_t EC_BLOCK = 64;   // one wave: 64 objects, one key
constexpr int EC_ENTRIES = 8;       // table entries per object (R, 3R, ..., 15R)
constexpr int EC_DIGITS = 64;       // signed odd base-16 digits per key, one int32 each
constexpr int EC_NO_MATCH = 0x7f7f7f7f;  // match[] before any key verified (a byte memset)

// One object's MACed bytes in the pool: data[:-32] padded as the tail of the inner HMAC hash (the
// message (K ^ ipad) || data), in 64-byte blocks; and the MAC it must equal, as big-endian words.
struct ec_obj {
  uint32_t blk;   // first 64-byte block in the pool
  uint32_t nblk;  // ceil((len + 9) / 64), >= 1
  uint32_t mac[8];
};

// Objects are indexed 0 .. n within a launch set; stride >= n is n rounded up to EC_BLOCK.
//   pts[o]                : the ephemeral point, coordinates canonical (< p)
//   tab[e * stride + o]   : (2e + 1) R of object o
//   ok[o]                 : 1 when the point is on the curve
//   dig[k * EC_DIGITS + i]: digit i of key k (ec_launch_keys), or of pair k (ec_launch_raw)
//   kout[w * plane + k * stride + o], plane = nkeys * stride: word w (big-endian u64) of
//                           SHA512(x(key k * R_o)); words 0..3 key_e, 4..7 key_m
hipError_t ec_launch_prep(hipStream_t st, const ec::ge* pts, uint32_t n, uint32_t stride, ec::ge* tab, uint32_t* ok);
hipError_t ec_launch_keys(hipStream_t st, const ec::ge* tab, uint32_t n, uint32_t stride, const int32_t* dig,
                          uint32_t nkeys, uint64_t* kout);
// One key per row, for rows first .. first + n of the set (first + n <= stride): row first + o takes key kidx[o] of
// the ntab recoded keys in dig and leaves SHA512(x(key * R)) at kout[w * stride + first + o], the layout of
// ec_launch_keys for nkeys == 1; ok[first + o] = 0 where kidx[o] is not in 0 .. ntab (no digit is read) or the
// product is infinite.  ec_launch_mac / ec_launch_gather then run with nkeys == 1, key0 == 0 and kout, objs, ok,
// match and key_e entered at `first`.
hipError_t ec_launch_rowkeys(hipStream_t st, const ec::ge* tab, uint32_t first, uint32_t n, uint32_t stride,
                             const int32_t* dig, uint32_t ntab, const int32_t* kidx, uint64_t* kout, uint32_t* ok);
// x_out[o] = x(k_o R_o), canonical little-endian limbs; ok[o] &= (k_o R_o is finite)
hipError_t ec_launch_raw(hipStream_t st, const ec::ge* tab, uint32_t n, uint32_t stride, const int32_t* dig,
                         ec::fe* x_out, uint32_t* ok);
// match[o] = min(match[o], key0 + k) over the keys k < nkeys whose HMAC of object o equals its MAC
hipError_t ec_launch_mac(hipStream_t st, const uint64_t* kout, uint32_t n, uint32_t stride, uint32_t nkeys,
                         const ec_obj* objs, const uint4* pool, const uint32_t* ok, int key0, int* match);
// key_e[4 o .. 4 o + 4) = key_e words of the pair (o, match[o]) when key0 <= match[o] < key0 + nkeys
hipError_t ec_launch_gather(hipStream_t st, const uint64_t* kout, uint32_t n, uint32_t stride, uint32_t nkeys, int key0,
                            const int* match, uint64_t* key_e);
