// bmpow_host_scalar.h -- the host units' scalar and byte toolkit (internal; host only, no HIP: plain g++
// compiles it, and tests/native/hostscalar_sim.cpp runs it under the sanitizers): big-endian bytes to
// scalars and back, the range checks of a scalar (1 <= a < n) and a coordinate (a < p), the SHA padding of
// a message, the DER encoder and the strict DER parser of a signature, and the secrets' helpers -- a host
// vector that is cleansed when it dies and the random draws.  One definition of each, for the signing,
// verifying and sending units alike.
#pragma once
#include <openssl/crypto.h>
#include <openssl/rand.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <memory>
#include <vector>

#include "scalar_dev.h"

namespace bmhost {

using sn::sc;

inline sc sc_from_be(const uint8_t* b) {  // 32 big-endian bytes
  sc r;
  for (int i = 0; i < 8; ++i)
    r.d[7 - i] = (uint32_t)b[4 * i] << 24 | (uint32_t)b[4 * i + 1] << 16 | (uint32_t)b[4 * i + 2] << 8 | b[4 * i + 3];
  return r;
}

inline void sc_to_be(const uint32_t (&d)[8], uint8_t* out) {
  for (int w = 0; w < 8; ++w)
    for (int q = 0; q < 4; ++q) out[4 * w + q] = (uint8_t)(d[7 - w] >> (24 - 8 * q));
}

inline bool scalar_in_range(const sc& a) {  // 1 <= a < n
  sc t;
  return !sn::is_zero(a) && !sn::cond_sub_n(t, a);
}

inline bool scalar_in_range(const uint8_t* b) { return scalar_in_range(sc_from_be(b)); }

inline bool coord_in_range(const sc& a) {  // a < p = 2^256 - 2^32 - 977
  for (int i = 7; i >= 2; --i)
    if (a.d[i] != 0xFFFFFFFFu) return true;
  if (a.d[1] != 0xFFFFFFFEu) return a.d[1] < 0xFFFFFFFEu;
  return a.d[0] < 0xFFFFFC2Fu;
}

inline uint32_t msg_blocks(size_t len) { return (uint32_t)((len + 9 + 63) / 64); }

// data || 0x80 || zeros || the bit length as 8 big-endian bytes, into nblk * 64 bytes
inline void pad_blocks(const uint8_t* data, size_t len, uint8_t* dst, uint32_t nblk) {
  const size_t total = (size_t)nblk * 64;
  if (len) std::memcpy(dst, data, len);
  dst[len] = 0x80;
  std::memset(dst + len + 1, 0, total - len - 1 - 8);
  const uint64_t bits = (uint64_t)len * 8;
  for (int j = 0; j < 8; ++j) dst[total - 8 + j] = (uint8_t)(bits >> (56 - 8 * j));
}

// ---- DER, out: a DER INTEGER of the 32 big-endian bytes v (not all zero): minimal, a 0x00 in front of a
// set top bit
inline size_t der_put_int(const uint8_t* v, uint8_t* out) {
  size_t skip = 0;
  while (skip < 31 && v[skip] == 0) ++skip;
  const size_t pad = v[skip] & 0x80 ? 1 : 0, l = 32 - skip + pad;
  out[0] = 0x02;
  out[1] = (uint8_t)l;
  out[2] = 0;
  std::memcpy(out + 2 + pad, v + skip, 32 - skip);
  return 2 + l;
}

inline bool all_zero(const uint8_t* p, size_t n) {
  uint8_t o = 0;
  for (size_t i = 0; i < n; ++i) o |= p[i];
  return o == 0;
}

inline size_t sig_der(const uint8_t rs[64], uint8_t out[72]) {
  const size_t lr = der_put_int(rs, out + 2), ls = der_put_int(rs + 32, out + 2 + lr);
  out[0] = 0x30;
  out[1] = (uint8_t)(lr + ls);  // at most 70: short form
  return 2 + lr + ls;
}

// ---- DER, in: one INTEGER at p[pos ..): minimal, non-negative, at most 32 value bytes; out = its 32-byte
// big-endian value, pos moved past it.
inline bool der_take_int(const uint8_t* p, size_t len, size_t& pos, uint8_t out[32]) {
  if (len - pos < 2 || p[pos] != 0x02) return false;
  size_t l = p[pos + 1];
  if (l == 0 || l >= 0x80 || len - pos - 2 < l) return false;
  const uint8_t* v = p + pos + 2;
  if (v[0] & 0x80) return false;                           // negative
  if (l > 1 && v[0] == 0 && !(v[1] & 0x80)) return false;  // a zero byte the sign does not need
  pos += 2 + l;
  if (v[0] == 0) ++v, --l;
  if (l > 32) return false;
  std::memset(out, 0, 32 - l);
  std::memcpy(out + 32 - l, v, l);
  return true;
}

inline bool sig_parse(const uint8_t* p, size_t len, uint8_t rs[64]) {
  if (len < 8 || p[0] != 0x30 || p[1] >= 0x80 || (size_t)p[1] != len - 2) return false;
  size_t pos = 2;
  uint8_t tmp[64];
  if (!der_take_int(p, len, pos, tmp) || !der_take_int(p, len, pos, tmp + 32) || pos != len) return false;
  if (!scalar_in_range(tmp) || !scalar_in_range(tmp + 32)) return false;
  std::memcpy(rs, tmp, 64);
  return true;
}

// ---- secrets.  A host vector that held some: sized once (a growth would leave an unwiped copy), zeroed
// when it dies.
template <class T>
struct Wiped {
  std::vector<T> v;
  ~Wiped() {
    if (!v.empty()) OPENSSL_cleanse(v.data(), v.size() * sizeof(T));
  }
};

// The same for a staging pool too large to zero-fill on allocation: n bytes, left as they come.
struct WipedBytes {
  std::unique_ptr<uint8_t[]> p;
  size_t bytes = 0;
  void alloc(size_t n) {
    wipe();
    p.reset(new uint8_t[n]);
    bytes = n;
  }
  uint8_t* get() const { return p.get(); }
  ~WipedBytes() { wipe(); }

 private:
  void wipe() {
    if (p) OPENSSL_cleanse(p.get(), bytes);
  }
};

inline bool draw_bytes(uint8_t* out, size_t len) {  // RAND_bytes takes an int
  for (size_t at = 0; at < len; at += 1u << 20)
    if (RAND_bytes(out + at, (int)std::min<size_t>(1u << 20, len - at)) != 1) return false;
  return true;
}

// 32 random bytes in [1, n - 1], by rejection (the excluded share is 2^-128)
inline bool draw_scalar(uint8_t out[32]) {
  do {
    if (RAND_bytes(out, 32) != 1) return false;
  } while (!scalar_in_range(out));
  return true;
}

// n of them: one draw for all, then the rejected rows again
inline bool draw_scalars(uint8_t* out, size_t n) {
  if (!draw_bytes(out, 32 * n)) return false;
  for (size_t i = 0; i < n; ++i)
    if (!scalar_in_range(out + 32 * i) && !draw_scalar(out + 32 * i)) return false;
  return true;
}

}  // namespace bmhost
