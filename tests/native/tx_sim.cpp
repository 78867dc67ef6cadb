// tx_sim.cpp -- the byte-oriented code of the outgoing-object kernels (pybitmessage_amd/csrc/bmpow_tx_fmt.h)
// on the host, as a stand-alone program: tests/test_tx.py builds it with g++ under AddressSanitizer + UBSan
// and runs it.  Every row works in heap blocks of exactly the size the device gives it (the body, the
// 64-byte head field, the hash blocks, the seal slot), so a byte read or written past one is an error; the
// DER encoding is compared with libcrypto's i2d_ECDSA_SIG.  Loads neither HIP nor the library.
#include <openssl/bn.h>
#include <openssl/ecdsa.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bmpow_tx_fmt.h"

static int g_fail = 0;
static long g_checks = 0;
#define CHECK(cond, ...)                                        \
  do {                                                          \
    ++g_checks;                                                 \
    if (!(cond)) {                                              \
      std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
      std::fprintf(stderr, __VA_ARGS__);                        \
      std::fputc('\n', stderr);                                 \
      if (++g_fail > 20) std::exit(1);                          \
    }                                                           \
  } while (0)

struct Exact {  // exactly n bytes from malloc: ASan's redzone starts at byte n
  uint8_t* p;
  explicit Exact(size_t n, int fill = 0xA5) : p((uint8_t*)std::malloc(n ? n : 1)) { std::memset(p, fill, n ? n : 1); }
  ~Exact() { std::free(p); }
};

typedef std::vector<uint8_t> bytes;

static void words(uint32_t (&w)[8], const bytes& v) {  // a value of at most 32 bytes, big-endian, into 8 words
  uint8_t b[32] = {0};
  std::memcpy(b + 32 - v.size(), v.data(), v.size());
  for (int i = 0; i < 8; ++i) w[i] = (uint32_t)b[4 * i] << 24 | (uint32_t)b[4 * i + 1] << 16 | (uint32_t)b[4 * i + 2] << 8 | b[4 * i + 3];
}

static bytes openssl_der(const bytes& r, const bytes& s) {
  ECDSA_SIG* sig = ECDSA_SIG_new();
  ECDSA_SIG_set0(sig, BN_bin2bn(r.data(), (int)r.size(), nullptr), BN_bin2bn(s.data(), (int)s.size(), nullptr));
  uint8_t buf[80], *p = buf;
  const int l = i2d_ECDSA_SIG(sig, &p);
  ECDSA_SIG_free(sig);
  return bytes(buf, buf + (l > 0 ? l : 0));
}

// a value whose minimal big-endian form is `len` bytes (1 .. 32), the first with its top bit as asked
static bytes value(size_t len, bool top, uint8_t seed) {
  bytes v(len);
  for (size_t i = 0; i < len; ++i) v[i] = (uint8_t)(seed * 31 + i * 7 + 1);
  v[0] = top ? (uint8_t)(0x80 | (seed & 0x7f)) : (uint8_t)(0x01 + (seed % 0x7f));
  return v;
}

static const uint8_t kOrder[32] = {0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFE,
                                   0xBA, 0xAE, 0xDC, 0xE6, 0xAF, 0x48, 0xA0, 0x3B, 0xBF, 0xD2, 0x5E, 0x8C, 0xD0, 0x36, 0x41, 0x41};

static void check_der() {
  std::vector<bytes> vals;
  for (size_t zeros : {0u, 1u, 2u, 31u})
    for (bool top : {false, true}) vals.push_back(value(32 - zeros, top, (uint8_t)(zeros + 3)));
  vals.push_back(bytes{1});
  bytes nm1(kOrder, kOrder + 32);
  nm1[31] -= 1;
  vals.push_back(nm1);
  for (const bytes& r : vals)
    for (const bytes& s : vals) {
      uint32_t rw[8], sw[8];
      words(rw, r);
      words(sw, s);
      const bytes want = openssl_der(r, s);
      Exact out(want.size());  // exactly the encoding's length: one byte more is an error
      const uint32_t got = txf::put_sig(out.p, rw, sw);
      CHECK(got == want.size(), "DER length %u, libcrypto %zu", got, want.size());
      CHECK(got == want.size() && std::memcmp(out.p, want.data(), got) == 0, "DER bytes differ (r %zu, s %zu bytes)", r.size(), s.size());
      CHECK(got <= txf::kMaxDer, "DER above 72 bytes");
    }
}

static void check_pack() {
  for (uint32_t head_len = txf::kHeadMin; head_len <= txf::kHeadMax; ++head_len) {
    Exact head(64, 0);  // the row struct's field: zero behind head_len
    for (uint32_t i = 0; i < head_len; ++i) head.p[i] = (uint8_t)(0x40 + i);
    // an empty body, then every signed length 64 .. 191: each residue mod 64 under two and under three blocks
    for (uint32_t signed_len = head_len; signed_len <= 191; signed_len = signed_len < 64 ? 64 : signed_len + 1) {
      const uint32_t body_len = signed_len - head_len, nblk = txf::signed_blocks(signed_len);
      Exact body(body_len);
      for (uint32_t i = 0; i < body_len; ++i) body.p[i] = (uint8_t)(i * 13 + 5);
      bytes want(64 * nblk, 0);
      std::memcpy(want.data(), head.p, head_len);
      if (body_len) std::memcpy(want.data() + head_len, body.p, body_len);
      want[signed_len] = 0x80;
      const uint64_t bits = (uint64_t)signed_len * 8;
      for (int j = 0; j < 8; ++j) want[64 * nblk - 8 + j] = (uint8_t)(bits >> (56 - 8 * j));
      CHECK(nblk == (signed_len + 9 + 63) / 64 && signed_len + 9 <= 64 * nblk, "block count");
      Exact pool(64 * nblk);
      for (uint32_t c = 0; c < 4 * nblk; ++c) {
        uint32_t w[4];
        txf::pack_chunk(c, nblk, head.p, head_len, body.p, body_len, w);
        std::memcpy(pool.p + 16 * c, w, 16);
      }
      CHECK(std::memcmp(pool.p, want.data(), want.size()) == 0, "packed blocks differ: head %u, signed %u", head_len, signed_len);
    }
  }
}

static void check_tail() {
  for (uint32_t body_len = 0; body_len <= 80; ++body_len)
    for (uint32_t sig_len = 8; sig_len <= txf::kMaxDer; ++sig_len) {
      // INTEGER contents of lr and ls bytes (1 .. 33 each, 33 = a 0x00 in front of 32) with 6 + lr + ls = sig_len
      const uint32_t sum = sig_len - 6, lr = sum - 1 < 33 ? sum - 1 : 33, ls = sum - lr;
      const bytes r = lr == 33 ? value(32, true, (uint8_t)body_len) : value(lr, false, (uint8_t)body_len);
      const bytes s = ls == 33 ? value(32, true, (uint8_t)sig_len) : value(ls, false, (uint8_t)sig_len);
      const bytes want = openssl_der(r, s);
      CHECK(want.size() == sig_len, "constructed signature is %zu bytes, wanted %u", want.size(), sig_len);
      const uint64_t slot_bytes = txf::slot_bytes(body_len);
      Exact slot(slot_bytes);
      for (uint32_t i = 0; i < body_len; ++i) slot.p[txf::body_at() + i] = (uint8_t)(i + 1);
      uint32_t rw[8], sw[8];
      words(rw, r);
      words(sw, s);
      const uint32_t got = txf::put_tail(slot.p, body_len, rw, sw);
      const uint32_t at = txf::tail_at(body_len);
      CHECK(got == sig_len, "put_tail returned %u for a %u-byte signature", got, sig_len);
      CHECK(at == SL_PLAIN_AT + body_len && at + 1 + got <= slot_bytes, "tail outside the slot");
      CHECK(slot.p[at] == sig_len, "the varint");
      CHECK(std::memcmp(slot.p + at + 1, want.data(), want.size()) == 0, "tail bytes differ: body %u, sig %u", body_len, sig_len);
      bool clean = true;
      for (uint32_t i = 0; i < txf::body_at(); ++i) clean = clean && slot.p[i] == 0xA5;
      for (uint32_t i = 0; i < body_len; ++i) clean = clean && slot.p[txf::body_at() + i] == (uint8_t)(i + 1);
      for (uint64_t i = at + 1 + got; i < slot_bytes; ++i) clean = clean && slot.p[i] == 0xA5;
      CHECK(clean, "bytes outside the tail changed: body %u, sig %u", body_len, sig_len);
      // the seal's plaintext length, and its bound
      CHECK(body_len + 1 + got <= body_len + txf::kTailMax, "plaintext above its bound");
      CHECK(slot_bytes == bmseal::seal_slot_bytes(body_len + txf::kTailMax) && slot_bytes % 16 == 0, "slot size");
    }
}

static void check_msg_words() {
  for (uint32_t head_len = txf::kHeadMin; head_len <= txf::kHeadMax; head_len += 5)
    for (uint32_t src_len = 0; src_len <= 300; ++src_len) {
      Exact head(64, 0), src(src_len);
      for (uint32_t i = 0; i < head_len; ++i) head.p[i] = (uint8_t)(0x11 + i);
      for (uint32_t i = 0; i < src_len; ++i) src.p[i] = (uint8_t)(i * 3 + 2);
      const uint32_t len = head_len + src_len, nblk = txf::payload_blocks(len);
      bytes want(128 * nblk, 0);
      std::memcpy(want.data(), head.p, head_len);
      if (src_len) std::memcpy(want.data() + head_len, src.p, src_len);
      want[len] = 0x80;
      CHECK(len + 17 <= 128 * nblk && len + 17 + 128 > 128 * nblk, "SHA-512 block count");
      bool same = true;
      for (uint32_t k = 0; k < 16 * nblk; ++k) {
        const uint64_t w = txf::msg_word(k, head.p, head_len, src.p, src_len);
        for (int j = 0; j < 8; ++j) same = same && (uint8_t)(w >> (56 - 8 * j)) == want[8 * k + j];
      }
      CHECK(same, "payload words differ: head %u, source %u", head_len, src_len);
    }
}

int main() {
  check_der();
  check_pack();
  check_tail();
  check_msg_words();
  if (g_fail) {
    std::fprintf(stderr, "%d tx checks failed\n", g_fail);
    return 1;
  }
  std::fprintf(stderr, "all tx checks passed (%ld checks)\n", g_checks);
  return 0;
}
