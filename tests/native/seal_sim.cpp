// seal_sim.cpp -- the seal kernels' per-row code (pybitmessage_amd/csrc/bmpow_seal_rows.h, aes256_dev.h,
// sha256_dev.h) and the set planner with its set cutter (bmpow_seal_plan.cpp) on the host, as a stand-alone program:
// tests/test_seal.py builds it with g++ under AddressSanitizer + UBSan and runs it.  Every row works in a
// heap slot of exactly the size the planner gives it, so a byte written or read past the slot is an error;
// the results are compared with libcrypto's EVP calls.  Loads neither HIP nor the library.
#include <openssl/evp.h>
#include <openssl/hmac.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

// the two gfx950 builtins sha256_dev.h uses, restated for the host
static inline uint32_t __builtin_amdgcn_alignbit(uint32_t hi, uint32_t lo, uint32_t n) {
  return (uint32_t)((((uint64_t)hi << 32) | lo) >> (n & 31));
}
static inline uint32_t __builtin_amdgcn_bitop3_b32(uint32_t a, uint32_t b, uint32_t c, uint32_t lut) {
  uint32_t r = 0;
  for (int i = 0; i < 32; ++i) {
    const uint32_t idx = ((a >> i) & 1) << 2 | ((b >> i) & 1) << 1 | ((c >> i) & 1);
    r |= ((lut >> idx) & 1u) << i;
  }
  return r;
}
struct uint4 {  // s256::hmac_inner's block type (HIP's); the rows do not call it
  uint32_t x, y, z, w;
};
#define BM_DEV [[maybe_unused]] static inline

#include "bmpow_seal_plan.h"
#include "bmpow_seal_rows.h"

static int g_fail = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
      std::fprintf(stderr, __VA_ARGS__);                  \
      std::fputc('\n', stderr);                           \
      if (++g_fail > 20) std::exit(1);                    \
    }                                                     \
  } while (0)

static aes::EncTab g_enc;
static aes::DecTab g_dec;

static std::vector<uint8_t> unhex(const char* h) {
  std::vector<uint8_t> v;
  for (; h[0] && h[1]; h += 2) {
    unsigned b = 0;
    std::sscanf(h, "%2x", &b);
    v.push_back((uint8_t)b);
  }
  return v;
}

static void words(uint32_t* w, const uint8_t* b, int n) {
  for (int i = 0; i < n; ++i) w[i] = (uint32_t)b[4 * i] << 24 | (uint32_t)b[4 * i + 1] << 16 | (uint32_t)b[4 * i + 2] << 8 | b[4 * i + 3];
}

struct Slot {  // 16-byte aligned, exactly n bytes
  uint8_t* p;
  explicit Slot(size_t n) : p((uint8_t*)std::aligned_alloc(16, n)) { std::memset(p, 0xA5, n); }
  ~Slot() { std::free(p); }
};

static std::vector<uint8_t> evp_cbc(bool enc, const uint8_t* key, const uint8_t* iv, const uint8_t* in, size_t len, bool& good) {
  std::vector<uint8_t> out(len + 32);
  EVP_CIPHER_CTX* c = EVP_CIPHER_CTX_new();
  int n1 = 0, n2 = 0;
  const uint8_t none = 0;
  good = EVP_CipherInit_ex(c, EVP_aes_256_cbc(), nullptr, key, iv, enc ? 1 : 0) == 1 &&
         EVP_CipherUpdate(c, out.data(), &n1, len ? in : &none, (int)len) == 1 && EVP_CipherFinal_ex(c, out.data() + n1, &n2) == 1;
  EVP_CIPHER_CTX_free(c);
  out.resize(good ? (size_t)(n1 + n2) : 0);
  return out;
}

static std::vector<uint8_t> ref_seal(const uint8_t* plain, size_t len, const uint8_t* iv, const uint8_t* R, const uint8_t* key) {
  size_t xs = 0, ys = 0;
  while (xs < 32 && R[xs] == 0) ++xs;
  while (ys < 32 && R[32 + ys] == 0) ++ys;
  std::vector<uint8_t> out(iv, iv + 16);
  out.push_back(0x02), out.push_back(0xCA);
  out.push_back(0), out.push_back((uint8_t)(32 - xs));
  out.insert(out.end(), R + xs, R + 32);
  out.push_back(0), out.push_back((uint8_t)(32 - ys));
  out.insert(out.end(), R + 32 + ys, R + 64);
  bool good = false;
  const std::vector<uint8_t> ct = evp_cbc(true, key, iv, plain, len, good);
  out.insert(out.end(), ct.begin(), ct.end());
  uint8_t mac[32];
  unsigned ml = 0;
  HMAC(EVP_sha256(), key + 32, 32, out.data(), out.size(), mac, &ml);
  out.insert(out.end(), mac, mac + 32);
  return out;
}

static void test_vectors() {
  // FIPS-197 C.3
  const auto key = unhex("000102030405060708090a0b0c0d0e0f101112131415161718191a1b1c1d1e1f");
  const auto pt = unhex("00112233445566778899aabbccddeeff"), want = unhex("8ea2b7ca516745bfeafc49904b496089");
  uint32_t k[8], s[4], w[4], rk[60], dk[60];
  words(k, key.data(), 8);
  words(s, pt.data(), 4);
  words(w, want.data(), 4);
  aes::expand_key(rk, k, g_enc.te0);
  aes::encrypt_block(s, rk, g_enc.te0);
  CHECK(std::memcmp(s, w, 16) == 0, "FIPS-197 C.3 encrypt: %08x %08x %08x %08x", s[0], s[1], s[2], s[3]);
  aes::expand_dec_key(dk, k, g_dec);
  aes::decrypt_block(s, dk, g_dec);
  words(w, pt.data(), 4);
  CHECK(std::memcmp(s, w, 16) == 0, "FIPS-197 C.3 decrypt");
  // SP 800-38A F.2.5 and the padding block behind it
  const auto key2 = unhex("603deb1015ca71be2b73aef0857d77811f352c073b6108d72d9810a30914dff4");
  const auto iv2 = unhex("000102030405060708090a0b0c0d0e0f");
  const auto p2 = unhex("6bc1bee22e409f96e93d7e117393172aae2d8a571e03ac9c9eb76fac45af8e5130c81c46a35ce411e5fbc1191a0a52eff69f2445df4f9b17ad2b417be66c3710");
  const auto c2 = unhex("f58c4c04d6e5f1ba779eabfb5f7bfbd69cfc4e967edb808d679f777bc6702c7d39f23369a9d9bacfa530e26304231461b2eb05e2c39be9fcda6c19078c6a9d1b3f461796d6b0d6b2e0c2a72b4d80e644");
  uint32_t ivw[4];
  words(k, key2.data(), 8);
  words(ivw, iv2.data(), 4);
  Slot sl(80);
  std::memcpy(sl.p, p2.data(), 64);
  CHECK(sl::cbc_encrypt_row(sl.p, 64, k, ivw, g_enc.te0) == 80, "F.2.5 length");
  CHECK(std::memcmp(sl.p, c2.data(), 80) == 0, "F.2.5 ciphertext");
  CHECK(sl::cbc_decrypt_row(sl.p, 80, k, ivw, g_dec) == 64, "F.2.5 decrypt length");
  CHECK(std::memcmp(sl.p, p2.data(), 64) == 0, "F.2.5 plaintext");
}

static void test_cbc(std::mt19937_64& rng) {
  std::vector<size_t> lens;
  for (size_t l = 0; l <= 80; ++l) lens.push_back(l);
  for (size_t l : {255, 256, 257, 4095, 4096, 65537}) lens.push_back(l);
  for (size_t len : lens) {
    uint8_t key[32], iv[16];
    for (auto& b : key) b = (uint8_t)rng();
    for (auto& b : iv) b = (uint8_t)rng();
    std::vector<uint8_t> plain(len);
    for (auto& b : plain) b = (uint8_t)rng();
    bool good = false;
    const auto want = evp_cbc(true, key, iv, plain.data(), len, good);
    uint32_t k[8], ivw[4];
    words(k, key, 8);
    words(ivw, iv, 4);
    const size_t clen = bmseal::cbc_len(len);
    Slot sl(clen);
    if (len) std::memcpy(sl.p, plain.data(), len);
    CHECK(sl::cbc_encrypt_row(sl.p, (uint32_t)len, k, ivw, g_enc.te0) == clen, "cbc length at %zu", len);
    CHECK(want.size() == clen && std::memcmp(sl.p, want.data(), clen) == 0, "cbc encrypt at %zu", len);
    CHECK(sl::cbc_decrypt_row(sl.p, (uint32_t)clen, k, ivw, g_dec) == (int32_t)len, "cbc decrypt length at %zu", len);
    CHECK(len == 0 || std::memcmp(sl.p, plain.data(), len) == 0, "cbc decrypt at %zu", len);
  }
  // padding as EVP_DecryptFinal_ex judges it: random two-block ciphertexts, and constructed last bytes
  for (int t = 0; t < 600; ++t) {
    uint8_t key[32], iv[16], last[32];
    for (auto& b : key) b = (uint8_t)rng();
    for (auto& b : iv) b = (uint8_t)rng();
    for (auto& b : last) b = (uint8_t)rng();
    if (t % 3) {  // a chosen plaintext tail, encrypted without padding
      const int pad = (int)(rng() % 19);  // 0, 17, 18: refused
      for (int i = 0; i < 16 && i < pad; ++i) last[31 - i] = (uint8_t)pad;
      if (t % 3 == 2 && pad >= 2 && pad <= 16) last[32 - pad] ^= 1;  // unequal pad bytes
      EVP_CIPHER_CTX* c = EVP_CIPHER_CTX_new();
      int n1 = 0;
      uint8_t ct[48];
      EVP_EncryptInit_ex(c, EVP_aes_256_cbc(), nullptr, key, iv);
      EVP_CIPHER_CTX_set_padding(c, 0);
      EVP_EncryptUpdate(c, ct, &n1, last, 32);
      EVP_CIPHER_CTX_free(c);
      std::memcpy(last, ct, 32);
    }
    bool good = false;
    const auto want = evp_cbc(false, key, iv, last, 32, good);
    uint32_t k[8], ivw[4];
    words(k, key, 8);
    words(ivw, iv, 4);
    Slot sl(32);
    std::memcpy(sl.p, last, 32);
    const int32_t got = sl::cbc_decrypt_row(sl.p, 32, k, ivw, g_dec);
    CHECK(got == (good ? (int32_t)want.size() : -1), "padding verdict %d, libcrypto %d / %zu", got, (int)good, want.size());
    CHECK(!good || std::memcmp(sl.p, want.data(), want.size()) == 0, "plaintext beside a padding verdict");
  }
}

static void test_seal(std::mt19937_64& rng) {
  bool residue[64] = {}, head4[4] = {};
  std::vector<size_t> lens;
  for (size_t l = 0; l <= 64; ++l) lens.push_back(l);
  for (int strip = 0; strip <= 64; ++strip) {
    std::vector<size_t> ls = lens;
    if (strip % 16 == 0)
      for (size_t l : {200, 255, 256, 257, 2000, 4095, 4096, 65537, 262144}) ls.push_back(l);
    for (size_t len : ls) {
      uint8_t key[64], iv[16], R[64];
      for (auto& b : key) b = (uint8_t)rng();
      for (auto& b : iv) b = (uint8_t)rng();
      for (auto& b : R) b = (uint8_t)(rng() | 1);
      const int xs = strip < 32 ? strip : 32, ys = strip - xs;
      std::memset(R, 0, xs);
      std::memset(R + 32, 0, ys);
      std::vector<uint8_t> plain(len);
      for (auto& b : plain) b = (uint8_t)rng();
      const auto want = ref_seal(plain.data(), len, iv, R, key);
      const size_t slot = bmseal::seal_slot_bytes(len);
      CHECK(slot % 16 == 0 && slot >= SL_PLAIN_AT + bmseal::cbc_len(len) && slot >= want.size(), "slot of %zu", len);
      Slot sl(slot);
      if (len) std::memcpy(sl.p + SL_PLAIN_AT, plain.data(), len);
      uint32_t ke[8], km[8], ivw[4], X[8], Y[8];
      words(ke, key, 8);
      words(km, key + 32, 8);
      words(ivw, iv, 4);
      words(X, R, 8);
      words(Y, R + 32, 8);
      const uint32_t got = sl::seal_row(sl.p, (uint32_t)len, ke, km, ivw, X, Y, g_enc.te0);
      CHECK(got == want.size(), "blob length %u, libcrypto %zu (strip %d, len %zu)", got, want.size(), strip, len);
      CHECK(got == want.size() && std::memcmp(sl.p, want.data(), want.size()) == 0, "blob (strip %d, len %zu)", strip, len);
      residue[(want.size() - 32) % 64] = true;
      head4[(86 - strip) % 4] = true;
    }
  }
  CHECK(residue[55] && residue[56] && residue[63] && residue[0], "SHA-256 boundaries not all met");
  CHECK(head4[0] && head4[1] && head4[2] && head4[3], "head alignments not all met");
}

static void check_plan(const std::vector<uint64_t>& lens, uint64_t max_rows, uint64_t max_bytes, int64_t want_sets) {
  const size_t n = lens.size();
  std::vector<uint32_t> set(n);
  std::vector<uint64_t> off(n);
  const int64_t sets = bmseal::plan_seal(n, lens.data(), max_rows, max_bytes, set.data(), off.data());
  CHECK(sets == want_sets || want_sets < 0, "sets %lld, expected %lld (n %zu)", (long long)sets, (long long)want_sets, n);
  uint64_t rows = 0, end = 0;
  for (size_t i = 0; i < n; ++i) {
    const uint64_t slot = bmseal::seal_slot_bytes(lens[i]);
    if (i == 0 || set[i] != set[i - 1]) {
      CHECK(set[i] == (i ? set[i - 1] + 1 : 0), "set numbering at %zu", i);
      rows = 0, end = 0;
    }
    CHECK(off[i] % 16 == 0 && off[i] == end, "offset at %zu", i);
    end = off[i] + slot;
    ++rows;
    CHECK(rows <= max_rows, "rows in a set at %zu", i);
    CHECK(end <= max_bytes || rows == 1, "bytes in a set at %zu", i);
  }
  CHECK(n == 0 || (int64_t)set[n - 1] + 1 == sets, "last set");
}

static void test_plan() {
  const uint64_t R = 1u << 18, B = 256ull << 20;
  check_plan({}, R, B, 0);
  check_plan({0}, R, B, 1);
  check_plan({15}, R, B, 1);
  check_plan({16}, R, B, 1);
  check_plan(std::vector<uint64_t>(R, 16), R, B, 1);
  check_plan(std::vector<uint64_t>(R + 1, 16), R, B, 2);
  const uint64_t s200 = bmseal::seal_slot_bytes(200);
  check_plan(std::vector<uint64_t>(10, 200), R, 10 * s200, 1);      // the cap met exactly
  check_plan(std::vector<uint64_t>(10, 200), R, 10 * s200 - 1, 2);  // crossed by one byte
  check_plan(std::vector<uint64_t>(11, 200), R, 10 * s200, 2);
  check_plan({300000, 16, 16}, R, 1000, 2);   // a row alone above the cap, the small ones behind it
  check_plan({16, 300000, 16}, R, 1000, 3);
  check_plan({bmseal::kMaxPlain, bmseal::kMaxPlain, 0}, R, B, 3);
  std::vector<uint32_t> set(1);
  std::vector<uint64_t> off(1);
  const uint64_t over = bmseal::kMaxPlain + 1, fine = 5;
  CHECK(bmseal::plan_seal(1, &over, R, B, set.data(), off.data()) == bmseal::kPlanBadArg, "length above the bound");
  CHECK(bmseal::plan_seal(1, &fine, 0, B, set.data(), off.data()) == bmseal::kPlanBadArg, "zero row limit");
  CHECK(bmseal::plan_seal(1, &fine, R, 0, set.data(), off.data()) == bmseal::kPlanBadArg, "zero byte limit");
  CHECK(bmseal::plan_seal(1, nullptr, R, B, set.data(), off.data()) == bmseal::kPlanBadArg, "null lengths");
  const uint64_t odd = 24;
  CHECK(bmseal::plan_slots(1, &odd, R, B, set.data(), off.data()) == bmseal::kPlanBadArg, "slot no multiple of 16");
}

// cut_sets over plan_slots at limits of max_rows rows and max_bytes: begin[] strictly increasing and ending at
// n, one set index per set, and max_rows / max_pool against a naive recomputation
static void check_cut(const std::vector<uint64_t>& slots, uint64_t max_rows, uint64_t max_bytes) {
  const size_t n = slots.size();
  std::vector<uint32_t> set(n);
  std::vector<uint64_t> off(n);
  CHECK(bmseal::plan_slots(n, slots.data(), max_rows, max_bytes, set.data(), off.data()) >= 0, "plan refused (n %zu)", n);
  const bmseal::Sets s = bmseal::cut_sets(set, off, slots);
  CHECK(!s.begin.empty() && s.begin.back() == n && s.begin.front() == 0, "begin[] ends (n %zu)", n);
  CHECK(s.count() == (n ? (size_t)set[n - 1] + 1 : 0), "set count %zu (n %zu)", s.count(), n);
  size_t want_rows = 0;
  uint64_t want_pool = 16;
  for (size_t k = 0; k + 1 < s.begin.size(); ++k) {
    const size_t i0 = s.begin[k], i1 = s.begin[k + 1];
    CHECK(i0 < i1 && i1 <= n, "begin[] strictly increasing at set %zu", k);
    if (!(i0 < i1 && i1 <= n)) return;
    uint64_t pool = 0;
    for (size_t i = i0; i < i1; ++i) {
      CHECK(set[i] == set[i0], "rows of set %zu share one index", k);
      pool += slots[i];
    }
    CHECK(i1 == n || set[i1] != set[i0], "set %zu ends where the index changes", k);
    want_rows = std::max(want_rows, i1 - i0);
    want_pool = std::max(want_pool, pool);
  }
  CHECK(s.max_rows == want_rows, "max_rows %zu, naive %zu (n %zu)", s.max_rows, want_rows, n);
  CHECK(s.max_pool == want_pool, "max_pool %llu, naive %llu (n %zu)", (unsigned long long)s.max_pool,
        (unsigned long long)want_pool, n);
  // the same plan through SlotPlan
  bmseal::SlotPlan p;
  p.slot = slots;
  CHECK(p.plan(max_rows, max_bytes) && p.sets.begin == s.begin && p.sets.max_pool == s.max_pool, "SlotPlan (n %zu)", n);
  for (size_t k = 0; k < p.sets.count(); ++k) {
    uint64_t pool = 0;
    for (size_t i = s.begin[k]; i < s.begin[k + 1]; ++i) pool += slots[i];
    CHECK(p.pool_bytes(k) == pool, "pool_bytes of set %zu", k);
  }
}

static void test_cut_sets() {
  const uint64_t R = 4, B = 64;  // tiny limits: 4 rows / 64 bytes
  check_cut({}, R, B);
  check_cut({16}, R, B);
  check_cut({16, 16, 16, 16}, R, B);      // exactly one set, by rows and by bytes
  check_cut({16, 16, 16, 16, 16}, R, B);  // one row over
  check_cut({32, 32}, R, B);              // exactly one set by bytes
  check_cut({32, 32, 16}, R, B);          // 16 bytes over
  check_cut({0, 0, 0, 0, 0}, R, B);       // empty slots still count as rows
  check_cut({80, 16, 16}, R, B);          // a row alone above the byte limit
  check_cut({16, 80, 16}, R, B);
  std::mt19937_64 rng(20261021);
  for (int t = 0; t < 1000; ++t) {
    std::vector<uint64_t> slots(rng() % 24);
    for (auto& s : slots) s = 16 * (rng() % 6);  // 0 .. 80: some alone above the limit
    check_cut(slots, R, B);
  }
}

int main() {
  aes::fill_enc(g_enc, 0, 1);
  aes::fill_dec(g_dec, 0, 1);
  std::mt19937_64 rng(20261020);
  test_vectors();
  test_cbc(rng);
  test_seal(rng);
  test_plan();
  test_cut_sets();
  if (g_fail) return 1;
  std::fprintf(stderr, "all seal checks passed\n");
  return 0;
}
