// ident_sim.cpp -- the byte-oriented half of the sender identification (pybitmessage_amd/csrc/
// bmpow_ident_fmt.h: varints, encodeAddress's zero-byte rule, base58) on the CPU, composed as the kernel's
// id_finish composes it, with libcrypto's SHA-512 where the device runs its own compression.
//
// A stand-alone program: g++ -fsanitize=address,undefined, its own main, loaded into nothing.
//   ident_sim ROWS.txt      one row per line:
//       A <version> <stream> <ripe hex, 40 digits> <address without BM->
//       V <value> <varint hex>
// On top of the rows it checks the conversion against a byte-wise long division for every string length
// 0 .. 42 with leading zero bytes, and the SHA-512 block against padding written out by hand.
#include <openssl/sha.h>

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "bmpow_ident_fmt.h"

namespace {

int g_fail = 0;
#define CHECK(cond, ...)                          \
  do {                                            \
    if (!(cond)) {                                \
      std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
      std::fprintf(stderr, __VA_ARGS__);          \
      std::fputc('\n', stderr);                   \
      ++g_fail;                                   \
    }                                             \
  } while (0)

std::vector<uint8_t> bytes_of(const idf::msg& m) {
  std::vector<uint8_t> out(m.len);
  for (uint32_t i = 0; i < m.len; ++i) out[i] = (uint8_t)(m.w[i >> 3] >> (56 - 8 * (i & 7)));
  return out;
}

bool zero_behind(const idf::msg& m) {
  for (uint32_t i = m.len; i < 8 * idf::kMsgWords; ++i)
    if ((uint8_t)(m.w[i >> 3] >> (56 - 8 * (i & 7)))) return false;
  return true;
}

std::vector<uint8_t> unhex(const std::string& s) {
  std::vector<uint8_t> out(s.size() / 2);
  for (size_t i = 0; i < out.size(); ++i) out[i] = (uint8_t)std::strtoul(s.substr(2 * i, 2).c_str(), nullptr, 16);
  return out;
}

std::string chars_of(uint32_t n, const uint32_t (&s)[idf::kMaxChars / 4]) {
  std::string out;
  for (uint32_t i = 0; i < (uint32_t)idf::kMaxChars; ++i) {
    const char c = (char)(s[i >> 2] >> (24 - 8 * (i & 3)));
    if (i < n) out.push_back(c);
    else CHECK(c == 0, "character %u behind the last is not zero", i);
  }
  return out;
}

// encodeBase58(int.from_bytes(data, 'big')) by long division of the byte string
std::string base58_ref(std::vector<uint8_t> v) {
  static const char* kAlphabet = "123456789ABCDEFGHJKLMNPQRSTUVWXYZabcdefghijkmnopqrstuvwxyz";
  std::string out;
  for (;;) {
    uint32_t rem = 0;
    bool any = false;
    for (uint8_t& b : v) {
      const uint32_t x = rem * 256 + b;
      b = (uint8_t)(x / 58);
      rem = x % 58;
      any = any || b;
    }
    out.insert(out.begin(), kAlphabet[rem]);
    if (!any) return out;
  }
}

// the SHA-512 of the string, through the block sha512_block builds: the block must be the padding
// FIPS 180-4 prescribes for these bytes
void sha512_of(const idf::msg& m, uint8_t digest[64]) {
  uint64_t w[16];
  idf::sha512_block(m, w);
  const std::vector<uint8_t> data = bytes_of(m);
  uint8_t want[128] = {0};
  if (!data.empty()) std::memcpy(want, data.data(), data.size());
  want[data.size()] = 0x80;
  const uint64_t bits = 8ull * data.size();
  for (int i = 0; i < 8; ++i) want[120 + i] = (uint8_t)(bits >> (56 - 8 * i));
  for (int i = 0; i < 128; ++i)
    CHECK((uint8_t)(w[i >> 3] >> (56 - 8 * (i & 7))) == want[i], "block byte %d of a %zu-byte string", i, data.size());
  SHA512(data.data(), data.size(), digest);
}

// id_finish's address: the record's addr_len and addr
std::string address(uint64_t version, uint64_t stream, const uint8_t ripe[20]) {
  uint32_t rh[5];
  for (int i = 0; i < 5; ++i)
    rh[i] = ripe[4 * i] | (uint32_t)ripe[4 * i + 1] << 8 | (uint32_t)ripe[4 * i + 2] << 16 | (uint32_t)ripe[4 * i + 3] << 24;
  idf::msg data;
  idf::put_address_data(data, version, stream, rh, idf::strip_count(version, rh));
  CHECK(zero_behind(data), "bytes behind the string");
  uint8_t d1[64], d2[64];
  sha512_of(data, d1);
  SHA512(d1, 64, d2);
  idf::put_be32(data, (uint32_t)d2[0] << 24 | (uint32_t)d2[1] << 16 | (uint32_t)d2[2] << 8 | d2[3]);
  uint32_t s[idf::kMaxChars / 4], field[16];
  const uint32_t n = idf::base58(data, s);
  const std::string chars = chars_of(n, s);
  CHECK(chars == base58_ref(bytes_of(data)), "base58 differs from the long division");
  idf::address_field(n, s, field);
  uint8_t rec[64];
  std::memcpy(rec, field, 64);  // the device stores these words as they are (little-endian)
  CHECK(rec[0] == n, "addr_len");
  for (uint32_t i = 0; i < 63; ++i) CHECK(rec[1 + i] == (i < n ? (uint8_t)chars[i] : 0), "addr[%u]", i);
  return chars;
}

void self_checks() {
  // every length 0 .. 42, every count of leading zero bytes, a few fillings
  uint64_t x = 0x9e3779b97f4a7c15ull;
  for (uint32_t len = 0; len <= 42; ++len)
    for (uint32_t zeros = 0; zeros <= len; ++zeros)
      for (int fill = 0; fill < 3; ++fill) {
        idf::msg m;
        idf::clear(m);
        std::vector<uint8_t> v;
        for (uint32_t i = 0; i < len; ++i) {
          x = x * 6364136223846793005ull + 1442695040888963407ull;
          const uint8_t b = i < zeros ? 0 : fill == 0 ? 0xff : fill == 1 ? 1 : (uint8_t)(x >> 56);
          idf::put_byte(m, b);
          v.push_back(b);
        }
        CHECK(bytes_of(m) == v && zero_behind(m), "put_byte at length %u", len);
        uint32_t s[idf::kMaxChars / 4];
        const uint32_t n = idf::base58(m, s);
        const std::string got = chars_of(n, s), want = base58_ref(v);
        CHECK(got == want, "base58 len %u zeros %u fill %d: %s != %s", len, zeros, fill, got.c_str(), want.c_str());
        uint8_t d[64];
        sha512_of(m, d);
      }
  static const char* kAlphabet = "123456789ABCDEFGHJKLMNPQRSTUVWXYZabcdefghijkmnopqrstuvwxyz";
  for (uint32_t d = 0; d < 58; ++d) CHECK(idf::base58_char(d) == (uint32_t)kAlphabet[d], "digit %u", d);
  // the zero-byte rule: every count of leading zeros under every kind of version
  for (uint32_t zeros = 0; zeros <= 20; ++zeros) {
    uint8_t ripe[20];
    for (uint32_t i = 0; i < 20; ++i) ripe[i] = i < zeros ? 0 : (uint8_t)(i + 1);
    uint32_t rh[5];
    std::memcpy(rh, ripe, 20);
    const uint64_t versions[] = {0, 1, 2, 3, 4, 5, 252, 253, ~0ull};
    for (uint64_t v : versions) {
      const uint32_t want = (v == 2 || v == 3) ? (zeros < 2 ? zeros : 2) : v == 4 ? zeros : 0;
      CHECK(idf::strip_count(v, rh) == want, "strip_count version %" PRIu64 " zeros %u", v, zeros);
    }
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: ident_sim ROWS.txt\n");
    return 2;
  }
  self_checks();
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) {
    std::fprintf(stderr, "cannot open %s\n", argv[1]);
    return 2;
  }
  char kind[4], a[64], b[64], c[128], d[128];
  int rows = 0;
  while (std::fscanf(f, "%3s", kind) == 1) {
    if (kind[0] == 'A' && std::fscanf(f, "%63s %63s %127s %127s", a, b, c, d) == 4) {
      const std::vector<uint8_t> ripe = unhex(c);
      CHECK(ripe.size() == 20, "ripe of %zu bytes", ripe.size());
      if (ripe.size() != 20) continue;
      const std::string got = address(std::strtoull(a, nullptr, 10), std::strtoull(b, nullptr, 10), ripe.data());
      CHECK(got == d, "address v%s s%s %s: %s != %s", a, b, c, got.c_str(), d);
    } else if (kind[0] == 'V' && std::fscanf(f, "%63s %127s", a, c) == 2) {
      idf::msg m;
      idf::clear(m);
      idf::put_varint(m, std::strtoull(a, nullptr, 10));
      CHECK(bytes_of(m) == unhex(c) && zero_behind(m), "varint %s", a);
    } else {
      CHECK(false, "malformed row %d", rows);
      break;
    }
    ++rows;
  }
  std::fclose(f);
  if (g_fail) {
    std::fprintf(stderr, "%d checks failed\n", g_fail);
    return 1;
  }
  std::fprintf(stderr, "all ident checks passed (%d rows)\n", rows);
  return 0;
}
