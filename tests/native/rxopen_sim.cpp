// rxopen_sim.cpp -- the opening kernel's per-row code (pybitmessage_amd/csrc/bmpow_rxopen_rows.h,
// aes256_dev.h) on the host, as a stand-alone program: tests/test_rxopen.py builds it with g++ under
// AddressSanitizer + UBSan and runs it.  The ciphertext lies in a heap row laid out as the MAC pool lays it
// out -- on a 64-byte boundary, the IV and a head of body_off bytes in front, the SHA padding behind, exactly
// nblk * 64 bytes -- so a byte read in front of or behind the row is an error; the plaintext goes to a heap slot
// of exactly clen bytes, and once more to a slot between two sentinels.  The results are compared with
// libcrypto's EVP calls.  Loads neither HIP nor the library.
#include <openssl/evp.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

// the two gfx950 builtins the included headers use, restated for the host
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

#include "bmpow_rxopen_rows.h"

static int g_fail = 0;
static long g_rows = 0;
#define CHECK(cond, ...)                                        \
  do {                                                          \
    if (!(cond)) {                                              \
      std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
      std::fprintf(stderr, __VA_ARGS__);                        \
      std::fputc('\n', stderr);                                 \
      if (++g_fail > 20) std::exit(1);                          \
    }                                                           \
  } while (0)

static aes::DecTab g_dec;
static std::mt19937_64 g_rng(20261020);

static void words(uint32_t* w, const uint8_t* b, int n) {
  for (int i = 0; i < n; ++i) w[i] = (uint32_t)b[4 * i] << 24 | (uint32_t)b[4 * i + 1] << 16 | (uint32_t)b[4 * i + 2] << 8 | b[4 * i + 3];
}

static void fill_random(uint8_t* p, size_t n) {
  for (size_t i = 0; i < n; ++i) p[i] = (uint8_t)g_rng();
}

// AES-256-CBC by libcrypto; pad: PKCS#7 on (the reference's cipher) or off (to craft any last block)
static std::vector<uint8_t> evp_cbc(bool enc, bool pad, const uint8_t* key, const uint8_t* iv, const uint8_t* in, size_t len,
                                    bool& good) {
  std::vector<uint8_t> out(len + 32);
  EVP_CIPHER_CTX* c = EVP_CIPHER_CTX_new();
  int n1 = 0, n2 = 0;
  const uint8_t none = 0;
  good = EVP_CipherInit_ex(c, EVP_aes_256_cbc(), nullptr, key, iv, enc ? 1 : 0) == 1 &&
         EVP_CIPHER_CTX_set_padding(c, pad ? 1 : 0) == 1 &&
         EVP_CipherUpdate(c, out.data(), &n1, len ? in : &none, (int)len) == 1 && EVP_CipherFinal_ex(c, out.data() + n1, &n2) == 1;
  EVP_CIPHER_CTX_free(c);
  out.resize(good ? (size_t)(n1 + n2) : 0);
  return out;
}

struct Heap {  // exactly n bytes on an `align` boundary: the sanitizer's red zones lie on either side
  uint8_t* p;
  Heap(size_t align, size_t n) : p((uint8_t*)std::aligned_alloc(align, n)) { std::memset(p, 0xA5, n); }
  ~Heap() { std::free(p); }
  Heap(const Heap&) = delete;
};

// One ciphertext at body_off of a pool row, opened into both kinds of slot; want: libcrypto's plaintext, or
// nullptr where it refuses the padding.
static void open_once(const std::vector<uint8_t>& ct, uint32_t body_off, const uint8_t* key, const uint8_t* iv,
                      const std::vector<uint8_t>* want, const char* what) {
  const uint32_t clen = (uint32_t)ct.size(), maced = body_off + clen, nblk = (maced + 9 + 63) / 64;
  Heap row(64, (size_t)nblk * 64);  // as pad_mac_blocks lays it out
  std::memcpy(row.p, iv, 16);
  fill_random(row.p + 16, body_off - 16);
  std::memcpy(row.p + body_off, ct.data(), clen);
  row.p[maced] = 0x80;
  std::memset(row.p + maced + 1, 0, (size_t)nblk * 64 - maced - 1 - 8);
  const uint64_t bits = (uint64_t)(64 + maced) * 8;
  for (int j = 0; j < 8; ++j) row.p[(size_t)nblk * 64 - 8 + j] = (uint8_t)(bits >> (56 - 8 * j));
  const std::vector<uint8_t> before(row.p, row.p + (size_t)nblk * 64);

  uint32_t k[8], ivw[4];
  words(k, key, 8);
  words(ivw, row.p, 4);
  std::vector<uint8_t> expect(clen, 0);
  if (want) std::memcpy(expect.data(), want->data(), want->size());
  const int32_t want_len = want ? (int32_t)want->size() : -1;

  Heap slot(16, clen);
  const int32_t got = rxs::open_row(row.p + body_off, clen, k, ivw, slot.p, g_dec);
  CHECK(got == want_len, "%s: length %d, want %d (body_off %u, clen %u)", what, got, want_len, body_off, clen);
  CHECK(std::memcmp(slot.p, expect.data(), clen) == 0, "%s: slot bytes (body_off %u, clen %u)", what, body_off, clen);

  Heap guarded(16, (size_t)clen + 32);  // sentinel | slot | sentinel
  const int32_t again = rxs::open_row(row.p + body_off, clen, k, ivw, guarded.p + 16, g_dec);
  CHECK(again == want_len, "%s: length %d the second time", what, again);
  CHECK(std::memcmp(guarded.p + 16, expect.data(), clen) == 0, "%s: guarded slot bytes", what);
  for (int i = 0; i < 16; ++i)
    CHECK(guarded.p[i] == 0xA5 && guarded.p[16 + clen + i] == 0xA5, "%s: a byte outside the slot changed (clen %u)", what, clen);
  CHECK(std::memcmp(row.p, before.data(), before.size()) == 0, "%s: the pool row changed", what);
  ++g_rows;
}

// the body_off in 22 .. 37 whose residue mod 16 is a: the row starts on a 64-byte boundary, so that is the
// ciphertext's alignment
static uint32_t body_off_for(uint32_t a) { return 22 + ((a + 16 - 22 % 16) % 16); }

static void test_good_padding() {
  static const uint32_t kBlocks[] = {1, 2, 3, 4, 5, 17};
  uint8_t key[32], iv[16];
  for (uint32_t a = 0; a < 16; ++a)
    for (uint32_t nb : kBlocks)
      for (uint32_t len = 16 * (nb - 1); len < 16 * nb; ++len) {  // every length mod 16: pad 16 .. 1; 0 is the empty one
        fill_random(key, 32), fill_random(iv, 16);
        std::vector<uint8_t> plain(len);
        fill_random(plain.data(), len);
        bool good = false;
        const std::vector<uint8_t> ct = evp_cbc(true, true, key, iv, plain.data(), len, good);
        CHECK(good && ct.size() == 16 * nb, "libcrypto encrypts %u bytes", len);
        const std::vector<uint8_t> back = evp_cbc(false, true, key, iv, ct.data(), ct.size(), good);
        CHECK(good && back == plain, "libcrypto decrypts its own ciphertext");
        open_once(ct, body_off_for(a), key, iv, &back, "good padding");
      }
  // every head length there is, once: 22 + xl + yl with xl, yl in 0 .. 32
  for (uint32_t body_off = 22; body_off <= 86; ++body_off) {
    fill_random(key, 32), fill_random(iv, 16);
    std::vector<uint8_t> plain(200 + body_off);
    fill_random(plain.data(), plain.size());
    bool good = false;
    const std::vector<uint8_t> ct = evp_cbc(true, true, key, iv, plain.data(), plain.size(), good);
    open_once(ct, body_off, key, iv, &plain, "every head");
  }
}

// a ciphertext whose plaintext is `blocks` as it stands (no padding added), and libcrypto's verdict on it
static void open_crafted(const std::vector<uint8_t>& blocks, uint32_t a, const char* what, bool must_refuse) {
  uint8_t key[32], iv[16];
  fill_random(key, 32), fill_random(iv, 16);
  bool good = false;
  const std::vector<uint8_t> ct = evp_cbc(true, false, key, iv, blocks.data(), blocks.size(), good);
  CHECK(good && ct.size() == blocks.size(), "libcrypto encrypts without padding");
  const std::vector<uint8_t> back = evp_cbc(false, true, key, iv, ct.data(), ct.size(), good);
  CHECK(good != must_refuse, "%s: libcrypto's verdict", what);
  open_once(ct, body_off_for(a), key, iv, good ? &back : nullptr, what);
}

static void test_bad_padding() {
  for (uint32_t a = 0; a < 16; ++a)
    for (uint32_t nb : {1u, 3u}) {
      std::vector<uint8_t> blocks(16 * nb);
      for (uint32_t last : {0u, 17u, 0xffu}) {
        fill_random(blocks.data(), blocks.size());
        blocks.back() = (uint8_t)last;
        open_crafted(blocks, a, "last byte out of range", true);
      }
      for (uint32_t pad = 1; pad <= 16; ++pad) {
        fill_random(blocks.data(), blocks.size());
        if (pad < 16) blocks[blocks.size() - pad - 1] = 0x55;  // not a longer run of pad bytes by chance
        std::memset(blocks.data() + blocks.size() - pad, (int)pad, pad);
        open_crafted(blocks, a, "well padded by hand", false);
        for (uint32_t at = 1; at < pad; ++at) {  // one wrong pad byte at each position in front of the last
          std::vector<uint8_t> bad = blocks;
          bad[bad.size() - 1 - at] ^= (uint8_t)(1u << (at % 8));
          open_crafted(bad, a, "one wrong pad byte", true);
        }
      }
    }
}

int main() {
  aes::fill_dec(g_dec, 0, 1);
  test_good_padding();
  test_bad_padding();
  if (g_fail) {
    std::fprintf(stderr, "%d rxopen checks failed\n", g_fail);
    return 1;
  }
  std::fprintf(stderr, "all rxopen checks passed (%ld rows)\n", g_rows);
  return 0;
}
