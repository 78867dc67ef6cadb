// rxobjopen_sim.cpp -- the host-only row and table code of bmpow_rx_sealed_objects
// (pybitmessage_amd/csrc/bmpow_rxobjopen_tab.h, bmpow_rxopen_rows.h) as a stand-alone program:
// tests/test_rxobjopen.py builds it with g++ under AddressSanitizer + UBSan and runs it.
//   * the tag table with no entry, one entry, entries that repeat a tag, and tags that collide in every slot the
//     hash can give (the same first eight bytes), each in a heap block of exactly its size;
//   * the routing of one object's head: every kind, version and length around the floors the reference has;
//   * rxs::open_row over a pool of slots laid side by side as the host unit lays the object family's out (clen
//     bytes each, poff the running sum), from ciphertexts at every alignment, against libcrypto: that no row
//     touches a neighbour's slot.  (The row function alone: rxo_row and the kernel's lane function are device
//     code and run in tests/test_gpu_rxobjopen.py.)
// Loads neither HIP nor the library.
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
struct uint4 {
  uint32_t x, y, z, w;
};
#define BM_DEV [[maybe_unused]] static inline

#include "bmpow_rxobjopen_tab.h"
#include "bmpow_rxopen_rows.h"

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

static std::mt19937_64 g_rng(20261021);
static void fill_random(uint8_t* p, size_t n) {
  for (size_t i = 0; i < n; ++i) p[i] = (uint8_t)g_rng();
}

struct Heap {  // exactly n bytes: the sanitizer's red zones lie on either side
  uint8_t* p;
  size_t n;
  Heap(size_t align, size_t n_) : p(n_ ? (uint8_t*)std::aligned_alloc(align, (n_ + align - 1) / align * align) : nullptr), n(n_) {
    if (p) std::memset(p, 0xA5, n);
  }
  ~Heap() { std::free(p); }
  Heap(const Heap&) = delete;
};

// ------------------------------------------------------------------ the tag table
static void test_tag_table() {
  using bmhost::TagTable;
  uint8_t probe[32];
  fill_random(probe, 32);
  {
    TagTable none(nullptr, 0);
    CHECK(none.find(probe) == -1, "an empty table finds nothing");
  }
  {
    std::vector<uint8_t> one(32);  // a vector of exactly 32 bytes: reading past it is an error
    fill_random(one.data(), 32);
    TagTable t(one.data(), 1);
    CHECK(t.find(one.data()) == 0, "one entry is found");
    CHECK(t.find(probe) == -1, "another tag is not");
    uint8_t near[32];
    std::memcpy(near, one.data(), 32);
    near[31] ^= 1;
    CHECK(t.find(near) == -1, "a tag that differs in its last byte is not");
  }
  for (size_t n : {2u, 3u, 4u, 5u, 63u, 64u, 65u, 1000u}) {
    // every tag has the same first eight bytes: they all hash to one slot and probe along
    std::vector<uint8_t> tags(32 * n);
    fill_random(tags.data(), tags.size());
    for (size_t i = 1; i < n; ++i) std::memcpy(tags.data() + 32 * i, tags.data(), 8);
    // entries n/2 .. repeat the tags of entries 0 ..: the first entry wins
    for (size_t i = n / 2; i < n; ++i) std::memcpy(tags.data() + 32 * i, tags.data() + 32 * (i - n / 2), 32);
    TagTable t(tags.data(), n);
    for (size_t i = 0; i < n; ++i) {
      int32_t want = 0;  // the first entry with this tag, by looking at them all
      while (std::memcmp(tags.data() + 32 * (size_t)want, tags.data() + 32 * i, 32) != 0) ++want;
      CHECK(t.find(tags.data() + 32 * i) == want, "n %zu: entry %zu found as %d, want %d", n, i, t.find(tags.data() + 32 * i), want);
    }
    uint8_t miss[32];
    std::memcpy(miss, tags.data(), 32);
    miss[20] ^= 0x40;  // collides with everything, equals nothing
    CHECK(t.find(miss) == -1, "n %zu: a colliding tag that is not there", n);
    CHECK(t.find(probe) == -1, "n %zu: a random tag", n);
  }
  {  // random tags, all different
    const size_t n = 4096;
    std::vector<uint8_t> tags(32 * n);
    fill_random(tags.data(), tags.size());
    TagTable t(tags.data(), n);
    for (size_t i = 0; i < n; ++i) CHECK(t.find(tags.data() + 32 * i) == (int32_t)i, "random entry %zu", i);
  }
}

// ------------------------------------------------------------------ the routing of a head
static std::vector<uint8_t> object(uint8_t type, std::vector<uint8_t> version, std::vector<uint8_t> stream, size_t len) {
  std::vector<uint8_t> o(20);
  fill_random(o.data(), 16);
  o[19] = type;
  o.insert(o.end(), version.begin(), version.end());
  o.insert(o.end(), stream.begin(), stream.end());
  while (o.size() < len) o.push_back((uint8_t)g_rng());
  o.resize(len);
  return o;
}

static bmhost::RouteClass route(int kind, const std::vector<uint8_t>& o, bmpow_rx_obj_rec& rec) {
  Heap h(1, o.size());  // exactly the object's bytes
  if (!o.empty()) std::memcpy(h.p, o.data(), o.size());
  return bmhost::route_object(kind, h.p, o.size(), rec);
}

static void test_routing() {
  using namespace bmhost;
  bmpow_rx_obj_rec rec;
  // broadcasts: versions 3 .. 6, a varint that does not decode, a tag the end cuts
  CHECK(route(BMPOW_RXO_KIND_BROADCAST, object(3, {3}, {1}, 400), rec) == ROUTE_DONE && rec.status == BMPOW_RXO_BC_VERSION, "v3");
  CHECK(route(BMPOW_RXO_KIND_BROADCAST, object(3, {6}, {1}, 400), rec) == ROUTE_DONE && rec.status == BMPOW_RXO_BC_VERSION, "v6");
  CHECK(route(BMPOW_RXO_KIND_BROADCAST, object(3, {0xfd, 0, 4}, {1}, 400), rec) == ROUTE_DONE && rec.status == BMPOW_RXO_VARINT, "varint");
  CHECK(route(BMPOW_RXO_KIND_BROADCAST, object(3, {4}, {1}, 400), rec) == ROUTE_TRIAL && rec.payload_off == 22 && rec.tag_off == 22, "v4");
  CHECK(route(BMPOW_RXO_KIND_BROADCAST, object(3, {5}, {1}, 400), rec) == ROUTE_TAG && rec.payload_off == 54 && rec.tag_off == 22, "v5");
  CHECK(route(BMPOW_RXO_KIND_BROADCAST, object(3, {5}, {0xff, 0, 0, 0, 1, 0, 0, 0, 0}, 400), rec) == ROUTE_TAG && rec.payload_off == 62, "v5 wide");
  for (size_t len = 0; len < 60; ++len) {
    const RouteClass c = route(BMPOW_RXO_KIND_BROADCAST, object(3, {5}, {1}, len), rec);
    // a varint read where the object has ended is 0, as the reference's decodeVarint gives it: 21 bytes are a head
    CHECK(len < 21 ? c == ROUTE_DONE : len < 54 ? c == ROUTE_NO_TAG : c == ROUTE_TAG, "v5 of %zu bytes routed %d", len, (int)c);
    const RouteClass d = route(BMPOW_RXO_KIND_BROADCAST, object(3, {4}, {1}, len), rec);
    CHECK(len < 21 ? d == ROUTE_DONE : d == ROUTE_TRIAL, "v4 of %zu bytes routed %d", len, (int)d);
  }
  // pubkeys: the version decides; 4 goes to the encrypted kind, with :411's floor
  for (size_t len : {0u, 19u, 20u, 21u, 22u, 53u, 54u, 145u, 146u, 169u, 170u, 349u, 350u, 351u, 1000u}) {
    const RouteClass c = route(BMPOW_RXO_KIND_PUBKEY, object(1, {4}, {1}, len), rec);
    if (len < 21) {  // no version byte: version 0
      CHECK(c == ROUTE_DONE && rec.kind == BMPOW_RXO_KIND_PUBKEY && rec.status != BMPOW_RXO_OK, "v4 pubkey of %zu bytes", len);
    } else {
      CHECK(c == (len < 350 ? ROUTE_V4_SHORT : ROUTE_NEEDED) && rec.kind == BMPOW_RXO_KIND_PUBKEY_V4, "v4 pubkey of %zu bytes routed %d",
            len, (int)c);
      CHECK(rec.tag_off == (len < 22 ? len : 22) && rec.payload_off == (len < 54 ? len : 54), "v4 pubkey of %zu bytes: offsets", len);
    }
    for (uint8_t v : {0, 1, 2, 3, 5}) {
      const RouteClass p = route(BMPOW_RXO_KIND_PUBKEY, object(1, {v}, {1}, len), rec);
      CHECK(rec.kind == BMPOW_RXO_KIND_PUBKEY && (p == ROUTE_DONE || p == ROUTE_CLEAR), "clear pubkey v%d of %zu bytes", v, len);
      CHECK((p == ROUTE_CLEAR) == (rec.status == BMPOW_RXO_OK), "clear pubkey v%d of %zu bytes: class and status", v, len);
    }
  }
}

// ------------------------------------------------------------------ the opening row code over object slots
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

static void words(uint32_t* w, const uint8_t* b, int n) {
  for (int i = 0; i < n; ++i) w[i] = (uint32_t)b[4 * i] << 24 | (uint32_t)b[4 * i + 1] << 16 | (uint32_t)b[4 * i + 2] << 8 | b[4 * i + 3];
}

// The rows of one set as bmpow_host_rxobjopen.hip lays them out: MAC pool rows of nblk * 64 bytes side by side,
// plaintext slots of clen bytes side by side (poff a multiple of 16), both pools of exactly their size.
static void test_open_rows() {
  static aes::DecTab dec;
  aes::fill_dec(dec, 0, 1);
  struct Row {
    uint32_t blk, body_off, clen;
    uint64_t poff;
    uint8_t key[32];
    std::vector<uint8_t> plain;
  };
  std::vector<Row> rows;
  uint32_t blk = 0;
  uint64_t poff = 0;
  // body_off 22 .. 86 gives every alignment several times; plaintexts around the 16- and 64-byte boundaries
  for (uint32_t body_off = 22; body_off <= 86; ++body_off)
    for (uint32_t plen : {0u, 1u, 15u, 16u, 17u, 47u, 48u, 63u, 64u, 65u, 200u}) {
      Row r;
      r.blk = blk, r.body_off = body_off, r.poff = poff;
      r.clen = 16 * (plen / 16 + 1);
      fill_random(r.key, 32);
      r.plain.resize(plen);
      fill_random(r.plain.data(), plen);
      blk += (body_off + r.clen + 9 + 63) / 64;
      poff += r.clen;
      rows.push_back(r);
    }
  Heap pool(64, (size_t)blk * 64), slots(16, poff);
  for (Row& r : rows) {
    uint8_t* row = pool.p + 64ull * r.blk;
    fill_random(row, r.body_off);  // the IV and the head
    bool good = false;
    const std::vector<uint8_t> ct = evp_cbc(true, r.key, row, r.plain.data(), r.plain.size(), good);
    CHECK(good && ct.size() == r.clen, "libcrypto encrypts %zu bytes", r.plain.size());
    std::memcpy(row + r.body_off, ct.data(), r.clen);
  }
  for (const Row& r : rows) {
    uint32_t k[8], iv[4];
    words(k, r.key, 8);
    words(iv, pool.p + 64ull * r.blk, 4);
    const int32_t got = rxs::open_row(pool.p + 64ull * r.blk + r.body_off, r.clen, k, iv, slots.p + r.poff, dec);
    CHECK(got == (int32_t)r.plain.size(), "body_off %u, %zu bytes: length %d", r.body_off, r.plain.size(), got);
  }
  for (const Row& r : rows) {  // after every row ran: no slot was touched by a neighbour
    CHECK(r.plain.empty() || std::memcmp(slots.p + r.poff, r.plain.data(), r.plain.size()) == 0, "body_off %u, %zu bytes: the slot", r.body_off, r.plain.size());
    for (size_t i = r.plain.size(); i < r.clen; ++i) CHECK(slots.p[r.poff + i] == 0, "zeros behind the plaintext");
  }
}

int main() {
  test_tag_table();
  test_routing();
  test_open_rows();
  if (g_fail) {
    std::fprintf(stderr, "%d rxobjopen checks failed\n", g_fail);
    return 1;
  }
  std::fprintf(stderr, "all rxobjopen checks passed (%ld checks)\n", g_checks);
  return 0;
}
