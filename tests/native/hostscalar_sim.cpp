// hostscalar_sim.cpp -- the host units' scalar and byte toolkit (pybitmessage_amd/csrc/bmpow_host_scalar.h) as
// a stand-alone program: tests/test_send.py builds it with g++ under AddressSanitizer + UBSan and runs it.
// The range checks at their edges, the byte conversions both ways, the SHA padding into heap blocks of
// exactly the size msg_blocks gives (one byte too many is an ASan error), the DER encoder against libcrypto's
// i2d_ECDSA_SIG and against the strict parser, the parser on the encoder's outputs bent four ways, and the
// random draws.  Loads neither HIP nor the library.
#include <openssl/bn.h>
#include <openssl/ecdsa.h>

#include <array>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>

#include "bmpow_host_scalar.h"

using namespace bmhost;

static int g_fail = 0;
#define CHECK(cond, ...)                                        \
  do {                                                          \
    if (!(cond)) {                                              \
      std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
      std::fprintf(stderr, __VA_ARGS__);                        \
      std::fputc('\n', stderr);                                 \
      if (++g_fail > 20) std::exit(1);                          \
    }                                                           \
  } while (0)

using B32 = std::array<uint8_t, 32>;

static B32 unhex32(const char* h) {
  B32 v{};
  for (int i = 0; i < 32; ++i) {
    unsigned b = 0;
    std::sscanf(h + 2 * i, "%2x", &b);
    v[i] = (uint8_t)b;
  }
  return v;
}

static B32 plus(B32 v, int delta) {  // v + delta as a 256-bit big-endian integer (no wrap in the cases used)
  int carry = delta;
  for (int i = 31; i >= 0 && carry; --i) {
    const int t = v[i] + carry;
    v[i] = (uint8_t)(t & 0xff);
    carry = t >> 8;  // arithmetic: -1 borrows on
  }
  return v;
}

static const B32 kN = unhex32("FFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141");
static const B32 kP = unhex32("FFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEFFFFFC2F");
static const B32 kOnes = unhex32("FFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFF");

static void test_ranges() {
  const B32 zero{}, one = plus(zero, 1);
  const struct {
    B32 v;
    bool in;
    const char* name;
  } scalars[] = {{zero, false, "0"},          {one, true, "1"},           {plus(kN, -1), true, "n - 1"},
                 {kN, false, "n"},            {plus(kN, 1), false, "n + 1"}, {kOnes, false, "2^256 - 1"}};
  for (const auto& c : scalars) {
    CHECK(scalar_in_range(c.v.data()) == c.in, "scalar_in_range(bytes %s)", c.name);
    CHECK(scalar_in_range(sc_from_be(c.v.data())) == c.in, "scalar_in_range(sc %s)", c.name);
  }
  B32 limb0 = kP, limb1 = kP, limb7 = kP;  // p with one limb lowered: below p whichever limb it is
  limb0[31] -= 1;   // limb 0 is bytes 28..31
  limb1[27] -= 1;   // limb 1 is bytes 24..27: 0xFFFFFFFE -> 0xFFFFFFFD
  limb7[0] -= 0x80;  // limb 7 is bytes 0..3
  B32 limb0_up = kP, limb1_up = kP;  // and raised: above p
  limb0_up[31] += 1;
  limb1_up[27] += 1;  // limb 1 all ones
  const struct {
    B32 v;
    bool in;
    const char* name;
  } coords[] = {{plus(kP, -1), true, "p - 1"},   {kP, false, "p"},         {plus(kP, 1), false, "p + 1"},
                {kOnes, false, "2^256 - 1"},     {limb0, true, "limb 0 lower"}, {limb1, true, "limb 1 lower"},
                {limb7, true, "limb 7 lower"},   {limb0_up, false, "limb 0 higher"}, {limb1_up, false, "limb 1 higher"},
                {B32{}, true, "0"}};
  for (const auto& c : coords) CHECK(coord_in_range(sc_from_be(c.v.data())) == c.in, "coord_in_range(%s)", c.name);
  // limbs are little-endian words of the big-endian bytes, and the way back is the inverse
  const sc n = sc_from_be(kN.data());
  CHECK(n.d[0] == 0xD0364141u && n.d[4] == 0xFFFFFFFEu && n.d[7] == 0xFFFFFFFFu, "limb order");
  for (const B32& v : {zero, one, kN, kP, kOnes, limb1, unhex32("000102030405060708090a0b0c0d0e0f101112131415161718191a1b1c1d1e1f")}) {
    B32 back;
    sc_to_be(sc_from_be(v.data()).d, back.data());
    CHECK(back == v, "sc_to_be(sc_from_be(x)) == x");
  }
}

static void test_padding() {
  for (size_t len : {0, 1, 55, 56, 63, 64, 119, 120}) {
    const uint32_t nblk = msg_blocks(len);
    CHECK(nblk == (len + 9 + 63) / 64, "msg_blocks(%zu) = %u", len, nblk);
    std::vector<uint8_t> msg(len);
    for (size_t i = 0; i < len; ++i) msg[i] = (uint8_t)(i * 7 + 1);
    const size_t total = (size_t)nblk * 64;
    uint8_t* block = (uint8_t*)std::malloc(total);  // exactly the blocks: ASan sees a byte beyond
    std::memset(block, 0xA5, total);
    pad_blocks(len ? msg.data() : nullptr, len, block, nblk);
    std::vector<uint8_t> want(msg);  // the naive restatement
    want.push_back(0x80);
    while (want.size() % 64 != 56) want.push_back(0);
    for (int j = 7; j >= 0; --j) want.push_back((uint8_t)(((uint64_t)len * 8) >> (8 * j)));
    CHECK(want.size() == total && std::memcmp(block, want.data(), total) == 0, "pad_blocks at %zu", len);
    std::free(block);
  }
}

static std::vector<uint8_t> i2d(const uint8_t* rs) {
  ECDSA_SIG* sig = ECDSA_SIG_new();
  ECDSA_SIG_set0(sig, BN_bin2bn(rs, 32, nullptr), BN_bin2bn(rs + 32, 32, nullptr));
  uint8_t buf[80], *p = buf;
  const int l = i2d_ECDSA_SIG(sig, &p);
  ECDSA_SIG_free(sig);
  return std::vector<uint8_t>(buf, buf + (l > 0 ? l : 0));
}

static bool parses(const std::vector<uint8_t>& der) {
  std::vector<uint8_t> exact(der);  // a heap copy of exactly the length: a read past it is an ASan error
  uint8_t rs[64];
  return sig_parse(exact.data(), exact.size(), rs);
}

static void test_der() {
  std::vector<B32> vals = {plus(B32{}, 1), unhex32("7FFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFF"),
                           unhex32("8000000000000000000000000000000000000000000000000000000000000000"), plus(kN, -1)};
  for (int zeros : {1, 15, 31})  // leading zero bytes, then a byte with the top bit set and one without
    for (uint8_t first : {0x80, 0x7f}) {
      B32 v{};
      v[zeros] = first;
      for (int i = zeros + 1; i < 32; ++i) v[i] = (uint8_t)(0x11 * (i % 15 + 1));
      vals.push_back(v);
    }
  CHECK(all_zero(B32{}.data(), 32) && !all_zero(vals[0].data(), 32) && all_zero(vals[0].data(), 31), "all_zero");
  for (const B32& r : vals)
    for (const B32& s : vals) {
      uint8_t rs[64], der[72], back[64];
      std::memcpy(rs, r.data(), 32);
      std::memcpy(rs + 32, s.data(), 32);
      const size_t l = sig_der(rs, der);
      const std::vector<uint8_t> mine(der, der + l), theirs = i2d(rs);
      CHECK(mine == theirs, "sig_der against i2d_ECDSA_SIG (%zu / %zu bytes)", mine.size(), theirs.size());
      CHECK(sig_parse(mine.data(), mine.size(), back) && std::memcmp(back, rs, 64) == 0, "sig_parse(sig_der(rs)) == rs");
      // the encoder's output bent: each is refused
      std::vector<uint8_t> bent(mine);
      bent.push_back(0);
      CHECK(!parses(bent), "one byte appended");
      for (int d : {-1, 1}) {
        bent = mine;
        bent[1] = (uint8_t)(bent[1] + d);
        CHECK(!parses(bent), "outer length off by %d", d);
      }
      for (int which = 0; which < 2; ++which) {  // r's INTEGER, then s's
        const size_t at = which == 0 ? 2 : 4 + mine[3];  // the INTEGER's tag
        bent = mine;  // a padding zero inserted in front of the value, the lengths following
        bent.insert(bent.begin() + at + 2, 0);
        bent[at + 1] += 1, bent[1] += 1;
        if (!(mine[at + 2] & 0x80)) CHECK(!parses(bent), "a padding zero inserted (integer %d)", which);
        else CHECK(!parses(bent), "a second padding zero inserted (integer %d)", which);
        if (mine[at + 2] == 0 && mine[at + 1] > 1) {  // its padding zero removed: the value reads as negative
          bent = mine;
          bent.erase(bent.begin() + at + 2);
          bent[at + 1] -= 1, bent[1] -= 1;
          CHECK(!parses(bent), "the padding zero removed (integer %d)", which);
        }
      }
    }
  // what the range check behind the parser refuses: r or s of 0 and of n
  for (const B32& bad : {B32{}, kN}) {
    uint8_t rs[64];
    std::memcpy(rs, vals[0].data(), 32);
    std::memcpy(rs + 32, bad.data(), 32);
    CHECK(!parses(i2d(rs)), "s out of range");
  }
}

static void test_draws() {
  std::vector<uint8_t> rows(32 * 64);
  CHECK(draw_scalars(rows.data(), 64), "draw_scalars");
  std::set<B32> seen;
  for (int i = 0; i < 64; ++i) {
    B32 v;
    std::memcpy(v.data(), rows.data() + 32 * i, 32);
    CHECK(scalar_in_range(v.data()), "drawn row %d in range", i);
    seen.insert(v);
  }
  CHECK(seen.size() == 64, "drawn rows differ");
  uint8_t one[32] = {};
  CHECK(draw_scalar(one) && scalar_in_range(one), "draw_scalar");
  std::vector<uint8_t> big((1u << 20) + 5, 0);  // more than one RAND_bytes call
  CHECK(draw_bytes(big.data(), big.size()) && !all_zero(big.data() + (1u << 20), 5), "draw_bytes across its chunk");
  {
    Wiped<uint8_t> w;  // the cleansing owners release what they hold (LeakSanitizer) and touch nothing beyond
    w.v.assign(33, 0xEE);
    WipedBytes p;
    p.alloc(17);
    std::memset(p.get(), 0xEE, 17);
    p.alloc(5);  // over a live one
    CHECK(p.bytes == 5, "WipedBytes");
    Wiped<uint8_t> empty;
    WipedBytes none;
  }
}

int main() {
  test_ranges();
  test_padding();
  test_der();
  test_draws();
  if (g_fail) return 1;
  std::fprintf(stderr, "all host scalar checks passed\n");
  return 0;
}
