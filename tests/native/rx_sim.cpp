// rx_sim.cpp -- the byte-oriented half of the msg processing (pybitmessage_amd/csrc/bmpow_rx_fmt.h: varints,
// the field walk, the DER parse, the prefix and the packing of signedData) on the CPU, called as the kernels
// of bmpow_rx.hip call it.
//
// A stand-alone program: g++ -fsanitize=address,undefined, its own main, loaded into nothing.  Every buffer
// the header reads is a heap block of exactly the size the device's is, so a read past a plaintext or past a
// pool slot is an error here.
//   rx_sim ROWS.txt      one row per line:
//       M <status the walk must leave> <object head hex | -> <plaintext hex | -> <toRipe hex, 40 digits>
// On top of the rows: the first row whose walk gets through is cut at every length 0 .. its own and walked,
// parsed and key-loaded again; and the pack routine's output is compared with data || 0x80 || zeros || the bit
// length for every signed length 170 .. 400 under the four prefix widths (14, 16, 18, 22), with and without
// plaintext behind the signed part.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "bmpow_rx_fmt.h"

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

std::vector<uint8_t> unhex(const std::string& s) {
  if (s == "-") return {};
  std::vector<uint8_t> out(s.size() / 2);
  for (size_t i = 0; i < out.size(); ++i) out[i] = (uint8_t)std::strtoul(s.substr(2 * i, 2).c_str(), nullptr, 16);
  return out;
}

// a heap block of exactly n bytes (null for n == 0: nothing may be read)
struct Exact {
  std::unique_ptr<uint8_t[]> p;
  size_t n;
  explicit Exact(const uint8_t* src, size_t len) : p(len ? new uint8_t[len] : nullptr), n(len) {
    if (len) std::memcpy(p.get(), src, len);
  }
};

// the whole of what rx_walk_kernel does with one row; returns the walk's status
int walk_row(const std::vector<uint8_t>& head_in, const std::vector<uint8_t>& plain_in, const uint8_t* to_ripe,
             bmpow_rx_msg_rec& rec, bool& der, bool& real) {
  const Exact head(head_in.data(), head_in.size() < rxf::kHeadBytes ? head_in.size() : rxf::kHeadBytes);
  const Exact plain(plain_in.data(), plain_in.size());
  std::memset(&rec, 0, sizeof rec);
  uint32_t key_off = 0;
  rxf::walk(head.p.get(), (uint32_t)head.n, plain.p.get(), plain.n, to_ripe, rec, key_off);
  der = real = false;
  if (rec.status == BMPOW_RX_OK) {
    uint32_t r[8], s[8], x[8], y[8];
    CHECK((uint64_t)rec.sig_off + rec.sig_len <= plain.n, "signature slice past the plaintext");
    CHECK((uint64_t)rec.msg_off + rec.msg_len <= plain.n && (uint64_t)rec.ack_off + rec.ack_len <= plain.n, "slice past the plaintext");
    CHECK(rec.bottom <= plain.n && key_off + 128 <= plain.n, "bottom or keys past the plaintext");
    der = rxf::der_parse(plain.p.get() + rec.sig_off, rec.sig_len, r, s);
    real = rxf::load_key(plain.p.get() + key_off, x, y) && der;
    uint32_t pre[6];
    uint8_t head38[rxf::kHeadBytes] = {0};
    if (head.n) std::memcpy(head38, head.p.get(), head.n);
    const uint32_t plen = rxf::put_prefix(head38, rec.claimed_stream, pre);
    CHECK(plen == rec.prefix_len, "prefix length %u against the record's %u", plen, rec.prefix_len);
    CHECK(rxf::signed_blocks(plen, rec.bottom) <= rxf::signed_blocks_bound(plain.n), "more blocks than the host reserved");
  }
  return rec.status;
}

struct HostSrc {  // a pool slot: the plaintext in a block of its length rounded up to 16 bytes
  const uint8_t* slot;
  uint32_t nchunks, len;
  void load16(uint32_t k, uint32_t (&w)[4]) const {
    for (int i = 0; i < 4; ++i) w[i] = 0;
    if (k < nchunks) std::memcpy(w, slot + 16 * (size_t)k, 16);
  }
  uint32_t byte(uint32_t i) const { return i < len ? slot[i] : 0u; }
};

void pack_checks() {
  uint64_t x = 0x9e3779b97f4a7c15ull;
  const uint64_t streams[4] = {7, 300, 70000, 1ull << 32};
  const uint32_t widths[4] = {14, 16, 18, 22};
  int compared = 0;
  for (int width = 0; width < 4; ++width) {
    uint8_t head[rxf::kHeadBytes];
    for (uint32_t i = 0; i < rxf::kHeadBytes; ++i) head[i] = (uint8_t)(0xa0 + i);
    uint32_t pre[6];
    const uint32_t plen = rxf::put_prefix(head, streams[width], pre);
    CHECK(plen == widths[width], "prefix width %u", plen);
    uint8_t prefix[24];
    std::memcpy(prefix, pre, 24);
    for (uint32_t i = 0; i < 12; ++i) CHECK(prefix[i] == head[8 + i], "prefix byte %u", i);
    CHECK(prefix[12] == 1, "varint(1)");
    for (uint32_t i = plen; i < 24; ++i) CHECK(prefix[i] == 0, "byte %u behind the prefix", i);
    for (uint32_t total = 170; total <= 400; ++total)
      for (uint32_t behind = 0; behind <= 75; behind += 75) {  // plaintext behind the signed part, or none
        const uint32_t bottom = total - plen, len = bottom + behind, slot_bytes = (len + 15) & ~15u;
        std::unique_ptr<uint8_t[]> slot(new uint8_t[slot_bytes]);
        std::memset(slot.get(), 0, slot_bytes);
        for (uint32_t i = 0; i < len; ++i) {
          x = x * 6364136223846793005ull + 1442695040888963407ull;
          slot[i] = (uint8_t)(x >> 56);
        }
        const HostSrc src = {slot.get(), slot_bytes / 16, len};
        const uint32_t nblk = rxf::signed_blocks(plen, bottom);
        CHECK(nblk == (total + 9 + 63) / 64, "block count of %u bytes", total);
        std::vector<uint8_t> want((size_t)nblk * 64, 0), got((size_t)nblk * 64, 0xcc);
        std::memcpy(want.data(), prefix, plen);
        std::memcpy(want.data() + plen, slot.get(), bottom);
        want[total] = 0x80;
        const uint64_t bits = 8ull * total;
        for (int j = 0; j < 8; ++j) want[want.size() - 8 + j] = (uint8_t)(bits >> (56 - 8 * j));
        for (uint32_t c = 0; c < 4 * nblk; ++c) {
          uint32_t w[4];
          rxf::pack_chunk(c, nblk, pre, plen, bottom, src, w);
          std::memcpy(got.data() + 16 * (size_t)c, w, 16);
        }
        CHECK(got == want, "packed blocks of %u signed bytes, prefix %u, %u behind", total, plen, behind);
        ++compared;
      }
  }
  CHECK(compared == 4 * 231 * 2, "pack cases");
}

void varint_checks() {
  struct { const char* hex; bool ok; uint64_t v; uint32_t n; } rows[] = {
      {"-", true, 0, 0}, {"00", true, 0, 1}, {"fc", true, 252, 1}, {"fd00fd", true, 253, 3}, {"fd00fc", false, 0, 0},
      {"fdffff", true, 65535, 3}, {"fd01", false, 0, 0}, {"fe00010000", true, 65536, 5}, {"fe0000ffff", false, 0, 0},
      {"fe000100", false, 0, 0}, {"ff0000000100000000", true, 1ull << 32, 9}, {"ff00000000ffffffff", false, 0, 0},
      {"ffffffffffffffffff", true, ~0ull, 9}, {"ff00000000000000", false, 0, 0}, {"fc77", true, 252, 1}};
  for (const auto& r : rows) {
    const std::vector<uint8_t> v = unhex(r.hex);
    const Exact e(v.data(), v.size());
    const rxf::varint got = rxf::get_varint(e.p.get(), e.n, 0);
    CHECK(got.ok == r.ok && (!r.ok || (got.v == r.v && got.n == r.n)), "varint %s", r.hex);
    CHECK(rxf::get_varint(e.p.get(), e.n, e.n).n == 0 && rxf::get_varint(e.p.get(), e.n, ~0ull).ok, "varint past the end");
  }
  CHECK(rxf::sat_add(~0ull, 1) == ~0ull && rxf::sat_add(~0ull - 1, 1) == ~0ull && rxf::sat_add(5, 6) == 11, "sat_add");
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: rx_sim ROWS.txt\n");
    return 2;
  }
  varint_checks();
  pack_checks();
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) {
    std::fprintf(stderr, "cannot open %s\n", argv[1]);
    return 2;
  }
  static char kind[4], want[16], head[256], plain[1 << 20], ripe[64];
  int rows = 0;
  bool swept = false;
  while (std::fscanf(f, "%3s %15s %255s %1048575s %63s", kind, want, head, plain, ripe) == 5) {
    const std::vector<uint8_t> h = unhex(head), p = unhex(plain), r = unhex(ripe);
    CHECK(kind[0] == 'M' && r.size() == 20, "malformed row %d", rows);
    if (r.size() != 20) break;
    bmpow_rx_msg_rec rec;
    bool der, real;
    const int status = walk_row(h, p, r.data(), rec, der, real);
    CHECK(status == std::atoi(want), "row %d: status %d, wanted %s", rows, status, want);
    if (status == BMPOW_RX_OK && real && !swept) {
      swept = true;
      int seen[10] = {0};
      for (size_t cut = 0; cut <= p.size(); ++cut) {
        const std::vector<uint8_t> q(p.begin(), p.begin() + cut);
        const int st = walk_row(h, q, r.data(), rec, der, real);
        CHECK(st >= 0 && st < 10, "status %d", st);
        if (st >= 0 && st < 10) seen[st]++;
        CHECK(cut == p.size() ? real : !real, "cut at %zu of %zu: real = %d", cut, p.size(), (int)real);
      }
      // nothing reads as sender version 0, then the floor of :500; from there on every status is one the walk
      // can leave, and the whole plaintext is the only cut that goes to the curve kernels as it stands
      int total = 0;
      for (int st = 0; st < 10; ++st) total += seen[st];
      CHECK(seen[BMPOW_RX_SENDER_VERSION_0] == 1 && seen[BMPOW_RX_TOO_SHORT] == 169 && seen[BMPOW_RX_OK] > 0 &&
                seen[BMPOW_RX_NOT_MINE] == 0 && seen[BMPOW_RX_BAD_SIGNATURE] == 0 && total == (int)p.size() + 1,
            "the sweep's statuses: %d %d %d of %d", seen[3], seen[5], seen[0], total);
    }
    ++rows;
  }
  std::fclose(f);
  CHECK(swept, "no row to sweep");
  if (g_fail) {
    std::fprintf(stderr, "%d checks failed\n", g_fail);
    return 1;
  }
  std::fprintf(stderr, "all rx checks passed (%d rows)\n", rows);
  return 0;
}
