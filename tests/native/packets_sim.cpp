// packets_sim.cpp -- the byte-oriented code of the packet kernels and of the frame walk
// (pybitmessage_amd/csrc/bmpow_packets_fmt.h) on the host, as a stand-alone program: tests/test_packets_native.py
// builds it with g++ under AddressSanitizer + UBSan and runs it.  The pack works from a heap block of exactly the
// arena's size (whole 16-byte chunks, as the device's allocation) into one of exactly the pool's, and the walk
// over heap blocks of exactly the buffer's length, so a byte read or written past one is an error.  Loads
// neither HIP nor the library.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bmpow_packets_fmt.h"

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

struct Exact {  // exactly n bytes from malloc (16-byte aligned): ASan's redzone starts at byte n
  uint8_t* p;
  explicit Exact(size_t n, int fill = 0xA5) : p((uint8_t*)std::malloc(n ? n : 1)) { std::memset(p, fill, n ? n : 1); }
  ~Exact() { std::free(p); }
};

typedef std::vector<uint8_t> bytes;

static uint8_t byte_of(size_t i, unsigned seed) { return (uint8_t)(i * 131 + seed * 29 + (i >> 8) + 7); }

// data || 0x80 || zeros || 128-bit big-endian bit length
static bytes padded(const uint8_t* data, size_t m) {
  const size_t total = (m + 17 + 127) / 128 * 128;
  bytes out(total, 0);
  if (m) std::memcpy(out.data(), data, m);
  out[m] = 0x80;
  const uint64_t bits = (uint64_t)m * 8;
  for (int j = 0; j < 8; ++j) out[total - 1 - j] = (uint8_t)(bits >> (8 * j));
  return out;
}

// One row the way pk_pack_kernel packs it: `front` bytes in front of the payload, which then ends `back` bytes
// before the arena's end.
static void pack_case(uint32_t kind, size_t front, size_t len, size_t back) {
  const size_t arena_bytes = front + len + back;
  const uint64_t arena_chunks = (arena_bytes + 15) / 16;
  Exact arena(arena_chunks * 16, 0xEE);
  for (size_t i = 0; i < arena_bytes; ++i) arena.p[i] = byte_of(i, (unsigned)(front + 3 * len));
  const uint32_t m = pkf::row_data_len(kind, (uint32_t)len), nblk = pkf::row_blocks(kind, (uint32_t)len);
  const uint64_t s = front + (kind == PK_OBJECT ? 8 : 0);
  const bytes want = padded(arena.p + s, m);
  CHECK(want.size() == 128u * nblk, "kind %u len %zu: %u blocks planned, %zu padded", kind, len, nblk, want.size() / 128);
  Exact pool(128u * nblk, 0x5A);
  for (uint32_t c = 0; c < 8 * nblk; ++c) {
    uint32_t w[4];
    pkf::pack_chunk(c, nblk, reinterpret_cast<const uint32_t*>(arena.p), arena_chunks, s, m, w);
    std::memcpy(pool.p + 16 * c, w, 16);
  }
  CHECK(std::memcmp(pool.p, want.data(), want.size()) == 0, "kind %u front %zu len %zu back %zu: packed bytes differ", kind,
        front, len, back);
}

static void put_be32(uint8_t* p, uint32_t v) {
  p[0] = (uint8_t)(v >> 24), p[1] = (uint8_t)(v >> 16), p[2] = (uint8_t)(v >> 8), p[3] = (uint8_t)v;
}

static void add_packet(bytes& buf, const char* cmd, size_t cmd_len, uint32_t claim, size_t have) {
  uint8_t h[24] = {0};
  put_be32(h, BMPOW_PKT_MAGIC);
  std::memcpy(h + 4, cmd, cmd_len);
  put_be32(h + 16, claim);
  put_be32(h + 20, 0x01020304u);
  buf.insert(buf.end(), h, h + 24);
  for (size_t i = 0; i < have; ++i) buf.push_back(byte_of(i, (unsigned)claim));
}

struct Walked {
  std::vector<bmpow_packet_rec> recs;
  uint64_t consumed;
  uint32_t close;
};

static Walked walk_exact(const bytes& buf, size_t cut, uint32_t flags, bool all) {
  Exact e(cut);
  if (cut) std::memcpy(e.p, buf.data(), cut);
  Walked w;
  const uint64_t n = pkf::walk(e.p, cut, flags, all, &w.consumed, &w.close,
                               [&](const bmpow_packet_rec& r) { w.recs.push_back(r); });
  CHECK(n == w.recs.size(), "count");
  CHECK(w.consumed <= cut, "consumed %llu past the %zu bytes", (unsigned long long)w.consumed, cut);
  for (const bmpow_packet_rec& r : w.recs)
    CHECK((uint64_t)r.offset + BMPOW_PKT_HEADER + r.length <= cut, "a packet framed past the buffer's end");
  return w;
}

static void walk_cases() {
  bytes buf;
  add_packet(buf, "ping", 4, 0, 0);
  add_packet(buf, "OBJECT", 6, 40, 40);
  add_packet(buf, "object\0x", 8, 3, 3);
  add_packet(buf, "abcdefghijkl", 12, 17, 17);
  buf.push_back(0x11);  // a byte that is no magic
  add_packet(buf, "inv", 3, 33, 33);
  add_packet(buf, "verack", 6, 0, 0);
  add_packet(buf, "addr", 4, 1, 1);
  add_packet(buf, "getdata", 7, BMPOW_PKT_MAX_MESSAGE + 1, 5);  // claims more than any buffer here holds
  for (uint32_t flags = 0; flags < 4; ++flags)
    for (int all = 0; all < 2; ++all) {
      const Walked full = walk_exact(buf, buf.size(), flags, all != 0);
      for (size_t cut = 0; cut <= buf.size(); ++cut) {
        const Walked w = walk_exact(buf, cut, flags, all != 0);
        CHECK(w.recs.size() <= full.recs.size(), "flags %u all %d cut %zu: more packets than the whole buffer", flags, all, cut);
        for (size_t i = 0; i < w.recs.size() && i < full.recs.size(); ++i)
          CHECK(std::memcmp(&w.recs[i], &full.recs[i], sizeof(bmpow_packet_rec)) == 0, "flags %u all %d cut %zu: record %zu", flags,
                all, cut, i);
      }
    }
  // the commands: matched without regard to case, exact only in the handler's spelling
  const Walked w = walk_exact(buf, buf.size(), BMPOW_PKT_CONN_ESTABLISHED | BMPOW_PKT_CONN_DATAGRAM, true);
  CHECK(w.recs.size() == 7, "%zu packets", w.recs.size());
  if (w.recs.size() == 7) {
    CHECK(w.recs[0].command == BMPOW_PKT_PING && w.recs[0].exact == 1, "ping");
    CHECK(w.recs[1].command == BMPOW_PKT_OBJECT && w.recs[1].exact == 0, "OBJECT");
    CHECK(w.recs[2].command == BMPOW_PKT_UNIMPLEMENTED, "object\\0x");
    CHECK(w.recs[3].command == BMPOW_PKT_UNIMPLEMENTED, "twelve bytes without a NUL");
    CHECK(w.recs[4].command == BMPOW_PKT_INV && w.recs[5].command == BMPOW_PKT_VERACK, "inv, verack");
  }
}

int main() {
  // every source residue, every length across the 111/112 and 239/240 padding edges, both kinds; the payload
  // ends on the arena's last byte (back 0: rows whose last chunk is the arena's last, whole or not) or before it
  for (size_t front = 0; front < 16; ++front)
    for (size_t len = 0; len <= 300; ++len)
      for (size_t back = 0; back < 2; ++back) {
        pack_case(PK_SUM, front, len, 17 * back);
        if (len >= 8) pack_case(PK_OBJECT, front, len, 17 * back);
      }
  pack_case(PK_SUM, 16 * 5, 16 * 9, 0);  // a row of whole chunks that ends on the arena's last byte
  pack_case(PK_OBJECT, 16 * 5 + 8, 16 * 9, 0);
  walk_cases();
  if (g_fail) {
    std::fprintf(stderr, "%d of %ld packets checks FAILED\n", g_fail, g_checks);
    return 1;
  }
  std::fprintf(stderr, "all packets checks passed (%ld)\n", g_checks);
  return 0;
}
