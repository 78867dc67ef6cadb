// proc_sim.cpp -- the watch index's probe, the byte compare and the mix, and the walks of a getpubkey and of an
// onionpeer (pybitmessage_amd/csrc/bmpow_proc_fmt.h) on the host, as a stand-alone program:
// tests/test_proc_native.py builds it with g++ under AddressSanitizer + UBSan and runs it.  Every buffer is a heap
// block of exactly the bytes the functions may read, so a load past a pool's end is ASan's to report.  One thread:
// what it cannot show is the order in which lanes meet at first[], which is an atomic minimum on the device.
// Loads neither HIP nor the library.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "bmpow_proc_fmt.h"

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
  size_t n;
  explicit Exact(size_t n_, int fill = 0xA5) : p((uint8_t*)std::malloc(n_ ? n_ : 1)), n(n_) { std::memset(p, fill, n_ ? n_ : 1); }
  ~Exact() { std::free(p); }
  const uint64_t* words() const { return reinterpret_cast<const uint64_t*>(p); }
};

static uint64_t g_rng = 0x2545F4914F6CDD1DULL;
static uint64_t rnd() {
  g_rng ^= g_rng << 13, g_rng ^= g_rng >> 7, g_rng ^= g_rng << 17;
  return g_rng;
}
static std::string rnd_key(size_t len, uint32_t family) {
  // keys of one family share their first 16 bytes: equal tags and start slots wherever their lengths are equal
  std::string k(len, '\0');
  for (size_t i = 0; i < len; ++i) k[i] = (char)(i < 16 ? (family * 37u + i * 11u) : rnd());
  return k;
}

// ---- 1. random watch sets against std::unordered_map ----
static void watch_sets() {
  for (int round = 0; round < 300; ++round) {
    const uint64_t seed = rnd() | 1;
    const size_t n = rnd() % 41;
    std::unordered_map<std::string, uint32_t> model;
    while (model.size() < n) {
      const size_t len = rnd() % 8 == 0 ? rnd() % 16 : 16 + rnd() % 33;
      model[rnd_key(len, (uint32_t)(rnd() % 5))] = (uint32_t)rnd();
    }
    // flattened as the host unit does it
    std::vector<std::string> flat;
    size_t bytes = 0;
    for (const auto& kv : model) flat.push_back(kv.first), bytes += kv.first.size();
    const uint32_t log2 = pcf::watch_log2_for(n), slots = 1u << log2;
    CHECK(slots >= 8 && slots >= 2 * n, "%u slots for %zu keys", slots, n);
    Exact pool(bytes);
    std::vector<uint64_t> tags(slots, 0);
    std::vector<uint32_t> slot_entry(slots, PC_NONE);
    std::vector<pcf::pc_entry> entries(n);
    uint32_t at = 0;
    for (size_t e = 0; e < n; ++e) {
      const std::string& k = flat[e];
      if (!k.empty()) std::memcpy(pool.p + at, k.data(), k.size());
      entries[e] = pcf::pc_entry{at, (uint32_t)k.size(), model[k]};
      at += (uint32_t)k.size();
      const uint64_t mix = pcf::watch_mix_of(seed, (const uint8_t*)k.data(), (uint32_t)k.size());
      CHECK(pcf::watch_tag(mix) != 0, "a zero tag");
      pcf::watch_place(tags.data(), slot_entry.data(), log2, mix, (uint32_t)e);
    }
    const pcf::WatchTable t{tags.data(), slot_entry.data(), entries.data(), pool.words(), bytes, seed, (uint32_t)n, log2};
    // probes: every resident key of 16 bytes or more, the same with one byte changed, and strangers of the families
    std::vector<std::string> probes;
    for (const std::string& k : flat) {
      if (k.size() < 16) continue;
      probes.push_back(k);
      std::string other = k;
      other[rnd() % other.size()] ^= (char)(1 << (rnd() % 8));
      probes.push_back(other);
      probes.push_back(k + "x");
      if (k.size() > 16) probes.push_back(k.substr(0, k.size() - 1));
    }
    for (int i = 0; i < 20; ++i) probes.push_back(rnd_key(16 + rnd() % 33, (uint32_t)(rnd() % 6)));
    // the tails back to back at whatever offsets that gives, the last one ending on the block's last byte
    size_t total = 0;
    for (const std::string& p : probes) total += p.size();
    Exact in(total);
    size_t off = 0;
    for (const std::string& p : probes) {
      std::memcpy(in.p + off, p.data(), p.size());
      const uint32_t e = pcf::watch_find(t, in.words(), total, off, (uint32_t)p.size());
      const auto it = model.find(p);
      if (it == model.end()) {
        CHECK(e == PC_NONE, "round %d: a stranger of %zu bytes found as entry %u", round, p.size(), e);
      } else {
        CHECK(e < n && flat[e] == p && entries[e].aux == it->second, "round %d: a resident key of %zu bytes not found", round, p.size());
      }
      off += p.size();
    }
  }
}

// ---- 2. compare and mix at every residue and tail length ----
static void compare_and_mix() {
  for (uint32_t len = 16; len <= 48; ++len)
    for (uint32_t ra = 0; ra < 8; ++ra)
      for (uint32_t rb = 0; rb < 8; ++rb) {
        Exact a(ra + len, 0x11), b(rb + len, 0x22);  // each run ends on its block's last byte
        for (uint32_t i = 0; i < len; ++i) a.p[ra + i] = b.p[rb + i] = (uint8_t)rnd();
        CHECK(pcf::bytes_eq(a.words(), a.n, ra, b.words(), b.n, rb, len), "equal runs differ: len %u at %u / %u", len, ra, rb);
        const uint64_t ma = pcf::watch_mix(7, len, pcf::load_u64_at(a.words(), a.n, ra), pcf::load_u64_at(a.words(), a.n, ra + 8));
        CHECK(ma == pcf::watch_mix_of(7, b.p + rb, len), "the mix depends on the offset: len %u at %u", len, ra);
        for (uint32_t at : {0u, len / 2, len - 1}) {
          b.p[rb + at] ^= 0x40;
          CHECK(!pcf::bytes_eq(a.words(), a.n, ra, b.words(), b.n, rb, len), "byte %u of %u not compared (%u / %u)", at, len, ra, rb);
          b.p[rb + at] ^= 0x40;
        }
        CHECK(!pcf::bytes_eq(a.words(), a.n, ra, b.words(), b.n, rb + 1, len), "a run past its block's end compared equal");
        // the bytes before a run are not part of it
        if (ra) a.p[ra - 1] ^= 0xff;
        CHECK(pcf::bytes_eq(a.words(), a.n, ra, b.words(), b.n, rb, len), "a byte before the run was compared");
      }
}

// ---- 3. the walks over every cut length ----
static void put_varint(std::vector<uint8_t>& v, uint64_t x) {
  if (x < 253) v.push_back((uint8_t)x);
  else {
    const int n = x < 65536 ? 2 : x < 4294967296ull ? 4 : 8;
    v.push_back(n == 2 ? 253 : n == 4 ? 254 : 255);
    for (int i = n - 1; i >= 0; --i) v.push_back((uint8_t)(x >> (8 * i)));
  }
}

static pcf::Bytes at_offset(const Exact& block, uint32_t lead, uint32_t avail, uint32_t len) {
  return pcf::Bytes{block.words(), block.n, lead, avail, len};
}

static void walks() {
  // my addresses
  std::vector<pc_addr> rows(5);
  std::memset(rows.data(), 0, rows.size() * sizeof(pc_addr));
  for (size_t r = 0; r < rows.size(); ++r) {
    for (int i = 0; i < 20; ++i) rows[r].ripe[i] = (uint8_t)rnd();
    for (int i = 0; i < 32; ++i) rows[r].tag[i] = (uint8_t)rnd();
    rows[r].version = r < 2 ? 3 : 4, rows[r].stream = 1;
  }
  const uint32_t log2 = pcf::addr_log2_for((uint32_t)rows.size());
  std::vector<uint32_t> by_ripe(1u << log2), by_tag(1u << log2);
  CHECK(pcf::fill_index(rows.data(), (uint32_t)rows.size(), log2, by_ripe.data(), by_tag.data()), "distinct rows refused");
  const pcf::AddrTable t{rows.data(), by_ripe.data(), by_tag.data(), (uint32_t)rows.size(), log2};
  std::vector<pc_addr> twice = rows;
  std::memcpy(twice[4].tag, twice[1].tag, 32);
  CHECK(!pcf::fill_index(twice.data(), 5, log2, by_ripe.data(), by_tag.data()), "two rows with one tag accepted");
  CHECK(pcf::fill_index(rows.data(), (uint32_t)rows.size(), log2, by_ripe.data(), by_tag.data()), "distinct rows refused");

  for (uint64_t version : {3ull, 4ull})
    for (uint64_t stream : {1ull, 300ull, 70000ull, 1ull << 40})
      for (uint32_t lead = 0; lead < 8; ++lead) {
        std::vector<uint8_t> obj(20, 0x33);
        put_varint(obj, version), put_varint(obj, stream);
        const size_t key_at = obj.size();
        const pc_addr& mine = rows[version == 3 ? 1 : 3];
        obj.insert(obj.end(), version == 3 ? mine.ripe : mine.tag, (version == 3 ? mine.ripe + 20 : mine.tag + 32));
        for (size_t cut = 0; cut <= obj.size(); ++cut) {
          Exact block(lead + cut);  // the object's bytes end on the block's last byte
          std::memcpy(block.p + lead, obj.data(), cut);
          pc_rec r{};
          pcf::walk_getpubkey(at_offset(block, lead, (uint32_t)cut, (uint32_t)cut), t, 5000000, &r);
          uint32_t want;
          if (cut <= 20) want = PC_VERSION_ZERO;                         // decodeVarint(b'') is (0, 0)
          else if (cut > 21 && cut < key_at) want = PC_MALFORMED;        // inside the stream's varint
          else if (cut < obj.size()) want = version == 3 ? PC_SHORT_HASH : PC_SHORT_TAG;  // cut 21: an empty stream slice
          else want = stream == 1 ? (version == 3 ? PC_SEND_V3 : PC_SEND_V4) : PC_STREAM_MISMATCH;
          CHECK(r.status == want, "getpubkey v%llu stream %llu cut %zu: status %u, want %u", (unsigned long long)version,
                (unsigned long long)stream, cut, r.status, want);
          if (want == PC_SHORT_HASH || want == PC_SHORT_TAG) CHECK(r.key_off + r.key_len == cut, "cut %zu: the slice's bounds", cut);
        }
      }

  const uint8_t mapped[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0xff, 0xff};
  for (uint64_t port : {8444ull, 70000ull, 1ull << 33})
    for (int kind = 0; kind < 3; ++kind)
      for (uint32_t lead = 0; lead < 8; ++lead) {
        std::vector<uint8_t> obj(20, 0x44);
        put_varint(obj, 3), put_varint(obj, 1);
        const size_t port_at = obj.size();
        put_varint(obj, port);
        const size_t host_at = obj.size();
        if (kind == 0) {
          obj.insert(obj.end(), mapped, mapped + 12);
          for (uint8_t b : {8, 8, 4, 4}) obj.push_back(b);
        } else if (kind == 1) {
          for (uint8_t b : {0xfd, 0x87, 0xd8, 0x7e, 0xeb, 0x43}) obj.push_back(b);
          for (int i = 0; i < 60; ++i) obj.push_back((uint8_t)rnd());
        } else {
          for (int i = 0; i < 16; ++i) obj.push_back((uint8_t)(0x20 + i));
        }
        for (size_t cut = 0; cut <= obj.size(); ++cut) {
          const uint32_t avail = (uint32_t)(cut < PC_ONION_HEAD ? cut : PC_ONION_HEAD);  // what the host uploads
          Exact block(lead + avail);
          std::memcpy(block.p + lead, obj.data(), avail);
          pc_rec r{};
          pcf::walk_onion(at_offset(block, lead, avail, (uint32_t)cut), &r);
          const size_t host = cut > host_at ? cut - host_at : 0;
          uint32_t want;
          if (cut > port_at && cut < host_at && port >= 253) want = PC_MALFORMED;
          else if (kind == 0) want = host < 12 ? PC_NO_HOST : host == 16 ? PC_PEER : PC_RAISES;
          else if (kind == 1) want = host < 6 ? PC_NO_HOST : PC_PEER;
          else want = host == 16 ? PC_PEER : PC_NO_HOST;
          CHECK(r.status == want, "onion kind %d port %llu cut %zu: status %u, want %u", kind, (unsigned long long)port, cut,
                r.status, want);
          if (want == PC_PEER) CHECK(r.host_off == host_at && r.host_len == host && r.port == port && r.stream == 1, "cut %zu: the peer's fields", cut);
        }
      }
}

int main() {
  watch_sets();
  compare_and_mix();
  walks();
  if (g_fail) {
    std::fprintf(stderr, "%d of %ld checks failed\n", g_fail, g_checks);
    return 1;
  }
  std::fprintf(stderr, "all proc checks passed (%ld)\n", g_checks);
  return 0;
}
