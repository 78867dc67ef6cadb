// inv_sim.cpp -- the slot steps, the key load and the payload walk of the inventory sets
// (pybitmessage_amd/csrc/bmpow_inv_fmt.h) on the host, as a stand-alone program: tests/test_inv_native.py builds
// it with g++ under AddressSanitizer + UBSan and runs it.  One thread drives claim / finalize / lookup / remove /
// rebuild through the functions the kernels call, on tables of 8 to 64 slots, against std::unordered_map; the
// key load and the walk work from heap blocks of exactly the bytes they may read.  One thread cannot show the
// kernels' races: what a compare-and-swap loses to, and which row of equal keys comes first, are only ever the
// sequential order here.  Loads neither HIP nor the library.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "bmpow_inv_fmt.h"

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

static uint64_t g_rng = 0x2545F4914F6CDD1DULL;
static uint64_t rnd() {
  g_rng ^= g_rng << 13, g_rng ^= g_rng >> 7, g_rng ^= g_rng << 17;
  return g_rng;
}

// key number id: the first 16 bytes are shared by ids 4 apart (equal tags), the rest differ
static void key_bytes(uint32_t id, uint8_t out[32]) {
  for (int i = 0; i < 32; ++i) out[i] = (uint8_t)(((i < 16 ? id % 4 : id) * 0x9E3779B1u + 0x7F4A7C15u * (uint32_t)i) >> 13);
  out[31] = (uint8_t)id, out[30] = (uint8_t)(id >> 8);
}

struct HostTable {
  std::vector<uint64_t> state, keys;
  std::vector<iv_val> vals;
  ivf::Table t;
  HostTable(uint32_t log2, uint64_t seed) : state(1u << log2, 0), keys(4u << log2, 0), vals(1u << log2) {
    t = ivf::Table{state.data(), keys.data(), vals.data(), seed, log2};
  }
};

typedef std::unordered_map<std::string, iv_val> Model;
static std::string skey(const uint8_t k[32]) { return std::string((const char*)k, 32); }

// one batch insert the way the host unit runs it: every row claims, then every row finalizes
static void add_batch(HostTable& h, Model& model, const std::vector<uint32_t>& ids, uint64_t stamp, uint64_t* live) {
  const uint32_t n = (uint32_t)ids.size();
  Exact in(32 * (size_t)n);
  for (uint32_t i = 0; i < n; ++i) key_bytes(ids[i], in.p + 32 * i);
  const ivf::Rows rows{(const uint64_t*)in.p, 32ull * n, nullptr, n};
  std::vector<uint32_t> first(n, IV_NONE), claim(n), slot(n);
  uint32_t probes = 0;
  bool bad = false;
  for (uint32_t i = 0; i < n; ++i) {
    uint64_t k[4];
    CHECK(ivf::row_key(rows, i, k), "row %u outside its upload", i);
    claim[i] = ivf::claim(h.t, rows, i, k, first.data(), &slot[i], &probes, &bad);
  }
  CHECK(!bad, "a claim ran over every slot");
  for (uint32_t i = 0; i < n; ++i) {
    uint64_t k[4];
    ivf::row_key(rows, i, k);
    const std::string sk = skey(in.p + 32 * i);
    const bool had = model.count(sk) != 0;
    uint32_t lowest = i;
    for (uint32_t j = 0; j < i; ++j)
      if (ids[j] == ids[i]) {
        lowest = j;
        break;
      }
    if (had) {
      CHECK(claim[i] == IV_PRESENT, "row %u: key resident, claim %u", i, claim[i]);
      continue;
    }
    CHECK(claim[i] < n && first[claim[i]] == lowest, "row %u: claim %u first %u, lowest %u", i, claim[i],
          claim[i] < n ? first[claim[i]] : 0u, lowest);
    if (claim[i] == i) {
      const uint32_t f = first[i];
      ivf::finalize_slot(h.t, slot[i], k, iv_val{stamp + f, ids[f] % 3, f});
      ++*live;
    }
  }
  for (uint32_t i = 0; i < n; ++i) {
    const std::string sk = skey(in.p + 32 * i);
    if (!model.count(sk)) model[sk] = iv_val{stamp + i, ids[i] % 3, i};  // the lowest row: the loop goes up
  }
}

static void check_all(HostTable& h, const Model& model, uint32_t universe) {
  for (uint32_t id = 0; id < universe; ++id) {
    uint8_t kb[32];
    key_bytes(id, kb);
    uint64_t k[4];
    std::memcpy(k, kb, 32);
    uint32_t probes = 0;
    bool bad = false;
    const uint32_t s = ivf::lookup(h.t, k, &probes, &bad);
    CHECK(!bad, "lookup of %u ran over every slot", id);
    const Model::const_iterator it = model.find(skey(kb));
    CHECK((s != IV_NONE) == (it != model.end()), "key %u: slot %u, model %d", id, s, (int)(it != model.end()));
    if (s != IV_NONE && it != model.end()) {
      const iv_val v = h.vals[s];
      CHECK(v.expires == it->second.expires && v.stream == it->second.stream && v.aux == it->second.aux,
            "key %u: value (%llu, %u, %u)", id, (unsigned long long)v.expires, v.stream, v.aux);
    }
  }
  for (uint64_t w : h.state) CHECK(!ivf::is_pending(w), "a pending word outlived its insert");
}

static void table_sequences() {
  for (int round = 0; round < 200; ++round) {
    const uint64_t seed = rnd() | 1;
    const uint32_t universe = 40;
    uint32_t log2 = 3;
    HostTable* h = new HostTable(log2, seed);
    Model model;
    uint64_t live = 0, tombs = 0;
    for (int op = 0; op < 60; ++op) {
      const uint64_t r = rnd();
      const uint32_t n = 1 + (uint32_t)((r >> 8) % 8);
      std::vector<uint32_t> ids(n);
      for (uint32_t i = 0; i < n; ++i) ids[i] = (uint32_t)(rnd() % universe);
      if (r % 4 < 2) {  // add, behind the host unit's load bound
        uint64_t kept = live;
        if (2 * (live + tombs + n) > (1ull << log2)) {
          uint32_t l2 = log2;
          while ((1ull << l2) < 2 * (live + n)) ++l2;
          if (l2 > 6) continue;  // this model stops at 64 slots
          HostTable* to = new HostTable(l2, seed);
          kept = 0;
          for (uint32_t s = 0; s < (1u << log2); ++s) {
            if (!ivf::is_full(h->state[s])) continue;
            const uint64_t k[4] = {h->keys[4 * s], h->keys[4 * s + 1], h->keys[4 * s + 2], h->keys[4 * s + 3]};
            uint32_t probes = 0;
            CHECK(ivf::reinsert(to->t, k, h->vals[s], &probes), "rebuild ran over every slot");
            ++kept;
          }
          CHECK(kept == live, "rebuild kept %llu of %llu", (unsigned long long)kept, (unsigned long long)live);
          delete h;
          h = to, log2 = l2, tombs = 0;
          check_all(*h, model, universe);
        }
        add_batch(*h, model, ids, 1000ull * (uint64_t)(round * 100 + op), &live);
      } else if (r % 4 == 2) {  // remove: every lookup first, then the tombstones
        std::vector<uint32_t> slot(n);
        for (uint32_t i = 0; i < n; ++i) {
          uint8_t kb[32];
          key_bytes(ids[i], kb);
          uint64_t k[4];
          std::memcpy(k, kb, 32);
          uint32_t probes = 0;
          bool bad = false;
          slot[i] = ivf::lookup(h->t, k, &probes, &bad);
          CHECK((slot[i] != IV_NONE) == (model.count(skey(kb)) != 0), "remove: key %u", ids[i]);
        }
        for (uint32_t i = 0; i < n; ++i) {
          if (slot[i] == IV_NONE) continue;
          if (ivf::bury(h->t, slot[i])) --live, ++tombs;
          uint8_t kb[32];
          key_bytes(ids[i], kb);
          model.erase(skey(kb));
        }
      }
      CHECK(live == model.size(), "live %llu, model %zu", (unsigned long long)live, model.size());
      check_all(*h, model, universe);
    }
    delete h;
  }
}

static void key_loads() {
  // an item behind `front` bytes, in a block that ends on the item's last byte, for every residue
  for (size_t front = 0; front < 24; ++front) {
    Exact block(front + 32);
    for (size_t i = 0; i < front + 32; ++i) block.p[i] = (uint8_t)(i * 37 + front);
    uint64_t k[4], want[4];
    ivf::load_key((const uint64_t*)block.p, front + 32, front, k);
    std::memcpy(want, block.p + front, 32);
    CHECK(ivf::key_eq(k, want), "front %zu: the key's words", front);
    // and with rows behind it, the last of which ends the block
    Exact two(front + 64);
    for (size_t i = 0; i < front + 64; ++i) two.p[i] = (uint8_t)(i * 11 + 3);
    const uint32_t offs[2] = {(uint32_t)front, (uint32_t)front + 32};
    const ivf::Rows rows{(const uint64_t*)two.p, front + 64, offs, 2};
    for (uint32_t i = 0; i < 2; ++i) {
      CHECK(ivf::row_key(rows, i, k), "row inside");
      std::memcpy(want, two.p + offs[i], 32);
      CHECK(ivf::key_eq(k, want), "front %zu row %u", front, i);
    }
    const uint32_t past[1] = {(uint32_t)front + 33};
    const ivf::Rows out{(const uint64_t*)two.p, front + 64, past, 1};
    CHECK(!ivf::row_key(out, 0, k), "a row past the upload is refused");
  }
}

static void walks() {
  // count c spelled in each width, m items behind it, every cut length
  const struct {
    uint64_t count;
    uint8_t head[9];
    size_t used;
  } heads[] = {{3, {3}, 1}, {0, {0}, 1}, {253, {0xfd, 0, 253}, 3}, {65536, {0xfe, 0, 1, 0, 0}, 5},
               {1ull << 32, {0xff, 0, 0, 0, 1, 0, 0, 0, 0}, 9}};
  for (const auto& hd : heads)
    for (size_t m = 0; m <= 4; ++m) {
      std::vector<uint8_t> whole(hd.head, hd.head + hd.used);
      whole.resize(hd.used + 32 * m, 0x5C);
      for (size_t cut = 0; cut <= whole.size(); ++cut) {
        Exact block(cut);
        if (cut) std::memcpy(block.p, whole.data(), cut);
        const ivf::Walk w = ivf::walk(block.p, cut);
        if (cut == 0) {
          CHECK(w.status == IV_WALK_OK && w.count == 1 && w.at == 0 && w.full == 0 && w.tail == 0, "the empty payload");
          continue;
        }
        if (cut < hd.used) {
          CHECK(w.status == IV_WALK_MALFORMED, "a truncated count (width %zu, cut %zu)", hd.used, cut);
          continue;
        }
        const uint64_t count = hd.count ? hd.count : 1, avail = cut - hd.used;
        CHECK(w.status == IV_WALK_OK && w.count == count && w.at == hd.used, "width %zu cut %zu", hd.used, cut);
        CHECK(w.full == (avail / 32 < count ? avail / 32 : count), "full items: width %zu cut %zu", hd.used, cut);
        CHECK(w.tail == (w.full < count ? avail % 32 : 0), "the short item: width %zu cut %zu", hd.used, cut);
      }
    }
  const uint8_t bad[][9] = {{0xfd, 0, 252}, {0xfe, 0, 0, 0xff, 0xff}, {0xff, 0, 0, 0, 0, 0xff, 0xff, 0xff, 0xff}};
  const size_t bad_len[] = {3, 5, 9};
  for (int i = 0; i < 3; ++i) {
    Exact block(bad_len[i] + 32);
    std::memcpy(block.p, bad[i], bad_len[i]);
    CHECK(ivf::walk(block.p, bad_len[i] + 32).status == IV_WALK_MALFORMED, "a non-minimal count (%d)", i);
  }
}

int main() {
  table_sequences();
  key_loads();
  walks();
  if (g_fail) {
    std::fprintf(stderr, "%d of %ld checks failed\n", g_fail, g_checks);
    return 1;
  }
  std::fprintf(stderr, "all inv checks passed (%ld)\n", g_checks);
  return 0;
}
