// rxobj_sim.cpp -- the byte-oriented half of the broadcast and pubkey processing
// (pybitmessage_amd/csrc/bmpow_rx_fmt.h: the three walks, the prefix of up to 62 bytes and the packing of
// signedData from a source that may start at byte 8) on the CPU, called as the kernels of bmpow_rxobj.hip call
// it.
//
// A stand-alone program: g++ -fsanitize=address,undefined, its own main, loaded into nothing.  Every buffer
// the header reads is a heap block of exactly the size the device's is, so a read past a plaintext, past an
// object's head or past a pool slot is an error here.
//   rxobj_sim ROWS.txt      one row per line:
//       <kind> <status the walk must leave> <keys_hashed> <object hex | -> <plaintext hex | ->
// On top of the rows: the first row of each kind whose walk gets through with a signature is cut at every
// length 0 .. its own and walked, parsed and key-loaded again; and the pack routine's output is compared with
// prefix || data || 0x80 || zeros || the bit length for every signed length 130 .. 400 under every prefix
// length 0, 14 .. 22 and 46 .. 62, with the source read from byte 0 and from byte 8, with and without bytes
// behind the signed part.
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

// the whole of what rxo_walk_kernel does with one row; returns the walk's status
int walk_row(uint32_t kind, const std::vector<uint8_t>& obj, const std::vector<uint8_t>& plain_in, bmpow_rx_obj_rec& rec,
             bool& real) {
  const Exact head(obj.data(), obj.size() < rxf::kObjHeadBytes ? obj.size() : rxf::kObjHeadBytes);
  const std::vector<uint8_t>& source = kind == BMPOW_RXO_KIND_PUBKEY ? obj : plain_in;
  const Exact src(source.data(), source.size());
  std::memset(&rec, 0, sizeof rec);
  rxf::obj_walk w;
  rxf::walk_object(kind, head.p.get(), (uint32_t)head.n, src.p.get(), src.n, rec, w);
  real = false;
  CHECK(rec.kind == kind && (!w.sig || w.keys) && w.keys == (rec.keys_hashed == 1), "flags of the walk");
  CHECK(rec.payload_off <= head.n && rec.tag_off <= rec.payload_off, "header offsets past the head");
  CHECK(rec.prefix_len <= 62 && rec.end_of_pubkey <= src.n && rec.bottom <= src.n, "offsets past the source");
  CHECK((uint64_t)rec.sig_off + rec.sig_len <= src.n && (uint64_t)rec.msg_off + rec.msg_len <= src.n, "slice past the source");
  if (w.keys) CHECK((uint64_t)w.key_off + 128 <= src.n, "keys past the source");
  uint32_t pre[rxf::kObjPrefixWords];
  rxf::put_prefix_obj(head.p.get(), rec.payload_off, pre);
  uint8_t prefix[64];
  std::memcpy(prefix, pre, 64);
  if (kind != BMPOW_RXO_KIND_PUBKEY)
    for (uint32_t i = 0; i < 64; ++i)
      CHECK(prefix[i] == (i < rec.prefix_len ? head.p.get()[8 + i] : 0), "prefix byte %u", i);
  if (w.sig) {
    uint32_t r[8], s[8], x[8], y[8];
    CHECK(rec.status == BMPOW_RXO_OK && (uint64_t)w.skip + rec.bottom <= src.n, "signed bytes past the source");
    real = rxf::der_parse(src.p.get() + rec.sig_off, rec.sig_len, r, s) && rxf::load_key(src.p.get() + w.key_off, x, y);
    CHECK(rxf::signed_blocks(rec.prefix_len, rec.bottom) <= rxf::signed_blocks_bound_obj(src.n), "more blocks than the host reserved");
  }
  return rec.status;
}

struct HostSrc {  // a pool slot: the source in a block of its length rounded up to 16 bytes
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
  int compared = 0, widths = 0;
  for (uint32_t plen = 0; plen <= 62; ++plen) {
    if (!(plen == 0 || (plen >= 14 && plen <= 22) || plen >= 46)) continue;
    ++widths;
    std::vector<uint8_t> obj(8 + plen);
    for (size_t i = 0; i < obj.size(); ++i) obj[i] = (uint8_t)(0xa0 + i);
    const Exact head(obj.data(), obj.size());
    uint32_t pre[rxf::kObjPrefixWords];
    rxf::put_prefix_obj(head.p.get(), 8 + plen, pre);
    uint8_t prefix[64];
    std::memcpy(prefix, pre, 64);
    for (uint32_t skip = 0; skip <= 8; skip += 8)
      for (uint32_t total = 130; total <= 400; ++total)
        for (uint32_t behind = 0; behind <= 75; behind += 75) {  // source bytes behind the signed part, or none
          const uint32_t bottom = total - plen, len = skip + bottom + behind, slot_bytes = (len + 15) & ~15u;
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
          std::memcpy(want.data() + plen, slot.get() + skip, bottom);
          want[total] = 0x80;
          const uint64_t bits = 8ull * total;
          for (int j = 0; j < 8; ++j) want[want.size() - 8 + j] = (uint8_t)(bits >> (56 - 8 * j));
          for (uint32_t c = 0; c < 4 * nblk; ++c) {
            uint32_t w[4];
            rxf::pack_chunk_n<(int)rxf::kObjPrefixWords>(c, nblk, pre, plen, bottom, skip, src, w);
            std::memcpy(got.data() + 16 * (size_t)c, w, 16);
          }
          CHECK(got == want, "packed blocks of %u signed bytes, prefix %u, skip %u, %u behind", total, plen, skip, behind);
          ++compared;
        }
  }
  CHECK(widths == 27 && compared == 27 * 2 * 271 * 2, "pack cases: %d widths, %d compared", widths, compared);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: rxobj_sim ROWS.txt\n");
    return 2;
  }
  pack_checks();
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) {
    std::fprintf(stderr, "cannot open %s\n", argv[1]);
    return 2;
  }
  static char kind_s[8], want[16], hashed[8], obj_s[1 << 20], plain_s[1 << 20];
  int rows = 0;
  bool swept[3] = {false, false, false};
  while (std::fscanf(f, "%7s %15s %7s %1048575s %1048575s", kind_s, want, hashed, obj_s, plain_s) == 5) {
    const std::vector<uint8_t> obj = unhex(obj_s), plain = unhex(plain_s);
    const uint32_t kind = (uint32_t)std::atoi(kind_s);
    CHECK(kind <= 2, "malformed row %d", rows);
    if (kind > 2) break;
    bmpow_rx_obj_rec rec;
    bool real;
    const int status = walk_row(kind, obj, plain, rec, real);
    CHECK(status == std::atoi(want) && rec.keys_hashed == std::atoi(hashed), "row %d: status %d hashed %d, wanted %s %s", rows,
          status, (int)rec.keys_hashed, want, hashed);
    if (status == BMPOW_RXO_OK && real && !swept[kind]) {
      swept[kind] = true;
      const std::vector<uint8_t>& whole = kind == BMPOW_RXO_KIND_PUBKEY ? obj : plain;
      for (size_t cut = 0; cut <= whole.size(); ++cut) {
        const std::vector<uint8_t> q(whole.begin(), whole.begin() + cut);
        const int st = kind == BMPOW_RXO_KIND_PUBKEY ? walk_row(kind, q, plain, rec, real) : walk_row(kind, obj, q, rec, real);
        CHECK(st >= 0 && st <= BMPOW_RXO_KEY_SHORT, "status %d", st);
        CHECK(cut == whole.size() ? real : !real, "kind %u cut at %zu of %zu: real = %d", kind, cut, whole.size(), (int)real);
      }
      // the header alone, cut at every length too
      for (size_t cut = 0; cut <= obj.size() && cut <= 80; ++cut) {
        const Exact head(obj.data(), cut < rxf::kObjHeadBytes ? cut : rxf::kObjHeadBytes);
        std::memset(&rec, 0, sizeof rec);
        if (kind == BMPOW_RXO_KIND_BROADCAST) rxf::walk_broadcast_header(head.p.get(), (uint32_t)head.n, rec);
        else rxf::walk_pubkey_v4_header(head.p.get(), (uint32_t)head.n, rec);
        CHECK(rec.payload_off <= head.n && rec.tag_off <= rec.payload_off, "header cut at %zu", cut);
        uint32_t pre[rxf::kObjPrefixWords];
        rxf::put_prefix_obj(head.p.get(), rec.payload_off, pre);
      }
    }
    ++rows;
  }
  std::fclose(f);
  CHECK(swept[0] && swept[1] && swept[2], "no row to sweep: %d %d %d", (int)swept[0], (int)swept[1], (int)swept[2]);
  if (g_fail) {
    std::fprintf(stderr, "%d checks failed\n", g_fail);
    return 1;
  }
  std::fprintf(stderr, "all rxobj checks passed (%d rows)\n", rows);
  return 0;
}
