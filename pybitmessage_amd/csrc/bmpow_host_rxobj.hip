// bmpow_host_rxobj.hip -- the broadcast and pubkey processing's host side: bmpow_rx_objects,
// bmpow_rx_walk_object and their counters (include/bmpow_rx.h) over the kernels of bmpow_rxobj.hip,
// bmpow_sig.hip, bmpow_ecies.hip (ec_prep_kernel) and bmpow_ident.hip.
#include "bmpow_host_rxobj.h"

// One call is run_rows (bmpow_host_rows.h) over the object family; what is an object's own is here: the bound
// of its signed data, its source (the decrypted payload of a broadcast or an encrypted pubkey, the object
// itself of a clear pubkey), and the kind, head and expected ripe or tag of its row.
namespace bmhost {
namespace {

bmpow_rx_obj_stats g_rxo_stats{};  // under g_mu

struct RxoPolicy {
  const uint8_t* kinds;
  const uint8_t* const* objs;
  const uint64_t* obj_lens;
  const uint8_t* const* plains;
  const uint64_t* plain_lens;
  const uint8_t* expect32;
  bmpow_rx_obj_stats& stats;
  uint32_t bound(size_t i) const { return rxf::signed_blocks_bound_obj(len(i)); }
  // a clear pubkey's source is the object
  const uint8_t* source(size_t i) const { return kinds[i] == BMPOW_RXO_KIND_PUBKEY ? objs[i] : plains[i]; }
  uint64_t len(size_t i) const { return kinds[i] == BMPOW_RXO_KIND_PUBKEY ? obj_lens[i] : plain_lens[i]; }
  void fill(rxo_row& r, size_t i) const {
    r.kind = kinds[i];
    r.hlen = (uint8_t)std::min<uint64_t>(obj_lens[i], rxf::kObjHeadBytes);
    if (r.hlen) std::memcpy(r.head, objs[i], r.hlen);
    std::memcpy(r.expect, expect32 + 32 * i, 32);
  }
};

bool known_kind(int kind) {
  return kind == BMPOW_RXO_KIND_BROADCAST || kind == BMPOW_RXO_KIND_PUBKEY_V4 || kind == BMPOW_RXO_KIND_PUBKEY;
}

}  // namespace
}  // namespace bmhost

using namespace bmhost;

extern "C" {

int bmpow_rx_objects(size_t n, const uint8_t* kinds, const uint8_t* const* objs, const uint64_t* obj_lens,
                     const uint8_t* const* plains, const uint64_t* plain_lens, const uint8_t* expect32,
                     bmpow_rx_obj_rec* out) {
  std::lock_guard<FairMutex> lk(g_mu);
  if (n == 0) return 0;
  if (!kinds || !objs || !obj_lens || !plains || !plain_lens || !expect32 || !out) return set_err(BMPOW_E_ARG, "null pointer");
  if (n > 0xffffffffull) return set_err(BMPOW_E_ARG, "too many objects");
  for (size_t i = 0; i < n; ++i) {
    if (!known_kind(kinds[i])) return set_err(BMPOW_E_ARG, "unknown kind of row");
    const bool clear = kinds[i] == BMPOW_RXO_KIND_PUBKEY;
    if ((obj_lens[i] && !objs[i]) || (!clear && plain_lens[i] && !plains[i]))
      return set_err(BMPOW_E_ARG, "null object or plaintext pointer");
    if (obj_lens[i] > (1ull << 31)) return set_err(BMPOW_E_ARG, "object above 2^31 bytes");
    if (!clear && plain_lens[i] > (1ull << 31)) return set_err(BMPOW_E_ARG, "plaintext above 2^31 bytes");
  }
  const auto t_begin = std::chrono::steady_clock::now();
  int rc = init_locked();
  if (rc >= 0)
    rc = run_rows<RxoFamily>(n, RxoPolicy{kinds, objs, obj_lens, plains, plain_lens, expect32, g_rxo_stats}, out);
  if (rc > 0) rc = 0;
  g_rxo_stats.rows += n;
  g_rxo_stats.host_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
  return rc;
}

int bmpow_rx_walk_object(int kind, const uint8_t* obj, size_t obj_len, const uint8_t* plain, size_t plain_len,
                         const uint8_t* expect32, bmpow_rx_obj_rec* rec) {
  (void)expect32;  // the comparisons are the device's: the walk decides nothing by it
  if (!known_kind(kind)) return set_err(BMPOW_E_ARG, "unknown kind of row");
  if ((obj_len && !obj) || !rec) return set_err(BMPOW_E_ARG, "null pointer");
  if (obj_len > (1ull << 31)) return set_err(BMPOW_E_ARG, "object above 2^31 bytes");
  if (plain && plain_len > (1ull << 31)) return set_err(BMPOW_E_ARG, "plaintext above 2^31 bytes");
  std::memset(rec, 0, sizeof *rec);
  rec->kind = (uint8_t)kind;
  const uint32_t hlen = (uint32_t)std::min<size_t>(obj_len, rxf::kObjHeadBytes);
  if (kind != BMPOW_RXO_KIND_PUBKEY && !plain) {  // the header alone
    if (plain_len) return set_err(BMPOW_E_ARG, "null plaintext pointer");
    if (kind == BMPOW_RXO_KIND_BROADCAST) rxf::walk_broadcast_header(obj, hlen, *rec);
    else rxf::walk_pubkey_v4_header(obj, hlen, *rec);
    return 0;
  }
  const uint8_t* src = kind == BMPOW_RXO_KIND_PUBKEY ? obj : plain;
  const size_t src_len = kind == BMPOW_RXO_KIND_PUBKEY ? obj_len : plain_len;
  rxf::obj_walk w;
  rxf::walk_object((uint32_t)kind, obj, hlen, src, src_len, *rec, w);
  if (!w.sig) return 0;
  uint32_t r[8], s[8], x[8], y[8];
  return rxf::der_parse(src + rec->sig_off, rec->sig_len, r, s) && rxf::load_key(src + w.key_off, x, y) ? 1 : 0;
}

int bmpow_rx_obj_get_stats(bmpow_rx_obj_stats* out) {
  std::lock_guard<FairMutex> lk(g_mu);
  if (!out) return set_err(BMPOW_E_ARG, "null pointer");
  *out = g_rxo_stats;
  return 0;
}

void bmpow_rx_obj_reset_stats(void) {
  std::lock_guard<FairMutex> lk(g_mu);
  g_rxo_stats = bmpow_rx_obj_stats{};
}

}  // extern "C"
