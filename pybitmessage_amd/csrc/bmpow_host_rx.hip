// bmpow_host_rx.hip -- the msg processing's host side: the bmpow_rx_* entry points (include/bmpow_rx.h)
// over the kernels of bmpow_rx.hip, bmpow_sig.hip, bmpow_ecies.hip (ec_prep_kernel) and bmpow_ident.hip.
#include "bmpow_host_rx.h"

#include "bmpow_rx_fmt.h"

// One call is run_rows (bmpow_host_rows.h) over the msg family; what is a msg's own is here: the bound of
// its signed data, its plaintext as the source, and the head and toRipe of its row.
namespace bmhost {
namespace {

bmpow_rx_stats g_rx_stats{};  // under g_mu

struct RxPolicy {
  const uint8_t* const* objs;
  const uint64_t* obj_lens;
  const uint8_t* const* plains;
  const uint64_t* plain_lens;
  const uint8_t* to_ripes;
  bmpow_rx_stats& stats;
  uint32_t bound(size_t i) const { return rxf::signed_blocks_bound(plain_lens[i]); }
  const uint8_t* source(size_t i) const { return plains[i]; }
  uint64_t len(size_t i) const { return plain_lens[i]; }
  void fill(rx_row& r, size_t i) const {
    r.hlen = (uint8_t)std::min<uint64_t>(obj_lens[i], rxf::kHeadBytes);
    if (r.hlen) std::memcpy(r.head, objs[i], r.hlen);
    std::memcpy(r.to_ripe, to_ripes + 20 * i, 20);
  }
};

}  // namespace
}  // namespace bmhost

using namespace bmhost;

extern "C" {

int bmpow_rx_msgs(size_t n, const uint8_t* const* objs, const uint64_t* obj_lens, const uint8_t* const* plains,
                  const uint64_t* plain_lens, const uint8_t* to_ripes20, bmpow_rx_msg_rec* out) {
  std::lock_guard<FairMutex> lk(g_mu);
  if (n == 0) return 0;
  if (!objs || !obj_lens || !plains || !plain_lens || !to_ripes20 || !out) return set_err(BMPOW_E_ARG, "null pointer");
  if (n > 0xffffffffull) return set_err(BMPOW_E_ARG, "too many msgs");
  for (size_t i = 0; i < n; ++i) {
    if ((obj_lens[i] && !objs[i]) || (plain_lens[i] && !plains[i])) return set_err(BMPOW_E_ARG, "null object or plaintext pointer");
    if (plain_lens[i] > (1ull << 31)) return set_err(BMPOW_E_ARG, "plaintext above 2^31 bytes");
  }
  const auto t_begin = std::chrono::steady_clock::now();
  int rc = init_locked();
  if (rc >= 0) rc = run_rows<RxFamily>(n, RxPolicy{objs, obj_lens, plains, plain_lens, to_ripes20, g_rx_stats}, out);
  if (rc > 0) rc = 0;
  g_rx_stats.rows += n;
  g_rx_stats.host_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
  return rc;
}

int bmpow_rx_walk_msg(const uint8_t* obj, size_t obj_len, const uint8_t* plain, size_t plain_len, const uint8_t* to_ripe20,
                      bmpow_rx_msg_rec* rec) {
  if ((obj_len && !obj) || (plain_len && !plain) || !to_ripe20 || !rec) return set_err(BMPOW_E_ARG, "null pointer");
  if (plain_len > (1ull << 31)) return set_err(BMPOW_E_ARG, "plaintext above 2^31 bytes");
  std::memset(rec, 0, sizeof *rec);
  uint32_t key_off = 0;
  rxf::walk(obj, (uint32_t)std::min<size_t>(obj_len, rxf::kHeadBytes), plain, plain_len, to_ripe20, *rec, key_off);
  if (rec->status != BMPOW_RX_OK) return 0;
  uint32_t r[8], s[8], x[8], y[8];
  return rxf::der_parse(plain + rec->sig_off, rec->sig_len, r, s) && rxf::load_key(plain + key_off, x, y) ? 1 : 0;
}

int bmpow_rx_get_stats(bmpow_rx_stats* out) {
  std::lock_guard<FairMutex> lk(g_mu);
  if (!out) return set_err(BMPOW_E_ARG, "null pointer");
  *out = g_rx_stats;
  return 0;
}

void bmpow_rx_reset_stats(void) {
  std::lock_guard<FairMutex> lk(g_mu);
  g_rx_stats = bmpow_rx_stats{};
}

}  // extern "C"
