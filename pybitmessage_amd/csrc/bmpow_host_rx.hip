// bmpow_host_rx.hip -- the msg processing's host side: the bmpow_rx_* entry points (include/bmpow_rx.h)
// over the kernels of bmpow_rx.hip, bmpow_sig.hip, bmpow_ecies.hip (ec_prep_kernel) and bmpow_ident.hip.
#include "bmpow_host_rx.h"

#include "bmpow_rx_fmt.h"

// ---------------------------------------------------------------------------------------
// One call: the rows, sorted by the upper bound of their signed data's block count (descending, so a
// wave's 64 lanes hash alike), go through the device in sets of at most kSigSetObjects rows and
// kSigSetPoolBytes of padded blocks.  Per set the host copies the plaintexts side by side into one staging
// buffer (each at a multiple of 16 bytes) and uploads it with the row descriptors; nothing else crosses:
// the walk, the packing, both digests, the scalars, the key tables, the ladder, the combs, the
// identification and the final record are nine launches on the first shard's stream, then one download.
// The abort flag is read between sets.  The buffers are the call's own (DevBuf owners).
// ---------------------------------------------------------------------------------------
namespace bmhost {

int rx_grow_set(Shard& sh, SigBufs& b, RxBufs& x, uint32_t stride, uint64_t pool_chunks, uint64_t plain_chunks) {
  HIPTRY(x.rows.grow(sh.dev, stride));
  HIPTRY(x.plain.grow(sh.dev, plain_chunks));
  HIPTRY(x.keys.grow(sh.dev, (size_t)8 * stride));
  HIPTRY(x.recs.grow(sh.dev, stride));
  HIPTRY(x.versions.grow(sh.dev, stride));
  HIPTRY(x.streams.grow(sh.dev, stride));
  HIPTRY(x.pk.grow(sh.dev, stride));
  HIPTRY(x.flags.grow(sh.dev, stride));
  HIPTRY(x.ident.grow(sh.dev, stride));
  HIPTRY(b.sigs.grow(sh.dev, stride));
  HIPTRY(b.pool.grow(sh.dev, pool_chunks));
  HIPTRY(b.e.grow(sh.dev, (size_t)2 * stride));
  HIPTRY(b.u1.grow(sh.dev, (size_t)2 * stride));
  HIPTRY(b.dig.grow(sh.dev, (size_t)SG_DIGITS * stride));
  HIPTRY(b.flip.grow(sh.dev, stride));
  HIPTRY(b.tinf.grow(sh.dev, stride));
  HIPTRY(b.verdict.grow(sh.dev, stride));
  HIPTRY(b.pts.grow(sh.dev, stride));
  HIPTRY(b.tab.grow(sh.dev, (size_t)EC_ENTRIES * stride));
  HIPTRY(b.ok.grow(sh.dev, stride));
  HIPTRY(b.T.grow(sh.dev, stride));
  return 0;
}

int rx_launch_set(Shard& sh, SigBufs& b, RxBufs& x, const ec::ge* comb, uint32_t n, uint32_t stride, uint64_t plain_chunks,
                  uint64_t pool_chunks) {
  const uint8_t* d_plain = reinterpret_cast<const uint8_t*>(x.plain.get());
  HIPTRY(hipEventRecord(x.ev[0].get(), sh.stream));
  HIPTRY(rx_launch_walk(sh.stream, x.rows.get(), d_plain, n, stride, x.recs.get(), b.sigs.get(), b.pts.get(),
                        x.keys.get(), x.versions.get(), x.streams.get(), x.pk.get(), x.flags.get()));
  HIPTRY(rx_launch_pack(sh.stream, x.rows.get(), x.plain.get(), plain_chunks, b.sigs.get(), x.pk.get(), n, b.pool.get(),
                        pool_chunks));
  HIPTRY(hipEventRecord(x.ev[1].get(), sh.stream));
  HIPTRY(sg_launch_hash(sh.stream, b.sigs.get(), b.pool.get(), n, stride, b.e.get()));
  HIPTRY(hipEventRecord(x.ev[2].get(), sh.stream));
  HIPTRY(sg_launch_scalars(sh.stream, b.sigs.get(), b.e.get(), n, stride, 2, b.u1.get(), b.dig.get(), b.flip.get()));
  HIPTRY(hipEventRecord(x.ev[3].get(), sh.stream));
  HIPTRY(ec_launch_prep(sh.stream, b.pts.get(), n, stride, b.tab.get(), b.ok.get()));
  HIPTRY(sg_launch_ladder(sh.stream, b.tab.get(), n, stride, b.dig.get(), b.flip.get(), b.T.get(), b.tinf.get()));
  HIPTRY(sg_launch_comb(sh.stream, comb, b.sigs.get(), b.u1.get(), b.T.get(), b.tinf.get(), b.ok.get(), n, stride, 2,
                        b.verdict.get()));
  HIPTRY(hipEventRecord(x.ev[4].get(), sh.stream));
  HIPTRY(id_launch_derive(sh.stream, x.keys.get(), x.versions.get(), x.streams.get(), n, x.ident.get()));
  HIPTRY(hipEventRecord(x.ev[5].get(), sh.stream));
  HIPTRY(rx_launch_finish(sh.stream, x.rows.get(), d_plain, b.verdict.get(), x.flags.get(), x.ident.get(), n,
                          x.recs.get()));
  HIPTRY(hipEventRecord(x.ev[6].get(), sh.stream));
  return 0;
}

int rx_phase_times(const RxBufs& x, bmpow_rx_stats& st) {
  double* const acc[6] = {&st.walk_ms, &st.hash_ms, &st.scalar_ms, &st.curve_ms, &st.ident_ms, &st.finish_ms};
  for (int k = 0; k < 6; ++k)
    if (const int rc = sig_elapsed(*acc[k], x.ev[k], x.ev[k + 1]); rc < 0) return rc;
  return 0;
}

namespace {

bmpow_rx_stats g_rx_stats{};  // under g_mu

struct RxItem {
  uint32_t orig;
  uint32_t bound;  // rxf::signed_blocks_bound of its plaintext
};

int rx_run_locked(size_t n_all, const uint8_t* const* objs, const uint64_t* obj_lens, const uint8_t* const* plains,
                  const uint64_t* plain_lens, const uint8_t* to_ripes, bmpow_rx_msg_rec* out) {
  std::vector<RxItem> items(n_all);
  for (size_t i = 0; i < n_all; ++i) items[i] = {(uint32_t)i, rxf::signed_blocks_bound(plain_lens[i])};
  std::stable_sort(items.begin(), items.end(), [](const RxItem& a, const RxItem& b) { return a.bound > b.bound; });
  Shard& sh = g_shards[0];
  HIPTRY(hipSetDevice(sh.dev));
  const ec::ge* comb = nullptr;
  if (const int rc = addr_comb16_table(sh, &comb); rc < 0) return rc;
  SigBufs b;
  RxBufs x;
  for (Event& e : x.ev) HIPTRY(e.alloc(sh.dev));
  g_rx_stats.calls++;

  std::vector<rx_row> rows;
  std::vector<uint8_t> stage;
  std::vector<bmpow_rx_msg_rec> recs;
  size_t i0 = 0;
  while (i0 < items.size()) {
    if (g_abort.load()) return set_err(BMPOW_E_ABORTED, "aborted");
    size_t i1 = i0;
    uint64_t blocks = 0;
    while (i1 < items.size() && i1 - i0 < kSigSetObjects &&
           (i1 == i0 || (blocks + items[i1].bound) * 64 <= kSigSetPoolBytes))
      blocks += items[i1++].bound;
    if (blocks > 0xffffffffull) return set_err(BMPOW_E_ARG, "message pool above 2^32 blocks");
    const uint32_t n = (uint32_t)(i1 - i0), stride = (n + SG_BLOCK - 1) / SG_BLOCK * SG_BLOCK;
    rows.assign(n, rx_row{});
    uint64_t poff = 0;
    uint32_t blk = 0;
    for (uint32_t j = 0; j < n; ++j) {
      const RxItem& it = items[i0 + j];
      rx_row& r = rows[j];
      r.poff = poff;
      r.plen = (uint32_t)plain_lens[it.orig];
      r.blk = blk;
      r.hlen = (uint8_t)std::min<uint64_t>(obj_lens[it.orig], rxf::kHeadBytes);
      if (r.hlen) std::memcpy(r.head, objs[it.orig], r.hlen);
      std::memcpy(r.to_ripe, to_ripes + 20 * (size_t)it.orig, 20);
      poff += ((uint64_t)r.plen + 15) & ~15ull;
      blk += it.bound;
    }
    const uint64_t plain_bytes = std::max<uint64_t>(poff, 16);
    stage.resize(plain_bytes);
    bmsched::parallel_for(n, 1024, [&](size_t a, size_t z) {
      for (size_t j = a; j < z; ++j) {
        const rx_row& r = rows[j];
        uint8_t* dst = stage.data() + r.poff;
        if (r.plen) std::memcpy(dst, plains[items[i0 + j].orig], r.plen);
        std::memset(dst + r.plen, 0, (size_t)(-(int64_t)r.plen & 15));
      }
    });
    const uint64_t pool_chunks = std::max<uint64_t>(blocks * 4, 4), plain_chunks = plain_bytes / 16;
    if (const int rc = rx_grow_set(sh, b, x, stride, pool_chunks, plain_chunks); rc < 0) return rc;
    HIPTRY(hipMemcpyAsync(x.rows.get(), rows.data(), n * sizeof(rx_row), hipMemcpyHostToDevice, sh.stream));
    HIPTRY(hipMemcpyAsync(x.plain.get(), stage.data(), plain_bytes, hipMemcpyHostToDevice, sh.stream));
    if (const int rc = rx_launch_set(sh, b, x, comb, n, stride, plain_chunks, pool_chunks); rc < 0) return rc;
    recs.resize(n);
    HIPTRY(hipMemcpyAsync(recs.data(), x.recs.get(), n * sizeof(bmpow_rx_msg_rec), hipMemcpyDeviceToHost, sh.stream));
    HIPTRY(hipStreamSynchronize(sh.stream));
    if (const int rc = rx_phase_times(x, g_rx_stats); rc < 0) return rc;
    for (uint32_t j = 0; j < n; ++j) out[items[i0 + j].orig] = recs[j];
    g_rx_stats.sets++;
    g_rx_stats.launches += 9;
    i0 = i1;
  }
  return 0;
}

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
  if (rc >= 0) rc = rx_run_locked(n, objs, obj_lens, plains, plain_lens, to_ripes20, out);
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
