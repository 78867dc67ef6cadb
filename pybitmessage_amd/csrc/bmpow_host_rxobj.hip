// bmpow_host_rxobj.hip -- the broadcast and pubkey processing's host side: bmpow_rx_objects,
// bmpow_rx_walk_object and their counters (include/bmpow_rx.h) over the kernels of bmpow_rxobj.hip,
// bmpow_sig.hip, bmpow_ecies.hip (ec_prep_kernel) and bmpow_ident.hip.
#include "bmpow_host_sig.h"

#include "../../include/bmpow_rx.h"
#include "bmpow_ident_kernels.h"
#include "bmpow_rx_fmt.h"
#include "bmpow_rxobj_kernels.h"

// ---------------------------------------------------------------------------------------
// One call, as bmpow_rx_msgs runs it (bmpow_host_rx.hip): the rows, sorted by the upper bound of their signed
// data's block count, go through the device in sets of at most kSigSetObjects rows and kSigSetPoolBytes of
// padded blocks; per set one staging buffer holds the sources side by side (the decrypted payload of a
// broadcast or an encrypted pubkey, the object itself of a clear pubkey), nine launches follow on the first
// shard's stream, then one download.  The abort flag is read between sets.
// ---------------------------------------------------------------------------------------
namespace bmhost {
namespace {

bmpow_rx_obj_stats g_rxo_stats{};  // under g_mu

struct RxoBufs {
  DevBuf<rxo_row> rows;
  DevBuf<uint4> plain, keys;
  DevBuf<bmpow_rx_obj_rec> recs;
  DevBuf<uint64_t> versions, streams;
  DevBuf<rxo_pk> pk;
  DevBuf<uint8_t> flags;
  DevBuf<bmpow_ident_rec> ident;
  Event ev[7];
};

struct RxoItem {
  uint32_t orig;
  uint32_t bound;  // rxf::signed_blocks_bound_obj of its source
};

int rxo_run_locked(size_t n_all, const uint8_t* kinds, const uint8_t* const* objs, const uint64_t* obj_lens,
                   const uint8_t* const* plains, const uint64_t* plain_lens, const uint8_t* expect32,
                   bmpow_rx_obj_rec* out) {
  // a clear pubkey's source is the object
  auto source = [&](size_t i) { return kinds[i] == BMPOW_RXO_KIND_PUBKEY ? objs[i] : plains[i]; };
  auto source_len = [&](size_t i) { return kinds[i] == BMPOW_RXO_KIND_PUBKEY ? obj_lens[i] : plain_lens[i]; };
  std::vector<RxoItem> items(n_all);
  for (size_t i = 0; i < n_all; ++i) items[i] = {(uint32_t)i, rxf::signed_blocks_bound_obj(source_len(i))};
  std::stable_sort(items.begin(), items.end(), [](const RxoItem& a, const RxoItem& b) { return a.bound > b.bound; });
  Shard& sh = g_shards[0];
  HIPTRY(hipSetDevice(sh.dev));
  const ec::ge* comb = nullptr;
  if (const int rc = addr_comb16_table(sh, &comb); rc < 0) return rc;
  SigBufs b;
  RxoBufs x;
  for (Event& e : x.ev) HIPTRY(e.alloc(sh.dev));
  g_rxo_stats.calls++;

  std::vector<rxo_row> rows;
  std::vector<uint8_t> stage;
  std::vector<bmpow_rx_obj_rec> recs;
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
    rows.assign(n, rxo_row{});
    uint64_t poff = 0;
    uint32_t blk = 0;
    for (uint32_t j = 0; j < n; ++j) {
      const RxoItem& it = items[i0 + j];
      rxo_row& r = rows[j];
      r.poff = poff;
      r.plen = (uint32_t)source_len(it.orig);
      r.blk = blk;
      r.kind = kinds[it.orig];
      r.hlen = (uint8_t)std::min<uint64_t>(obj_lens[it.orig], rxf::kObjHeadBytes);
      if (r.hlen) std::memcpy(r.head, objs[it.orig], r.hlen);
      std::memcpy(r.expect, expect32 + 32 * (size_t)it.orig, 32);
      poff += ((uint64_t)r.plen + 15) & ~15ull;
      blk += it.bound;
    }
    const uint64_t plain_bytes = std::max<uint64_t>(poff, 16);
    stage.resize(plain_bytes);
    bmsched::parallel_for(n, 1024, [&](size_t a, size_t z) {
      for (size_t j = a; j < z; ++j) {
        const rxo_row& r = rows[j];
        uint8_t* dst = stage.data() + r.poff;
        if (r.plen) std::memcpy(dst, source(items[i0 + j].orig), r.plen);
        std::memset(dst + r.plen, 0, (size_t)(-(int64_t)r.plen & 15));
      }
    });
    const uint64_t pool_chunks = std::max<uint64_t>(blocks * 4, 4), plain_chunks = plain_bytes / 16;
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
    HIPTRY(hipMemcpyAsync(x.rows.get(), rows.data(), n * sizeof(rxo_row), hipMemcpyHostToDevice, sh.stream));
    HIPTRY(hipMemcpyAsync(x.plain.get(), stage.data(), plain_bytes, hipMemcpyHostToDevice, sh.stream));
    const uint8_t* d_plain = reinterpret_cast<const uint8_t*>(x.plain.get());
    HIPTRY(hipEventRecord(x.ev[0].get(), sh.stream));
    HIPTRY(rxo_launch_walk(sh.stream, x.rows.get(), d_plain, n, stride, x.recs.get(), b.sigs.get(), b.pts.get(),
                           x.keys.get(), x.versions.get(), x.streams.get(), x.pk.get(), x.flags.get()));
    HIPTRY(rxo_launch_pack(sh.stream, x.rows.get(), x.plain.get(), plain_chunks, b.sigs.get(), x.pk.get(), n,
                           b.pool.get(), pool_chunks));
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
    HIPTRY(rxo_launch_finish(sh.stream, x.rows.get(), d_plain, b.verdict.get(), x.flags.get(), x.ident.get(), n,
                             x.recs.get()));
    HIPTRY(hipEventRecord(x.ev[6].get(), sh.stream));
    recs.resize(n);
    HIPTRY(hipMemcpyAsync(recs.data(), x.recs.get(), n * sizeof(bmpow_rx_obj_rec), hipMemcpyDeviceToHost, sh.stream));
    HIPTRY(hipStreamSynchronize(sh.stream));
    double* const acc[6] = {&g_rxo_stats.walk_ms,  &g_rxo_stats.hash_ms,  &g_rxo_stats.scalar_ms,
                            &g_rxo_stats.curve_ms, &g_rxo_stats.ident_ms, &g_rxo_stats.finish_ms};
    for (int k = 0; k < 6; ++k)
      if (const int rc = sig_elapsed(*acc[k], x.ev[k], x.ev[k + 1]); rc < 0) return rc;
    for (uint32_t j = 0; j < n; ++j) out[items[i0 + j].orig] = recs[j];
    g_rxo_stats.sets++;
    g_rxo_stats.launches += 9;
    i0 = i1;
  }
  return 0;
}

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
  if (rc >= 0) rc = rxo_run_locked(n, kinds, objs, obj_lens, plains, plain_lens, expect32, out);
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
