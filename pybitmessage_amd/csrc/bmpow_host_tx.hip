// bmpow_host_tx.hip -- the host unit of the one-call assembly of outgoing objects: argument and range
// checks, random draws, the set loop that takes head and body bytes through packing, hashing, signing, the
// tail, the ECIES key agreement, the seal and the payload's SHA-512 on the device, the scatter of the
// payloads, and the entry points of include/bmpow_tx.h.
#include "bmpow_host_sendkit.h"

#include "../../include/bmpow_tx.h"
#include "bmpow_seal_kernels.h"
#include "bmpow_seal_plan.h"
#include "bmpow_tx_fmt.h"
#include "bmpow_tx_kernels.h"

// ---------------------------------------------------------------------------------------
// One call: the rows that can go to the device are ordered once -- the sealed ones first, each kind by body
// length, descending, so a wave's 64 lanes hash and encrypt alike -- and cut by bmseal::plan_slots into sets
// of at most kTxSetRows rows and kTxSetPoolBytes of slots (a row's slot is the seal's, for the longest
// tail).  The padded signed data of a set is never larger than its slots (134 against 192 bytes beyond the
// body), so the one cut bounds both pools.  Per set: the bodies are packed into the staging pool and go up
// once, with the row structs, keys, nonces, ephemeral keys, IVs and recipient points; then the launches, one
// per phase, the sealed rows' (the set's first ns) between the tail and the finish; the pool and the
// records come down.  The abort flag is read between sets and before the ladder.  The buffers are the
// call's own, sized once for its largest set: TxBufs, and a KeySet (bmpow_host_sendkit.h) for the sealed rows'
// key agreement; those that held a private key, a nonce, an ephemeral key, a derived key or plaintext zero
// themselves before they are released, on the device (WipeDevBuf) and on the host (Wiped, WipedBytes).
// Everything runs on the first shard's device and stream.
// ---------------------------------------------------------------------------------------
namespace bmhost {
namespace {

constexpr size_t kTxSetRows = 1u << 18;
constexpr size_t kTxSetPoolBytes = 256ull << 20;

bmpow_tx_stats g_tx_stats{};  // under g_mu

struct TxBufs {  // one call's buffers on the device and their staging copies, beside the sealed rows' KeySet
  DevBuf<tx_row> rows;
  DevBuf<sl_row> sl;
  WipeDevBuf<uint8_t> pool;
  WipeDevBuf<uint4> hpool;
  DevBuf<uint8_t> ok8;
  DevBuf<uint4> iv;
  DevBuf<sg_sig> sigs;
  WipeDevBuf<sg_kw> kw;
  WipeDevBuf<sc> d;
  DevBuf<sc> e, rs;
  DevBuf<ec::ge> pt;
  DevBuf<uint32_t> blob_len;
  DevBuf<bmpow_tx_rec> recs;
  Event ev[7];
  WipedBytes host;  // the pool's staging copy: packed, uploaded, downloaded over, scattered
  Wiped<sg_kw> hkw;
  Wiped<sc> hd;
  std::vector<tx_row> hrows;
  std::vector<uint8_t> hiv;
  std::vector<bmpow_tx_rec> hrecs;
};

// The caller's arrays, indexed by the caller's row.
struct TxCall {
  const uint8_t* kinds;
  const uint8_t* const* heads;
  const uint8_t* head_lens;
  const uint8_t* const* bodies;
  const uint64_t* body_lens;
  const uint8_t* priv;
  const uint8_t* pubkeys;
  int digest;
  const uint8_t* nonces;
  const uint8_t* ephem;
  const uint8_t* ivs;
  uint8_t* const* outs;
  const uint64_t* out_caps;
  bmpow_tx_rec* out;
};

// `rows`: the rows that go to the device (every scalar in [1, n - 1], every coordinate below p, the body at
// most 2^18 bytes); reordered here.
int tx_run_locked(const TxCall& c, std::vector<uint32_t>& rows) {
  std::stable_sort(rows.begin(), rows.end(), [&](uint32_t a, uint32_t b) {
    if (c.kinds[a] != c.kinds[b]) return c.kinds[a] == BMPOW_TX_SEALED;
    return c.body_lens[a] > c.body_lens[b];
  });
  const size_t total = rows.size();
  bmseal::SlotPlan p;
  p.slot.resize(total);
  for (size_t i = 0; i < total; ++i) p.slot[i] = txf::slot_bytes(c.body_lens[rows[i]]);
  if (!p.plan(kTxSetRows, kTxSetPoolBytes)) return set_err(BMPOW_E_ARG, "slot plan refused");
  const std::vector<uint64_t>& off = p.off;
  const std::vector<size_t>& begin = p.sets.begin;
  // the largest set's sealed rows and hash blocks, beside the planner's rows and slot pool
  const size_t max_rows = p.sets.max_rows;
  const uint64_t max_pool = p.sets.max_pool;
  size_t max_sealed = 0;
  uint64_t max_blocks = 1;
  for (size_t k = 0; k < p.sets.count(); ++k) {
    size_t sealed = 0;
    uint64_t blocks = 0;
    for (size_t i = begin[k]; i < begin[k + 1]; ++i) {
      const uint32_t row = rows[i];
      sealed += c.kinds[row] == BMPOW_TX_SEALED;
      blocks += txf::signed_blocks((uint32_t)(c.head_lens[row] + c.body_lens[row]));
    }
    max_sealed = std::max(max_sealed, sealed);
    max_blocks = std::max(max_blocks, blocks);
  }
  if (max_blocks > 0xffffffffull / 4) return set_err(BMPOW_E_ARG, "signed data above 2^30 blocks");

  Shard& sh = g_shards[0];
  HIPTRY(hipSetDevice(sh.dev));
  const ec::ge* comb = nullptr;
  if (const int rc = addr_comb16_table(sh, &comb); rc < 0) return rc;
  TxBufs b;
  KeySet ks;  // the sealed rows (a set's first ns): ephemeral keys and recipient points
  for (Event& e : b.ev) HIPTRY(e.alloc(sh.dev));
  const uint32_t cap = round_up((uint32_t)max_rows, TX_BLOCK), cap_s = round_up((uint32_t)max_sealed, TX_BLOCK);
  // every buffer sized once for the largest set
  HIPTRY(b.rows.alloc(sh.dev, cap));
  HIPTRY(b.sl.alloc(sh.dev, cap));
  HIPTRY(b.pool.alloc(sh.dev, max_pool));
  HIPTRY(b.hpool.alloc(sh.dev, 4 * max_blocks));
  HIPTRY(b.sigs.alloc(sh.dev, cap));
  HIPTRY(b.kw.alloc(sh.dev, cap));
  HIPTRY(b.d.alloc(sh.dev, cap));
  HIPTRY(b.e.alloc(sh.dev, (size_t)2 * cap));
  HIPTRY(b.rs.alloc(sh.dev, (size_t)2 * cap));
  HIPTRY(b.ok8.alloc(sh.dev, cap));
  HIPTRY(b.pt.alloc(sh.dev, cap));
  HIPTRY(b.recs.alloc(sh.dev, cap));
  if (const int rc = ks.alloc(sh.dev, cap_s); rc < 0) return rc;
  if (cap_s) {
    HIPTRY(b.blob_len.alloc(sh.dev, cap_s));
    HIPTRY(b.iv.alloc(sh.dev, cap_s));
  }
  b.host.alloc(max_pool);
  b.hkw.v.resize(max_rows);
  b.hd.v.resize(max_rows);
  b.hrows.resize(max_rows);
  b.hiv.resize(16 * max_sealed);
  b.hrecs.resize(max_rows);
  uint8_t* hp = b.host.get();
  g_tx_stats.calls++;

  for (size_t k = 0; k < p.sets.count(); ++k) {
    if (g_abort.load()) return set_err(BMPOW_E_ABORTED, "aborted");
    const size_t i0 = begin[k];
    const uint32_t n = (uint32_t)(begin[k + 1] - i0), stride = round_up(n, TX_BLOCK);
    const uint64_t pool_bytes = p.pool_bytes(k);
    uint32_t ns = 0, blk = 0;
    for (uint32_t j = 0; j < n; ++j) {
      const uint32_t row = rows[i0 + j];
      tx_row& r = b.hrows[j];
      r = tx_row{};
      r.off16 = (uint32_t)(off[i0 + j] / 16);
      r.body_len = (uint32_t)c.body_lens[row];
      r.blk = blk;
      r.head_len = c.head_lens[row];
      r.kind = c.kinds[row];
      r.digest = (uint8_t)c.digest;
      std::memcpy(r.head, c.heads[row], r.head_len);
      blk += txf::signed_blocks(r.head_len + r.body_len);
      ns += r.kind == BMPOW_TX_SEALED;  // a prefix of the set: the order puts the sealed rows first
    }
    const uint32_t stride_s = round_up(ns, TX_BLOCK);
    bmsched::parallel_for(n, 1024, [&](size_t a, size_t z) {
      for (size_t j = a; j < z; ++j) {
        const size_t row = rows[i0 + j];
        if (c.body_lens[row]) std::memcpy(hp + off[i0 + j] + txf::body_at(), c.bodies[row], c.body_lens[row]);
        b.hkw.v[j] = kw_from_be(c.nonces + 32 * row);
        b.hd.v[j] = sc_from_be(c.priv + 32 * row);
        if (j < ns) {
          ks.stage(j, c.ephem + 32 * row, c.pubkeys + 64 * row);
          std::memcpy(b.hiv.data() + 16 * j, c.ivs + 16 * row, 16);
        }
      }
    });
    HIPTRY(hipMemcpyAsync(b.pool.get(), hp, pool_bytes, hipMemcpyHostToDevice, sh.stream));
    HIPTRY(hipMemcpyAsync(b.rows.get(), b.hrows.data(), n * sizeof(tx_row), hipMemcpyHostToDevice, sh.stream));
    HIPTRY(hipMemcpyAsync(b.kw.get(), b.hkw.v.data(), n * sizeof(sg_kw), hipMemcpyHostToDevice, sh.stream));
    HIPTRY(hipMemcpyAsync(b.d.get(), b.hd.v.data(), n * sizeof(sc), hipMemcpyHostToDevice, sh.stream));
    if (ns) {
      if (const int rc = ks.upload(sh.stream, ns); rc < 0) return rc;
      HIPTRY(hipMemcpyAsync(b.iv.get(), b.hiv.data(), (size_t)16 * ns, hipMemcpyHostToDevice, sh.stream));
    }
    // the selected digest's plane of e: SHA-1 first, SHA-256 behind it
    const sc* e_dev = b.e.get() + (c.digest == BMPOW_SIG_SHA256 ? stride : 0);
    HIPTRY(hipEventRecord(b.ev[0].get(), sh.stream));
    HIPTRY(tx_launch_pack(sh.stream, b.rows.get(), b.pool.get(), pool_bytes, n, b.hpool.get(), 4ull * blk, b.sigs.get()));
    HIPTRY(hipEventRecord(b.ev[1].get(), sh.stream));
    HIPTRY(sg_launch_hash(sh.stream, b.sigs.get(), b.hpool.get(), n, stride, b.e.get()));
    HIPTRY(hipEventRecord(b.ev[2].get(), sh.stream));
    HIPTRY(sd_launch_comb(sh.stream, comb, b.kw.get(), n, stride, b.pt.get()));
    HIPTRY(sd_launch_sign(sh.stream, b.pt.get(), b.kw.get(), b.d.get(), e_dev, n, stride, b.rs.get(), b.ok8.get()));
    HIPTRY(tx_launch_tail(sh.stream, b.rows.get(), b.rs.get(), b.ok8.get(), n, stride, b.pool.get(), pool_bytes, b.sl.get(),
                          b.recs.get()));
    HIPTRY(hipEventRecord(b.ev[3].get(), sh.stream));
    uint64_t launches = 6;
    if (ns) {
      if (g_abort.load()) {
        HIPTRY(hipStreamSynchronize(sh.stream));
        return set_err(BMPOW_E_ABORTED, "aborted");
      }
      if (const int rc = ks.launch_ephemeral(sh.stream, comb, ns, stride_s); rc < 0) return rc;
      if (const int rc = ks.launch_shared(sh.stream, ns, stride_s); rc < 0) return rc;
      launches += 5;
    }
    HIPTRY(hipEventRecord(b.ev[4].get(), sh.stream));
    if (ns)
      HIPTRY(sl_launch_seal(sh.stream, ks.kout.get(), ks.pt.get(), ks.ok32.get(), b.iv.get(), b.sl.get(), b.pool.get(), ns,
                            stride_s, b.blob_len.get()));
    HIPTRY(hipEventRecord(b.ev[5].get(), sh.stream));
    HIPTRY(tx_launch_finish(sh.stream, b.rows.get(), b.blob_len.get(), ns, b.pool.get(), pool_bytes, n, b.recs.get()));
    HIPTRY(hipEventRecord(b.ev[6].get(), sh.stream));
    HIPTRY(hipMemcpyAsync(hp, b.pool.get(), pool_bytes, hipMemcpyDeviceToHost, sh.stream));
    HIPTRY(hipMemcpyAsync(b.hrecs.data(), b.recs.get(), n * sizeof(bmpow_tx_rec), hipMemcpyDeviceToHost, sh.stream));
    HIPTRY(hipStreamSynchronize(sh.stream));
    double* const acc[6] = {&g_tx_stats.pack_ms, &g_tx_stats.hash_ms, &g_tx_stats.sign_ms,
                            &g_tx_stats.ladder_ms, &g_tx_stats.seal_ms, &g_tx_stats.finish_ms};
    if (const int rc = elapsed_phases(acc, b.ev, 6); rc < 0) return rc;
    std::atomic<bool> bad{false};
    bmsched::parallel_for(n, 1024, [&](size_t a, size_t z) {
      for (size_t j = a; j < z; ++j) {
        const size_t row = rows[i0 + j];
        const bmpow_tx_rec& r = b.hrecs[j];
        c.out[row] = r;
        if (r.status != BMPOW_TX_OK) continue;
        const uint32_t hl = c.head_lens[row];
        if (r.obj_len < hl || r.obj_len > c.out_caps[row]) {  // never: the kernel's lengths follow the host's
          bad.store(true);
          continue;
        }
        std::memcpy(c.outs[row], c.heads[row], hl);
        const uint8_t* src = hp + off[i0 + j] + (r.kind == BMPOW_TX_SEALED ? 0u : txf::body_at());
        std::memcpy(c.outs[row] + hl, src, r.obj_len - hl);
      }
    });
    if (bad.load()) return set_err(BMPOW_E_HIP, "the finish kernel returned a length above the payload's bound");
    g_tx_stats.rows += n;
    g_tx_stats.sets++;
    g_tx_stats.launches += launches;
  }
  return 0;
}

int tx_run(const TxCall& c, std::vector<uint32_t>& rows) {
  if (rows.empty()) return 0;
  int rc = init_locked();
  if (rc >= 0) rc = tx_run_locked(c, rows);
  return rc > 0 ? 0 : rc;
}

}  // namespace
}  // namespace bmhost

using namespace bmhost;

extern "C" {

int bmpow_tx_objects(size_t n, const uint8_t* kinds, const uint8_t* const* heads, const uint8_t* head_lens,
                     const uint8_t* const* bodies, const uint64_t* body_lens, const uint8_t* privkeys,
                     const uint8_t* pubkeys, int digest, const uint8_t* nonces, const uint8_t* ephem, const uint8_t* ivs,
                     uint8_t* const* outs, const uint64_t* out_caps, bmpow_tx_rec* out) {
  std::lock_guard<FairMutex> lk(g_mu);
  if (n == 0) return 0;
  if (!kinds || !heads || !head_lens || !bodies || !body_lens || !privkeys || !outs || !out_caps || !out)
    return set_err(BMPOW_E_ARG, "null pointer");
  if (n > 0xffffffffull) return set_err(BMPOW_E_ARG, "too many objects");
  if (digest != BMPOW_SIG_SHA1 && digest != BMPOW_SIG_SHA256) return set_err(BMPOW_E_ARG, "digest is neither SHA-1 nor SHA-256");
  WallClock clock{g_tx_stats.host_ms};
  size_t sealed = 0;
  for (size_t i = 0; i < n; ++i) {
    if (kinds[i] != BMPOW_TX_SEALED && kinds[i] != BMPOW_TX_CLEAR) return set_err(BMPOW_E_ARG, "unknown kind");
    if (head_lens[i] < BMPOW_TX_HEAD_MIN || head_lens[i] > BMPOW_TX_HEAD_MAX)
      return set_err(BMPOW_E_ARG, "a head is 12 to 62 bytes");
    if (!heads[i] || (body_lens[i] && !bodies[i])) return set_err(BMPOW_E_ARG, "null head or body pointer");
    if (!scalar_in_range(privkeys + 32 * i)) return set_err(BMPOW_E_ARG, "private key is zero or not below the group order");
    if (nonces && !scalar_in_range(nonces + 32 * i)) return set_err(BMPOW_E_ARG, "nonce is zero or not below the group order");
    if (kinds[i] == BMPOW_TX_SEALED) {
      ++sealed;
      if (!pubkeys) return set_err(BMPOW_E_ARG, "null pointer: a sealed row needs its recipient key");
      if (ephem && !scalar_in_range(ephem + 32 * i))
        return set_err(BMPOW_E_ARG, "ephemeral key is zero or not below the group order");
    }
    if (body_lens[i] > txf::kMaxBody) continue;
    if (!outs[i]) return set_err(BMPOW_E_ARG, "null output pointer");
    if (out_caps[i] < BMPOW_TX_OBJ_CAP(head_lens[i], body_lens[i])) return set_err(BMPOW_E_ARG, "output buffer below BMPOW_TX_OBJ_CAP");
  }
  Wiped<uint8_t> k_drawn, e_drawn;
  std::vector<uint8_t> iv_drawn;
  if (!nonces) {
    k_drawn.v.resize(32 * n);
    if (!draw_scalars(k_drawn.v.data(), n)) return set_err(BMPOW_E_ARG, "RAND_bytes failed");
  }
  if (sealed && !ephem) {
    e_drawn.v.resize(32 * n);
    if (!draw_scalars(e_drawn.v.data(), n)) return set_err(BMPOW_E_ARG, "RAND_bytes failed");
  }
  if (sealed && !ivs) {
    iv_drawn.resize(16 * n);
    if (!draw_bytes(iv_drawn.data(), iv_drawn.size())) return set_err(BMPOW_E_ARG, "RAND_bytes failed");
  }
  TxCall c;
  c.kinds = kinds, c.heads = heads, c.head_lens = head_lens, c.bodies = bodies, c.body_lens = body_lens;
  c.priv = privkeys, c.pubkeys = pubkeys, c.digest = digest;
  c.nonces = nonces ? nonces : k_drawn.v.data();
  c.ephem = ephem ? ephem : e_drawn.v.data();
  c.ivs = ivs ? ivs : iv_drawn.data();
  c.outs = outs, c.out_caps = out_caps, c.out = out;
  // what decides before a device: a body no object can hold, a recipient coordinate that is no field element
  std::vector<uint32_t> rows;
  rows.reserve(n);
  for (size_t i = 0; i < n; ++i) {
    bmpow_tx_rec& r = out[i];
    std::memset(&r, 0, sizeof r);
    r.kind = kinds[i];
    r.digest = (uint8_t)digest;
    if (body_lens[i] > txf::kMaxBody) r.status = BMPOW_TX_TOO_LARGE;
    else if (kinds[i] == BMPOW_TX_SEALED &&
             !(coord_in_range(sc_from_be(pubkeys + 64 * i)) && coord_in_range(sc_from_be(pubkeys + 64 * i + 32))))
      r.status = BMPOW_TX_BAD_RECIPIENT;
    else rows.push_back((uint32_t)i);
  }
  // r == 0 or s == 0: another nonce, the whole chain again
  return sign_passes(
      rows, nonces ? nullptr : k_drawn.v.data(), [&](std::vector<uint32_t>& r) { return tx_run(c, r); },
      [&](uint32_t row) { return out[row].status == BMPOW_TX_NO_SIGNATURE; });
}

int bmpow_tx_layout_row(uint32_t head_len, uint64_t body_len, bmpow_tx_layout* out) {
  if (!out) return set_err(BMPOW_E_ARG, "null pointer");
  if (head_len < txf::kHeadMin || head_len > txf::kHeadMax) return set_err(BMPOW_E_ARG, "a head is 12 to 62 bytes");
  if (body_len > txf::kMaxBody) return set_err(BMPOW_E_ARG, "body above 2^18 bytes");
  const uint32_t bl = (uint32_t)body_len;
  *out = bmpow_tx_layout{};
  out->slot_bytes = txf::slot_bytes(body_len);
  out->body_at = txf::body_at();
  out->tail_at = txf::tail_at(bl);
  out->plain_cap = bl + txf::kTailMax;
  out->signed_len = head_len + bl;
  out->hash_blocks = txf::signed_blocks(head_len + bl);
  return 0;
}

int bmpow_tx_get_stats(bmpow_tx_stats* out) {
  std::lock_guard<FairMutex> lk(g_mu);
  if (!out) return set_err(BMPOW_E_ARG, "null pointer");
  *out = g_tx_stats;
  return 0;
}

void bmpow_tx_reset_stats(void) {
  std::lock_guard<FairMutex> lk(g_mu);
  g_tx_stats = bmpow_tx_stats{};
}

}  // extern "C"
