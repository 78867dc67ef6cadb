// bmpow_host_rxopen.hip -- the one-call opening of received msgs: the bmpow_rx_sealed_* entry points
// (include/bmpow_rxopen.h) over the ECIES set of bmpow_host_ecies.hip, the opening kernel of bmpow_rxopen.hip
// and the msg family's set of the rows pipeline (bmpow_host_rx.h, bmpow_host_rows.h).
#include "bmpow_host_ecies.h"
#include "bmpow_host_rx.h"

#include "../../include/bmpow_rxopen.h"
#include "bmpow_rx_fmt.h"
#include "bmpow_rxopen_kernels.h"

// ---------------------------------------------------------------------------------------
// One call.  The host walks every object's head (rxf::walk with an empty plaintext); the payloads behind the
// heads that pass go through ecies_parse and, sorted by MAC block count, through the device in the ECIES sets
// of bmpow_ecies_match: per set ecies_match_set uploads the padded MAC pool once and runs the preparation,
// ladder, MAC and gather launches for every key group.  match[] of the set comes down (4 bytes per row); for
// the rows it names whose ciphertext is a positive multiple of 16 bytes the host builds compacted rx_rows
// and rxs_rows (96 bytes per matched row) and uploads only those.  rxs_open_kernel then decrypts each from the
// MAC pool into the plaintext pool and writes the row's plen, and the nine launches of launch_set
// (bmpow_host_rows.h) read that pool where it lies.  Down come the matched rows' records, opened[] and the plaintext pool, in one copy each.
// A set without a matched row launches none of the ten.  The abort flag is read between sets and (by
// ecies_match_set) between key groups.  The buffers are the call's own (DevBuf owners).
// ---------------------------------------------------------------------------------------
namespace bmhost {
namespace {

bmpow_rx_sealed_stats g_sealed_stats{};  // under g_mu

// The head of one object: rec as bmpow_rx_walk_msg leaves it for an empty plaintext where the head refuses
// (false); else (true) the record of a row no key opens -- claimed_stream and prefix_len from the head, status
// BMPOW_RX_NOT_MINE -- and where the payload starts.
bool walk_head(const uint8_t* obj, uint64_t len, bmpow_rx_msg_rec& rec, size_t& payload_off) {
  static const uint8_t no_ripe[20] = {};
  const uint32_t hlen = (uint32_t)std::min<uint64_t>(len, rxf::kHeadBytes);
  std::memset(&rec, 0, sizeof rec);
  uint32_t key_off = 0;
  rxf::walk(obj, hlen, nullptr, 0, no_ripe, rec, key_off);
  if (rec.status == BMPOW_RX_MSG_VERSION) return false;
  const rxf::varint mv = rxf::get_varint(obj, hlen, 20);
  const rxf::varint claimed = rxf::get_varint(obj, hlen, 20 + mv.n);
  payload_off = 20 + mv.n + claimed.n;
  const uint8_t prefix_len = rec.prefix_len;
  std::memset(&rec, 0, sizeof rec);
  rec.claimed_stream = claimed.v;
  rec.prefix_len = prefix_len;
  rec.status = BMPOW_RX_NOT_MINE;
  return true;
}

struct SealedBufs {
  DevBuf<rxs_row> orows;
  DevBuf<int32_t> opened;
  Event ev[2];
};

int sealed_run_locked(const std::vector<Item>& items, const uint8_t* const* payloads, const uint64_t* pay_lens,
                      const uint32_t* pay_orig, const uint8_t* const* objs, const uint64_t* obj_lens,
                      const std::vector<int32_t>& dig, size_t n_keys, const uint8_t* ripes, bmpow_rx_msg_rec* recs,
                      int32_t* match, uint8_t* arena, const uint64_t* slot_off, uint64_t* plain_off, uint64_t* plain_len) {
  bmpow_rx_sealed_stats& st = g_sealed_stats;
  Shard& sh = g_shards[0];
  HIPTRY(hipSetDevice(sh.dev));
  EciesBufs b;
  if (const int rc = ecies_events(b, sh.dev); rc < 0) return rc;
  HIPTRY(b.dig.alloc(sh.dev, dig.size()));
  HIPTRY(hipMemcpyAsync(b.dig.get(), dig.data(), dig.size() * sizeof(int32_t), hipMemcpyHostToDevice, sh.stream));
  st.calls++;
  st.bytes_up += dig.size() * sizeof(int32_t);

  const ec::ge* comb = nullptr;
  SigBufs sb;
  RxBufs x;
  SealedBufs o;
  EciesStage h;
  std::vector<rx_row> rows;
  std::vector<rxs_row> orows;
  std::vector<uint32_t> who;  // the input index of each matched row
  std::vector<bmpow_rx_msg_rec> drecs;
  std::vector<int32_t> opened;
  std::vector<uint8_t> plain;
  size_t i0 = 0;
  while (i0 < items.size()) {
    if (g_abort.load()) return set_err(BMPOW_E_ABORTED, "aborted");
    uint64_t blocks = 0;
    const size_t i1 = ecies_set_end(items, i0, blocks);
    const uint32_t n = (uint32_t)(i1 - i0);
    bmpow_ecies_stats es{};
    const int rc_set = ecies_match_set(sh, b, h, items.data() + i0, n, blocks, payloads, pay_lens, n_keys, true, es);
    st.match_ms += es.prep_ms + es.ecdh_ms + es.mac_ms;
    st.launches += 1 + 3 * es.launches;
    if (rc_set < 0) return rc_set;
    HIPTRY(hipStreamSynchronize(sh.stream));
    st.sets++;
    st.bytes_up += n * (sizeof(ec::ge) + sizeof(ec_obj)) + h.pool.size();
    st.bytes_down += n * sizeof(int);

    rows.clear(), orows.clear(), who.clear();
    uint64_t poff = 0, blk = 0;
    for (uint32_t j = 0; j < n; ++j) {
      const int m = h.match[j];
      if (m < 0 || (size_t)m >= n_keys) continue;
      const Item& it = items[i0 + j];
      const uint32_t orig = pay_orig[it.orig];
      match[orig] = m;
      const uint64_t clen = pay_lens[it.orig] - 32 - it.hdr.body_off;
      if (clen == 0 || clen % 16) continue;  // the reference's decrypt raises: the loop goes on, to :478
      rx_row r{};
      r.poff = poff;
      r.blk = (uint32_t)blk;
      r.hlen = (uint8_t)std::min<uint64_t>(obj_lens[orig], rxf::kHeadBytes);
      std::memcpy(r.head, objs[orig], r.hlen);
      std::memcpy(r.to_ripe, ripes + 20 * (size_t)m, 20);
      rows.push_back(r);
      orows.push_back(rxs_row{j, h.objs[j].blk, (uint32_t)it.hdr.body_off, (uint32_t)clen});
      who.push_back(orig);
      poff += clen;
      blk += rxf::signed_blocks_bound(clen - 1);  // the plaintext is at least one byte shorter
    }
    const uint32_t nm = (uint32_t)rows.size();
    if (nm) {
      // no more blocks than the MAC pool's: (22 + clen - 1 + 72) / 64 <= (body_off + clen + 72) / 64
      if (blk > 0xffffffffull) return set_err(BMPOW_E_ARG, "message pool above 2^32 blocks");
      if (!comb)
        if (const int rc = addr_comb16_table(sh, &comb); rc < 0) return rc;
      for (Event& e : x.ev)
        if (!e) HIPTRY(e.alloc(sh.dev));
      for (Event& e : o.ev)
        if (!e) HIPTRY(e.alloc(sh.dev));
      const uint32_t stride = (nm + SG_BLOCK - 1) / SG_BLOCK * SG_BLOCK;
      const uint64_t plain_bytes = std::max<uint64_t>(poff, 16), plain_chunks = plain_bytes / 16;
      const uint64_t pool_chunks = std::max<uint64_t>(blk * 4, 4);
      if (const int rc = grow_set(sh, sb, x, stride, pool_chunks, plain_chunks); rc < 0) return rc;
      HIPTRY(o.orows.grow(sh.dev, stride));
      HIPTRY(o.opened.grow(sh.dev, stride));
      HIPTRY(hipMemcpyAsync(x.rows.get(), rows.data(), nm * sizeof(rx_row), hipMemcpyHostToDevice, sh.stream));
      HIPTRY(hipMemcpyAsync(o.orows.get(), orows.data(), nm * sizeof(rxs_row), hipMemcpyHostToDevice, sh.stream));
      HIPTRY(hipEventRecord(o.ev[0].get(), sh.stream));
      HIPTRY(rxs_launch_open(sh.stream, o.orows.get(), b.key_e.get(), n, reinterpret_cast<const uint8_t*>(b.pool.get()),
                             h.pool.size(), x.rows.get(), reinterpret_cast<uint8_t*>(x.plain.get()), plain_bytes, nm,
                             o.opened.get()));
      HIPTRY(hipEventRecord(o.ev[1].get(), sh.stream));
      if (const int rc = launch_set(sh, sb, x, comb, nm, stride, plain_chunks, pool_chunks); rc < 0) return rc;
      drecs.resize(nm);
      opened.resize(nm);
      plain.resize(poff);
      HIPTRY(hipMemcpyAsync(drecs.data(), x.recs.get(), nm * sizeof(bmpow_rx_msg_rec), hipMemcpyDeviceToHost, sh.stream));
      HIPTRY(hipMemcpyAsync(opened.data(), o.opened.get(), nm * sizeof(int32_t), hipMemcpyDeviceToHost, sh.stream));
      HIPTRY(hipMemcpyAsync(plain.data(), x.plain.get(), poff, hipMemcpyDeviceToHost, sh.stream));
      HIPTRY(hipStreamSynchronize(sh.stream));
      if (const int rc = elapsed(st.open_ms, o.ev[0], o.ev[1]); rc < 0) return rc;
      bmpow_rx_stats rs{};
      if (const int rc = phase_times(x, rs); rc < 0) return rc;
      st.walk_ms += rs.walk_ms, st.hash_ms += rs.hash_ms, st.scalar_ms += rs.scalar_ms;
      st.curve_ms += rs.curve_ms, st.ident_ms += rs.ident_ms, st.finish_ms += rs.finish_ms;
      st.matched += nm;
      st.launches += 10;
      st.rx_launches += 10;
      st.bytes_up += (uint64_t)nm * (sizeof(rx_row) + sizeof(rxs_row));
      st.bytes_down += (uint64_t)nm * (sizeof(bmpow_rx_msg_rec) + sizeof(int32_t)) + poff;
      bmsched::parallel_for(nm, 1024, [&](size_t a, size_t z) {
        for (size_t k = a; k < z; ++k) {
          if (opened[k] < 0) continue;  // bad padding: BMPOW_RX_NOT_MINE stands, match[] names the key
          const uint32_t orig = who[k];
          recs[orig] = drecs[k];
          plain_off[orig] = slot_off[orig];
          plain_len[orig] = (uint64_t)opened[k];
          if (opened[k]) std::memcpy(arena + slot_off[orig], plain.data() + rows[k].poff, (size_t)opened[k]);
        }
      });
    }
    i0 = i1;
  }
  return 0;
}

}  // namespace
}  // namespace bmhost

using namespace bmhost;

extern "C" {

int bmpow_rx_sealed_msgs(size_t n, const uint8_t* const* objs, const uint64_t* obj_lens, size_t n_keys,
                         const uint8_t* privkeys32, const uint8_t* ripes20, bmpow_rx_msg_rec* recs, int32_t* match,
                         uint8_t* arena, uint64_t arena_cap, uint64_t* plain_off, uint64_t* plain_len) {
  std::lock_guard<FairMutex> lk(g_mu);
  if (n == 0) return 0;
  if (!objs || !obj_lens || !recs || !match || !plain_off || !plain_len) return set_err(BMPOW_E_ARG, "null pointer");
  if (n_keys && (!privkeys32 || !ripes20)) return set_err(BMPOW_E_ARG, "null pointer");
  if (n > 0xffffffffull || n_keys > 0x7fffffffull) return set_err(BMPOW_E_ARG, "too many objects or keys");
  const auto t_begin = std::chrono::steady_clock::now();
  // an object's plaintext goes to the arena where the objects in front of it end: a plaintext is shorter than
  // its object, so the sum of the objects' lengths holds them all, whatever the outcome
  std::vector<uint64_t> slot_off(n);
  uint64_t total = 0;
  for (size_t i = 0; i < n; ++i) {
    if (obj_lens[i] && !objs[i]) return set_err(BMPOW_E_ARG, "null object pointer");
    slot_off[i] = total;
    if (total + obj_lens[i] < total) return set_err(BMPOW_E_ARG, "objects above 2^64 bytes");
    total += obj_lens[i];
  }
  if (arena_cap < total) return set_err(BMPOW_E_ARG, "arena smaller than the objects together");
  if (total && !arena) return set_err(BMPOW_E_ARG, "null pointer");
  std::vector<int32_t> dig(n_keys * EC_DIGITS);
  for (size_t k = 0; k < n_keys; ++k) {
    const U256 key = u256_from_be(privkeys32 + 32 * k);
    if (!key_in_range(key)) return set_err(BMPOW_E_ARG, "private key is zero or not below the group order");
    recode_key(key, dig.data() + k * EC_DIGITS);
  }
  std::vector<const uint8_t*> payloads;
  std::vector<uint64_t> pay_lens;
  std::vector<uint32_t> pay_orig;
  std::vector<Item> items;
  for (size_t i = 0; i < n; ++i) {
    match[i] = -1;
    plain_off[i] = plain_len[i] = 0;
    size_t payload_off = 0;
    if (!walk_head(objs[i], obj_lens[i], recs[i], payload_off)) continue;
    if (n_keys == 0) continue;
    Item it;
    const uint8_t* p = objs[i] + payload_off;  // payload_off <= the object's length: both varints lie inside it
    const uint64_t len = obj_lens[i] - payload_off;
    if (!ecies_parse(p, len, it.hdr)) continue;
    if (len - 32 > (1ull << 31)) return set_err(BMPOW_E_ARG, "payload above 2^31 bytes");
    it.orig = (uint32_t)payloads.size();
    it.nblk = mac_blocks(len - 32);
    items.push_back(it);
    payloads.push_back(p);
    pay_lens.push_back(len);
    pay_orig.push_back((uint32_t)i);
  }
  std::stable_sort(items.begin(), items.end(), [](const Item& a, const Item& b) { return a.nblk > b.nblk; });
  int rc = 0;
  if (!items.empty()) {
    rc = init_locked();
    if (rc >= 0)
      rc = sealed_run_locked(items, payloads.data(), pay_lens.data(), pay_orig.data(), objs, obj_lens, dig, n_keys,
                             ripes20, recs, match, arena, slot_off.data(), plain_off, plain_len);
    if (rc > 0) rc = 0;
  }
  g_sealed_stats.rows += n;
  g_sealed_stats.host_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
  return rc;
}

int bmpow_rx_sealed_plan(const uint8_t* obj, size_t len, size_t* payload_off, size_t* body_off, size_t* clen,
                         int* reason) {
  if ((len && !obj) || !payload_off || !body_off || !clen || !reason) return set_err(BMPOW_E_ARG, "null pointer");
  *payload_off = *body_off = *clen = 0;
  bmpow_rx_msg_rec rec;
  size_t off = 0;
  if (!walk_head(obj, len, rec, off)) {
    *reason = BMPOW_RXS_PLAN_HEAD;
    return 0;
  }
  *payload_off = off;
  Parsed p;
  if (!ecies_parse(obj + off, len - off, p)) {
    *reason = BMPOW_RXS_PLAN_PAYLOAD;
    return 0;
  }
  *body_off = p.body_off;
  *clen = len - off - 32 - p.body_off;
  if (*clen == 0 || *clen % 16) {
    *reason = BMPOW_RXS_PLAN_CIPHER;
    return 0;
  }
  *reason = BMPOW_RXS_PLAN_OK;
  return 1;
}

int bmpow_rx_sealed_get_stats(bmpow_rx_sealed_stats* out) {
  std::lock_guard<FairMutex> lk(g_mu);
  if (!out) return set_err(BMPOW_E_ARG, "null pointer");
  *out = g_sealed_stats;
  return 0;
}

void bmpow_rx_sealed_reset_stats(void) {
  std::lock_guard<FairMutex> lk(g_mu);
  g_sealed_stats = bmpow_rx_sealed_stats{};
}

}  // extern "C"
