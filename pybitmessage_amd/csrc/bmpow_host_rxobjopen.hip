// bmpow_host_rxobjopen.hip -- the one-call opening of received broadcasts and pubkeys: the bmpow_rx_sealed_obj*
// entry points (include/bmpow_rxobjopen.h) over the ECIES set of bmpow_host_ecies.hip, the per-row-key ladder of
// bmpow_ecies.hip, the opening kernel of bmpow_rxopen.hip and the object family's set of the rows pipeline
// (bmpow_host_rxobj.h, bmpow_host_rows.h).
#include "bmpow_host_ecies.h"
#include "bmpow_host_rxobj.h"

#include "../../include/bmpow_rxobjopen.h"
#include "bmpow_rxobjopen_tab.h"
#include "bmpow_rxopen_kernels.h"

// ---------------------------------------------------------------------------------------
// One call.  The host walks every object's head once (route_object, the rxf walk code the kernels are built
// from), looks the tags up in two hash tables built for the call, and settles every status that needs no key.
// What is left are three classes of rows: v4 broadcasts (every trial key), and v5 broadcasts and v4 pubkeys (the
// one key their table entry names).  Their payloads go through ecies_parse and, sorted by MAC block count,
// through the device in the ECIES sets of bmpow_ecies_match; within a set the trial rows come first.  Per set
// ecies_stage_set uploads the padded MAC pool once and prepares every row's table; ecies_try_keys runs the trial
// key groups over the trial rows; one ec_launch_rowkeys launch derives each tagged row's key from the digits of
// its own entry, and the MAC and gather launches follow over those rows with one key each.  match[] of the set
// comes down (4 bytes per row); for the rows it names whose ciphertext is a positive multiple of 16 bytes the host
// builds compacted rxo_rows and rxs_rows and uploads only those.  rxo_open_kernel decrypts each from the MAC pool
// into the plaintext pool and writes the row's plen, and the nine launches of launch_set read that pool where it
// lies.  Down come the matched rows' records, opened[] and the plaintext pool, in one copy each.  A set without a
// matched row launches none of the ten.  Clear pubkeys the walk accepts are rows of run_rows, uploaded as
// bmpow_rx_objects uploads them.  The abort flag is read between sets and between key groups.  The buffers are
// the call's own (DevBuf owners).
// ---------------------------------------------------------------------------------------
namespace bmhost {
namespace {

bmpow_rx_sealed_obj_stats g_sealed_obj_stats{};  // under g_mu

struct Sealed {  // one row that is tried, by the index of its payload (Item::orig)
  uint32_t orig;   // the input index
  uint8_t cls;     // ROUTE_TRIAL, ROUTE_TAG or ROUTE_NEEDED
  int32_t entry;   // the index into the row's own table (ROUTE_TAG, ROUTE_NEEDED)
};

struct Call {
  const uint8_t* const* objs;
  const uint64_t* obj_lens;
  const bmpow_rx_obj_tables* t;
  bmpow_rx_obj_rec* recs;
  int32_t* match;
  uint8_t* arena;
  const uint64_t* slot_off;
  uint64_t* plain_off;
  uint64_t* plain_len;
};

struct ClearPolicy {  // the clear pubkeys of a call as rows of run_rows
  const std::vector<uint32_t>& who;
  const uint8_t* const* objs;
  const uint64_t* obj_lens;
  bmpow_rx_obj_stats& stats;
  uint32_t bound(size_t i) const { return rxf::signed_blocks_bound_obj(len(i)); }
  const uint8_t* source(size_t i) const { return objs[who[i]]; }
  uint64_t len(size_t i) const { return obj_lens[who[i]]; }
  void fill(rxo_row& r, size_t i) const {
    r.kind = BMPOW_RXO_KIND_PUBKEY;
    r.hlen = (uint8_t)std::min<uint64_t>(len(i), rxf::kObjHeadBytes);
    if (r.hlen) std::memcpy(r.head, source(i), r.hlen);
  }
};

int clear_run_locked(const std::vector<uint32_t>& clear, const Call& c) {
  bmpow_rx_sealed_obj_stats& st = g_sealed_obj_stats;
  bmpow_rx_obj_stats rs{};
  std::vector<bmpow_rx_obj_rec> out(clear.size());
  if (const int rc = run_rows<RxoFamily>(clear.size(), ClearPolicy{clear, c.objs, c.obj_lens, rs}, out.data()); rc < 0)
    return rc;
  for (size_t k = 0; k < clear.size(); ++k) {
    c.recs[clear[k]] = out[k];
    st.bytes_up += ((c.obj_lens[clear[k]] + 15) & ~15ull) + sizeof(rxo_row);
  }
  st.bytes_down += clear.size() * sizeof(bmpow_rx_obj_rec);
  st.clear += clear.size();
  st.launches += rs.launches, st.rx_launches += rs.launches;
  st.walk_ms += rs.walk_ms, st.hash_ms += rs.hash_ms, st.scalar_ms += rs.scalar_ms;
  st.curve_ms += rs.curve_ms, st.ident_ms += rs.ident_ms, st.finish_ms += rs.finish_ms;
  return 0;
}

struct OpenBufs {
  DevBuf<rxs_row> orows;
  DevBuf<int32_t> opened, kidx;
  Event ev[2];
};

// items: sorted by MAC block count, descending.  dig: the digits of the trial keys, then of the tag keys, then of
// the needed entries' keys.
int sealed_run_locked(std::vector<Item>& items, const uint8_t* const* payloads, const uint64_t* pay_lens,
                      const std::vector<Sealed>& pay, const std::vector<int32_t>& dig, const Call& c) {
  bmpow_rx_sealed_obj_stats& st = g_sealed_obj_stats;
  const bmpow_rx_obj_tables& t = *c.t;
  const size_t n_trial = t.n_trial, n_tab = dig.size() / EC_DIGITS;
  Shard& sh = g_shards[0];
  HIPTRY(hipSetDevice(sh.dev));
  EciesBufs b;
  if (const int rc = ecies_events(b, sh.dev); rc < 0) return rc;
  HIPTRY(b.dig.alloc(sh.dev, dig.size()));
  HIPTRY(hipMemcpyAsync(b.dig.get(), dig.data(), dig.size() * sizeof(int32_t), hipMemcpyHostToDevice, sh.stream));
  st.bytes_up += dig.size() * sizeof(int32_t);

  const ec::ge* comb = nullptr;
  SigBufs sb;
  RxoBufs x;
  OpenBufs o;
  EciesStage h;
  std::vector<rxo_row> rows;
  std::vector<rxs_row> orows;
  std::vector<uint32_t> who;  // the input index of each matched row
  std::vector<int32_t> kidx;
  std::vector<bmpow_rx_obj_rec> drecs;
  std::vector<int32_t> opened;
  std::vector<uint8_t> plain;
  size_t i0 = 0;
  while (i0 < items.size()) {
    if (g_abort.load()) return set_err(BMPOW_E_ABORTED, "aborted");
    uint64_t blocks = 0;
    const size_t i1 = ecies_set_end(items, i0, blocks);
    const uint32_t n = (uint32_t)(i1 - i0), stride = (n + EC_BLOCK - 1) / EC_BLOCK * EC_BLOCK;
    // the trial rows first: both halves stay sorted by block count
    const uint32_t nt = (uint32_t)(std::stable_partition(items.begin() + i0, items.begin() + i1,
                                                         [&](const Item& it) { return pay[it.orig].cls == ROUTE_TRIAL; }) -
                                   (items.begin() + i0));
    const uint32_t ng = n - nt;
    bmpow_ecies_stats es{};
    int rc_set = ecies_stage_set(sh, b, h, items.data() + i0, n, blocks, payloads, pay_lens, n_trial, true, es);
    if (rc_set >= 0) rc_set = ecies_try_keys(sh, b, nt, n, n_trial, true, es);
    st.match_ms += es.prep_ms + es.ecdh_ms + es.mac_ms;
    st.launches += 1 + 3 * es.launches;
    st.trial_tries += es.pairs;
    if (rc_set < 0) return rc_set;
    if (ng) {
      if (g_abort.load()) return set_err(BMPOW_E_ABORTED, "aborted");
      kidx.resize(ng);
      for (uint32_t j = 0; j < ng; ++j) {
        const Sealed& s = pay[items[i0 + nt + j].orig];
        kidx[j] = (int32_t)(n_trial + (s.cls == ROUTE_NEEDED ? t.n_tags : 0) + (size_t)s.entry);
      }
      HIPTRY(o.kidx.grow(sh.dev, ng));
      HIPTRY(hipMemcpyAsync(o.kidx.get(), kidx.data(), ng * sizeof(int32_t), hipMemcpyHostToDevice, sh.stream));
      HIPTRY(hipEventRecord(b.ev[0].get(), sh.stream));
      HIPTRY(ec_launch_rowkeys(sh.stream, b.tab.get(), nt, ng, stride, b.dig.get(), (uint32_t)n_tab, o.kidx.get(),
                               b.kout.get(), b.ok.get()));
      HIPTRY(ec_launch_mac(sh.stream, b.kout.get() + nt, ng, stride, 1, b.objs.get() + nt, b.pool.get(), b.ok.get() + nt, 0,
                           b.match.get() + nt));
      HIPTRY(ec_launch_gather(sh.stream, b.kout.get() + nt, ng, stride, 1, 0, b.match.get() + nt,
                              b.key_e.get() + (size_t)4 * nt));
      HIPTRY(hipEventRecord(b.ev[1].get(), sh.stream));
      st.launches += 3;
      st.tagged_tries += ng;
      st.bytes_up += ng * sizeof(int32_t);
    }
    h.match.resize(n);
    HIPTRY(hipMemcpyAsync(h.match.data(), b.match.get(), n * sizeof(int), hipMemcpyDeviceToHost, sh.stream));
    HIPTRY(hipStreamSynchronize(sh.stream));
    if (ng)
      if (const int rc = elapsed(st.match_ms, b.ev[0], b.ev[1]); rc < 0) return rc;
    st.sets++;
    st.bytes_up += n * (sizeof(ec::ge) + sizeof(ec_obj)) + h.pool.size();
    st.bytes_down += n * sizeof(int);

    rows.clear(), orows.clear(), who.clear();
    uint64_t poff = 0, blk = 0;
    for (uint32_t j = 0; j < n; ++j) {
      const int m = h.match[j];
      const Item& it = items[i0 + j];
      const Sealed& s = pay[it.orig];
      const uint8_t* expect = nullptr;
      if (s.cls == ROUTE_TRIAL) {
        if (m < 0 || (size_t)m >= n_trial) continue;
        c.match[s.orig] = m;
        expect = t.trial_ripe20 + 20 * (size_t)m;
      } else {
        if (m != 0) continue;
        c.match[s.orig] = s.entry;
        if (s.cls == ROUTE_NEEDED) expect = t.needed_ripe20 + 20 * (size_t)s.entry;
      }
      const uint64_t clen = pay_lens[it.orig] - 32 - it.hdr.body_off;
      if (clen == 0 || clen % 16) continue;  // the reference's decrypt raises: the status of a row no key opened stands
      rxo_row r{};
      r.poff = poff;
      r.blk = (uint32_t)blk;
      r.hlen = (uint8_t)std::min<uint64_t>(c.obj_lens[s.orig], rxf::kObjHeadBytes);
      std::memcpy(r.head, c.objs[s.orig], r.hlen);
      r.kind = c.recs[s.orig].kind;
      if (expect) std::memcpy(r.expect, expect, 20);
      rows.push_back(r);
      orows.push_back(rxs_row{j, h.objs[j].blk, (uint32_t)it.hdr.body_off, (uint32_t)clen});
      who.push_back(s.orig);
      poff += clen;
      blk += rxf::signed_blocks_bound_obj(clen - 1);  // the plaintext is at least one byte shorter
      // Unlike a msg's, this bound may exceed the row's MAC blocks by one (a prefix of up to 62 bytes against a
      // head of body_off >= 22), so the signed-data pool of a set may be above its MAC pool, by at most one block
      // per matched row (16 MB for 2^18 rows); the 2^32-block check below is the guard.
    }
    const uint32_t nm = (uint32_t)rows.size();
    if (nm) {
      if (blk > 0xffffffffull) return set_err(BMPOW_E_ARG, "message pool above 2^32 blocks");
      if (!comb)
        if (const int rc = addr_comb16_table(sh, &comb); rc < 0) return rc;
      for (Event& e : x.ev)
        if (!e) HIPTRY(e.alloc(sh.dev));
      for (Event& e : o.ev)
        if (!e) HIPTRY(e.alloc(sh.dev));
      const uint32_t rstride = (nm + SG_BLOCK - 1) / SG_BLOCK * SG_BLOCK;
      const uint64_t plain_bytes = std::max<uint64_t>(poff, 16), plain_chunks = plain_bytes / 16;
      const uint64_t pool_chunks = std::max<uint64_t>(blk * 4, 4);
      if (const int rc = grow_set(sh, sb, x, rstride, pool_chunks, plain_chunks); rc < 0) return rc;
      HIPTRY(o.orows.grow(sh.dev, rstride));
      HIPTRY(o.opened.grow(sh.dev, rstride));
      HIPTRY(hipMemcpyAsync(x.rows.get(), rows.data(), nm * sizeof(rxo_row), hipMemcpyHostToDevice, sh.stream));
      HIPTRY(hipMemcpyAsync(o.orows.get(), orows.data(), nm * sizeof(rxs_row), hipMemcpyHostToDevice, sh.stream));
      HIPTRY(hipEventRecord(o.ev[0].get(), sh.stream));
      HIPTRY(rxo_launch_open(sh.stream, o.orows.get(), b.key_e.get(), n, reinterpret_cast<const uint8_t*>(b.pool.get()),
                             h.pool.size(), x.rows.get(), reinterpret_cast<uint8_t*>(x.plain.get()), plain_bytes, nm,
                             o.opened.get()));
      HIPTRY(hipEventRecord(o.ev[1].get(), sh.stream));
      if (const int rc = launch_set(sh, sb, x, comb, nm, rstride, plain_chunks, pool_chunks); rc < 0) return rc;
      drecs.resize(nm);
      opened.resize(nm);
      plain.resize(poff);
      HIPTRY(hipMemcpyAsync(drecs.data(), x.recs.get(), nm * sizeof(bmpow_rx_obj_rec), hipMemcpyDeviceToHost, sh.stream));
      HIPTRY(hipMemcpyAsync(opened.data(), o.opened.get(), nm * sizeof(int32_t), hipMemcpyDeviceToHost, sh.stream));
      HIPTRY(hipMemcpyAsync(plain.data(), x.plain.get(), poff, hipMemcpyDeviceToHost, sh.stream));
      HIPTRY(hipStreamSynchronize(sh.stream));
      if (const int rc = elapsed(st.open_ms, o.ev[0], o.ev[1]); rc < 0) return rc;
      if (const int rc = phase_times(x, st); rc < 0) return rc;
      st.matched += nm;
      st.launches += 10;
      st.rx_launches += 10;
      st.bytes_up += (uint64_t)nm * (sizeof(rxo_row) + sizeof(rxs_row));
      st.bytes_down += (uint64_t)nm * (sizeof(bmpow_rx_obj_rec) + sizeof(int32_t)) + poff;
      bmsched::parallel_for(nm, 1024, [&](size_t a, size_t z) {
        for (size_t k = a; k < z; ++k) {
          if (opened[k] < 0) continue;  // bad padding: the status of a row no key opened stands, match[] names the key
          const uint32_t orig = who[k];
          c.recs[orig] = drecs[k];
          c.plain_off[orig] = c.slot_off[orig];
          c.plain_len[orig] = (uint64_t)opened[k];
          if (opened[k]) std::memcpy(c.arena + c.slot_off[orig], plain.data() + rows[k].poff, (size_t)opened[k]);
        }
      });
    }
    i0 = i1;
  }
  return 0;
}

bool kind_ok(int kind) { return kind == BMPOW_RXO_KIND_BROADCAST || kind == BMPOW_RXO_KIND_PUBKEY; }

bool needed_tryable(const bmpow_rx_obj_tables& t, size_t e) {
  const uint8_t both = BMPOW_RXOS_NEEDED_DECODED | BMPOW_RXOS_NEEDED_OWN_TAG;
  return (t.needed_flags[e] & both) == both;
}

}  // namespace
}  // namespace bmhost

using namespace bmhost;

extern "C" {

int bmpow_rx_sealed_objects(size_t n, const uint8_t* kinds, const uint8_t* const* objs, const uint64_t* obj_lens,
                            const bmpow_rx_obj_tables* tables, bmpow_rx_obj_rec* recs, int32_t* match, uint8_t* arena,
                            uint64_t arena_cap, uint64_t* plain_off, uint64_t* plain_len) {
  std::lock_guard<FairMutex> lk(g_mu);
  if (n == 0) return 0;
  if (!kinds || !objs || !obj_lens || !tables || !recs || !match || !plain_off || !plain_len)
    return set_err(BMPOW_E_ARG, "null pointer");
  const bmpow_rx_obj_tables& t = *tables;
  if (t.n_trial && (!t.trial_priv32 || !t.trial_ripe20)) return set_err(BMPOW_E_ARG, "null pointer");
  if (t.n_tags && (!t.tag32 || !t.tag_priv32)) return set_err(BMPOW_E_ARG, "null pointer");
  if (t.n_needed && (!t.needed_tag32 || !t.needed_priv32 || !t.needed_ripe20 || !t.needed_version || !t.needed_stream ||
                     !t.needed_flags))
    return set_err(BMPOW_E_ARG, "null pointer");
  // one table of digits holds all three: its indices are int32
  if (n > 0xffffffffull || t.n_trial > 0x1fffffffull || t.n_tags > 0x1fffffffull || t.n_needed > 0x1fffffffull)
    return set_err(BMPOW_E_ARG, "too many objects or keys");
  const auto t_begin = std::chrono::steady_clock::now();
  std::vector<uint64_t> slot_off(n);
  uint64_t total = 0;
  for (size_t i = 0; i < n; ++i) {
    if (!kind_ok(kinds[i])) return set_err(BMPOW_E_ARG, "unknown kind of object");
    if (obj_lens[i] && !objs[i]) return set_err(BMPOW_E_ARG, "null object pointer");
    if (obj_lens[i] > (1ull << 31)) return set_err(BMPOW_E_ARG, "object above 2^31 bytes");
    slot_off[i] = total;
    total += obj_lens[i];
  }
  if (arena_cap < total) return set_err(BMPOW_E_ARG, "arena smaller than the objects together");
  if (total && !arena) return set_err(BMPOW_E_ARG, "null pointer");
  // the digits of every key that may be tried: trial keys, tag keys, needed entries' keys (the key 1 stands in for
  // an entry that is never tried)
  std::vector<int32_t> dig((t.n_trial + t.n_tags + t.n_needed) * EC_DIGITS);
  {
    int32_t* d = dig.data();
    const auto put = [&](const uint8_t* key32, bool tried) {
      const U256 key = tried ? u256_from_be(key32) : U256{{1, 0, 0, 0}};
      if (!key_in_range(key)) return false;
      recode_key(key, d);
      d += EC_DIGITS;
      return true;
    };
    bool good = true;
    for (size_t k = 0; k < t.n_trial; ++k) good = good && put(t.trial_priv32 + 32 * k, true);
    for (size_t k = 0; k < t.n_tags; ++k) good = good && put(t.tag_priv32 + 32 * k, true);
    for (size_t k = 0; k < t.n_needed; ++k) good = good && put(t.needed_priv32 + 32 * k, needed_tryable(t, k));
    if (!good) return set_err(BMPOW_E_ARG, "private key is zero or not below the group order");
  }
  const TagTable by_tag(t.tag32, t.n_tags), by_needed(t.needed_tag32, t.n_needed);

  std::vector<const uint8_t*> payloads;
  std::vector<uint64_t> pay_lens;
  std::vector<Sealed> pay;
  std::vector<Item> items;
  std::vector<uint32_t> clear;
  for (size_t i = 0; i < n; ++i) {
    match[i] = -1;
    plain_off[i] = plain_len[i] = 0;
    bmpow_rx_obj_rec& rec = recs[i];
    const RouteClass cls = route_object(kinds[i], objs[i], obj_lens[i], rec);
    int32_t entry = -1;
    switch (cls) {
      case ROUTE_DONE:
        continue;
      case ROUTE_CLEAR:
        clear.push_back((uint32_t)i);
        continue;
      case ROUTE_NO_TAG:
        rec.status = rec.kind == BMPOW_RXO_KIND_BROADCAST ? BMPOW_RXO_NOT_SUBSCRIBED : BMPOW_RXO_NOT_NEEDED;
        continue;
      case ROUTE_V4_SHORT:
        rec.status = BMPOW_RXO_V4_TOO_SHORT;
        continue;
      case ROUTE_TRIAL:
        rec.status = BMPOW_RXO_NOT_SUBSCRIBED;
        if (t.n_trial == 0) continue;
        break;
      case ROUTE_TAG:
        entry = by_tag.find(objs[i] + rec.tag_off);
        rec.status = entry < 0 ? BMPOW_RXO_NOT_SUBSCRIBED : BMPOW_RXO_NOT_DECRYPTED;
        if (entry < 0) continue;
        break;
      case ROUTE_NEEDED:
        entry = by_needed.find(objs[i] + rec.tag_off);  // 32 whole bytes: the object has at least 350
        if (entry < 0) {
          rec.status = BMPOW_RXO_NOT_NEEDED;
          continue;
        }
        if (!(t.needed_flags[entry] & BMPOW_RXOS_NEEDED_DECODED) || t.needed_version[entry] != rec.object_version ||
            t.needed_stream[entry] != rec.object_stream) {
          rec.status = BMPOW_RXO_ADDRESS_MISMATCH;
          continue;
        }
        if (!(t.needed_flags[entry] & BMPOW_RXOS_NEEDED_OWN_TAG)) {  // the entry is another address's
          rec.status = BMPOW_RXO_NOT_NEEDED;
          continue;
        }
        rec.status = BMPOW_RXO_NOT_DECRYPTED;
        break;
    }
    Item it;
    const uint8_t* p = objs[i] + rec.payload_off;  // payload_off <= the object's length
    const uint64_t len = obj_lens[i] - rec.payload_off;
    if (!ecies_parse(p, len, it.hdr)) continue;
    it.orig = (uint32_t)payloads.size();
    it.nblk = mac_blocks(len - 32);
    items.push_back(it);
    payloads.push_back(p);
    pay_lens.push_back(len);
    pay.push_back(Sealed{(uint32_t)i, (uint8_t)cls, entry});
  }
  std::stable_sort(items.begin(), items.end(), [](const Item& a, const Item& b) { return a.nblk > b.nblk; });
  int rc = 0;
  if (!items.empty() || !clear.empty()) {
    const Call c{objs, obj_lens, tables, recs, match, arena, slot_off.data(), plain_off, plain_len};
    rc = init_locked();
    if (rc >= 0) g_sealed_obj_stats.calls++;
    if (rc >= 0 && !clear.empty()) rc = clear_run_locked(clear, c);
    if (rc >= 0 && !items.empty()) rc = sealed_run_locked(items, payloads.data(), pay_lens.data(), pay, dig, c);
    if (rc > 0) rc = 0;
  }
  g_sealed_obj_stats.rows += n;
  g_sealed_obj_stats.host_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
  return rc;
}

int bmpow_rx_sealed_object_plan(int kind, const uint8_t* obj, size_t len, int* routed, size_t* payload_off,
                                size_t* tag_off, size_t* body_off, size_t* clen, int* reason) {
  if ((len && !obj) || !routed || !payload_off || !tag_off || !body_off || !clen || !reason)
    return set_err(BMPOW_E_ARG, "null pointer");
  if (!kind_ok(kind)) return set_err(BMPOW_E_ARG, "unknown kind of object");
  if (len > (1ull << 31)) return set_err(BMPOW_E_ARG, "object above 2^31 bytes");
  *payload_off = *tag_off = *body_off = *clen = 0;
  bmpow_rx_obj_rec rec;
  const RouteClass cls = route_object(kind, obj, len, rec);
  *routed = rec.kind;
  if (cls == ROUTE_DONE && (kind == BMPOW_RXO_KIND_BROADCAST || rec.payload_off == 0)) {
    *reason = BMPOW_RXS_PLAN_HEAD;  // no payload_off: the varints in front of it did not decode, or the version refuses
    return 0;
  }
  *payload_off = rec.payload_off;
  *tag_off = kind == BMPOW_RXO_KIND_BROADCAST || cls == ROUTE_NEEDED || cls == ROUTE_V4_SHORT ? rec.tag_off : rec.payload_off;
  if (cls == ROUTE_DONE || cls == ROUTE_CLEAR) {
    *reason = BMPOW_RXOS_PLAN_CLEAR;
    return 0;
  }
  if (cls == ROUTE_V4_SHORT) {
    *reason = BMPOW_RXOS_PLAN_V4_SHORT;
    return 0;
  }
  Parsed p;
  if (cls == ROUTE_NO_TAG || !ecies_parse(obj + rec.payload_off, len - rec.payload_off, p)) {
    *reason = BMPOW_RXS_PLAN_PAYLOAD;  // a v5 tag cut short leaves no payload at all
    return 0;
  }
  *body_off = p.body_off;
  *clen = len - rec.payload_off - 32 - p.body_off;
  if (*clen == 0 || *clen % 16) {
    *reason = BMPOW_RXS_PLAN_CIPHER;
    return 0;
  }
  *reason = BMPOW_RXS_PLAN_OK;
  return 1;
}

int bmpow_rx_sealed_obj_get_stats(bmpow_rx_sealed_obj_stats* out) {
  std::lock_guard<FairMutex> lk(g_mu);
  if (!out) return set_err(BMPOW_E_ARG, "null pointer");
  *out = g_sealed_obj_stats;
  return 0;
}

void bmpow_rx_sealed_obj_reset_stats(void) {
  std::lock_guard<FairMutex> lk(g_mu);
  g_sealed_obj_stats = bmpow_rx_sealed_obj_stats{};
}

}  // extern "C"
