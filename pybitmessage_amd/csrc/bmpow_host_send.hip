// bmpow_host_send.hip -- the send side's host unit: the set loop that takes public keys, signatures and ECIES
// key agreements through the device (range checks, draws and DER from bmpow_host_scalar.h), the AES / HMAC pass
// of the blobs -- libcrypto on the host's threads, or the seal kernel behind the ladder
// (bmpow_host_seal.hip), by bmpow_send_set_seal -- and the entry points of include/bmpow_send.h.
#include "bmpow_host_seal.h"

#include <openssl/evp.h>

#include "../../include/bmpow_send.h"
#include "bmpow_set_plan.h"

// ---------------------------------------------------------------------------------------
// One call: the rows whose inputs are in range go through the device in sets of at most kSendSetRows
// rows (and, with messages to hash, kSendSetPoolBytes of padded blocks; those rows sorted by block
// count, descending, so a wave's 64 lanes hash alike).  Per set: upload, then the phases one launch
// each -- hash, comb, then the signature's scalars, or the ephemeral key's digits, the recipient tables
// (ec_prep_kernel) and the ladder -- with the abort flag read between sets and before the ladder.  One
// loop serves the three kinds of call.  The buffers are the call's own: a KeySet (bmpow_host_sendkit.h) for
// the scalars, their points and the key agreement, SendBufs for the signature's; those that held a private
// key, a nonce, an ephemeral key or a derived key zero themselves before they are released, on the device
// (WipeDevBuf) and on the host (Wiped).  Everything runs on the first shard's device and stream.
// ---------------------------------------------------------------------------------------
namespace bmhost {
namespace {

constexpr size_t kSendSetRows = 1u << 18;  // as the signature and ECIES sets: 4,096 waves, 128 MB of key tables
constexpr size_t kSendSetPoolBytes = 256ull << 20;

bmpow_send_stats g_send_stats{};  // under g_mu

struct SendBufs {  // one call's buffers on the device, beside its KeySet
  WipeDevBuf<sc> d;
  DevBuf<sc> e, rs;
  DevBuf<sg_sig> sigs;
  DevBuf<uint4> pool;
  DevBuf<uint8_t> ok8;
  Event ev[5];
};

enum SendMode { kModePubkeys, kModeSign, kModeEncrypt };

// Inputs and outputs are the caller's arrays, indexed by the caller's row; `rows` lists the rows that go
// to the device (every scalar of theirs in [1, n - 1], every coordinate below p).
struct SendCall {
  SendMode mode;
  const uint8_t* scalars = nullptr;  // 32 bytes per row: the private key (pubkeys), the nonce (sign), the ephemeral key
  // sign: the keys, and the digests (32 bytes per row) or the messages with the digest to take
  const uint8_t* priv = nullptr;
  const uint8_t* digests = nullptr;
  const uint8_t* const* msgs = nullptr;
  const uint64_t* msg_lens = nullptr;
  int digest = 0;
  const uint8_t* pubkeys = nullptr;  // encrypt: X || Y per row
  uint8_t* xy = nullptr;   // pubkeys, encrypt: X || Y of scalar G
  uint8_t* rs = nullptr;   // sign: r || s
  uint8_t* key = nullptr;  // encrypt: key_e || key_m
  uint8_t* ok = nullptr;   // sign: r and s nonzero; encrypt: the recipient key is on the curve
  // encrypt, sealed on the device: the derived keys and the points stay there (xy, key and ok are not
  // written); the blobs go straight to outs / out_lens, 0 for a recipient key off the curve
  bool seal = false;
  const uint8_t* const* plains = nullptr;
  const uint64_t* lens = nullptr;
  const uint8_t* ivs = nullptr;
  uint8_t* const* outs = nullptr;
  uint64_t* out_lens = nullptr;
};

int send_run_locked(const SendCall& c, std::vector<uint32_t>& rows) {
  const bool hashing = c.mode == kModeSign && c.msgs, sign = c.mode == kModeSign, agree = c.mode == kModeEncrypt;
  // The order and the sets.  Messages to hash go by block count, descending, and are cut as the receive side
  // cuts its own (plan_set: rows and pool bytes), and so are the rows with nothing to hash (no blocks: rows
  // alone); plaintexts to seal go by AES block count and are laid out in slots by the seal's planner.
  const auto blocks_of = [&](uint32_t row) { return hashing ? msg_blocks(c.msg_lens[row]) : 0u; };
  bmseal::SlotPlan p;
  if (hashing)
    std::stable_sort(rows.begin(), rows.end(), [&](uint32_t a, uint32_t b) { return blocks_of(a) > blocks_of(b); });
  if (c.seal) {
    std::stable_sort(rows.begin(), rows.end(), [&](uint32_t a, uint32_t b) { return c.lens[a] / 16 > c.lens[b] / 16; });
    p.slot.reserve(rows.size());
    for (uint32_t row : rows) p.slot.push_back(bmseal::seal_slot_bytes(c.lens[row]));
    if (!p.plan(kSendSetRows, kSendSetPoolBytes)) return set_err(BMPOW_E_ARG, "seal plan refused");
  }
  Shard& sh = g_shards[0];
  HIPTRY(hipSetDevice(sh.dev));
  const ec::ge* comb = nullptr;
  if (const int rc = addr_comb16_table(sh, &comb); rc < 0) return rc;
  SendBufs b;
  KeySet ks;
  for (Event& e : b.ev) HIPTRY(e.alloc(sh.dev));
  g_send_stats.calls++;

  // the buffers that hold secrets, on the device and on the host, sized once for the largest set
  const size_t cap = std::min(rows.size(), kSendSetRows), cap_stride = round_up((uint32_t)cap, SD_BLOCK);
  if (const int rc = ks.alloc(sh.dev, cap_stride, agree); rc < 0) return rc;
  Wiped<sc> d;
  Wiped<uint64_t> kout;
  if (sign) {
    d.v.resize(cap);
    HIPTRY(b.d.alloc(sh.dev, cap_stride));
  }
  if (agree && !c.seal) kout.v.resize(8 * cap_stride);
  SealIo sio;
  if (c.seal) {
    if (const int rc = sio.init(sh.dev, cap, p.sets.max_pool); rc < 0) return rc;
    g_seal_stats.calls++;
  }
  std::vector<sc> e, rs;
  std::vector<sg_sig> sigs;
  std::vector<uint8_t> pool, ok8;
  std::vector<ec::ge> pt;
  std::vector<uint32_t> ok32;
  for (size_t i0 = 0, k = 0; i0 < rows.size(); ++k) {
    if (g_abort.load()) return set_err(BMPOW_E_ABORTED, "aborted");
    const SetCut cut = c.seal ? SetCut{p.sets.begin[k + 1], 0} : plan_set(rows, i0, blocks_of, kSendSetRows, kSendSetPoolBytes);
    if (cut.blocks > 0xffffffffull) return set_err(BMPOW_E_ARG, "message pool above 2^32 blocks");
    const size_t i1 = cut.i1;
    const uint32_t n = (uint32_t)(i1 - i0), stride = round_up(n, SD_BLOCK);
    for (uint32_t j = 0; j < n; ++j) {
      const size_t row = rows[i0 + j];
      ks.stage(j, c.scalars + 32 * row, agree ? c.pubkeys + 64 * row : nullptr);
    }
    if (const int rc = ks.upload(sh.stream, n); rc < 0) return rc;
    if (sign) {
      for (uint32_t j = 0; j < n; ++j) d.v[j] = sc_from_be(c.priv + 32 * (size_t)rows[i0 + j]);
      HIPTRY(b.e.grow(sh.dev, (size_t)2 * stride));
      HIPTRY(b.rs.grow(sh.dev, (size_t)2 * stride));
      HIPTRY(b.ok8.grow(sh.dev, stride));
      HIPTRY(hipMemcpyAsync(b.d.get(), d.v.data(), n * sizeof(sc), hipMemcpyHostToDevice, sh.stream));
      if (hashing) {
        sigs.assign(n, sg_sig{});
        pool.resize(cut.blocks * 64);
        uint32_t blk = 0;
        for (uint32_t j = 0; j < n; ++j) {
          sigs[j].blk = blk;
          sigs[j].nblk = blocks_of(rows[i0 + j]);
          blk += sigs[j].nblk;
        }
        bmsched::parallel_for(n, 1024, [&](size_t a, size_t z) {
          for (size_t j = a; j < z; ++j) {
            const uint32_t row = rows[i0 + j];
            pad_blocks(c.msgs[row], c.msg_lens[row], pool.data() + (size_t)sigs[j].blk * 64, sigs[j].nblk);
          }
        });
        HIPTRY(b.sigs.grow(sh.dev, stride));
        HIPTRY(b.pool.grow(sh.dev, pool.size() / sizeof(uint4)));
        HIPTRY(hipMemcpyAsync(b.sigs.get(), sigs.data(), n * sizeof(sg_sig), hipMemcpyHostToDevice, sh.stream));
        HIPTRY(hipMemcpyAsync(b.pool.get(), pool.data(), pool.size(), hipMemcpyHostToDevice, sh.stream));
      } else {
        e.resize(n);
        for (uint32_t j = 0; j < n; ++j) e[j] = sc_from_be(c.digests + 32 * (size_t)rows[i0 + j]);
        HIPTRY(hipMemcpyAsync(b.e.get(), e.data(), n * sizeof(sc), hipMemcpyHostToDevice, sh.stream));
      }
    }
    // the selected digest's plane of e: SHA-1 first, SHA-256 behind it; a given digest is the first
    const sc* e_dev = sign ? b.e.get() + (hashing && c.digest == BMPOW_SIG_SHA256 ? stride : 0) : nullptr;
    uint64_t launches = 1;
    HIPTRY(hipEventRecord(b.ev[0].get(), sh.stream));
    if (hashing) {
      HIPTRY(sg_launch_hash(sh.stream, b.sigs.get(), b.pool.get(), n, stride, b.e.get()));
      ++launches;
    }
    HIPTRY(hipEventRecord(b.ev[1].get(), sh.stream));
    if (agree) {
      if (const int rc = ks.launch_ephemeral(sh.stream, comb, n, stride, &b.ev[2]); rc < 0) return rc;
      ++launches;
    } else {
      HIPTRY(sd_launch_comb(sh.stream, comb, ks.kw.get(), n, stride, ks.pt.get()));
      HIPTRY(hipEventRecord(b.ev[2].get(), sh.stream));
      if (sign) {
        HIPTRY(sd_launch_sign(sh.stream, ks.pt.get(), ks.kw.get(), b.d.get(), e_dev, n, stride, b.rs.get(), b.ok8.get()));
        ++launches;
      }
    }
    HIPTRY(hipEventRecord(b.ev[3].get(), sh.stream));
    if (agree) {
      if (g_abort.load()) {
        HIPTRY(hipStreamSynchronize(sh.stream));
        return set_err(BMPOW_E_ABORTED, "aborted");
      }
      if (const int rc = ks.launch_shared(sh.stream, n, stride); rc < 0) return rc;
      launches += 2;
    }
    HIPTRY(hipEventRecord(b.ev[4].get(), sh.stream));
    if (sign) {
      rs.resize((size_t)2 * stride);
      ok8.resize(n);
      HIPTRY(hipMemcpyAsync(rs.data(), b.rs.get(), rs.size() * sizeof(sc), hipMemcpyDeviceToHost, sh.stream));
      HIPTRY(hipMemcpyAsync(ok8.data(), b.ok8.get(), n, hipMemcpyDeviceToHost, sh.stream));
    } else if (c.seal) {
      SealSet s;
      s.n = n, s.stride = stride;
      s.row = rows.data() + i0, s.off = p.off.data() + i0;
      s.pool_bytes = p.pool_bytes(k);
      s.plains = c.plains, s.lens = c.lens, s.ivs = c.ivs, s.outs = c.outs, s.out_lens = c.out_lens;
      if (const int rc = seal_set(sh, sio, s, ks.kout.get(), ks.pt.get(), ks.ok32.get()); rc < 0) return rc;
    } else {
      pt.resize(n);
      HIPTRY(hipMemcpyAsync(pt.data(), ks.pt.get(), n * sizeof(ec::ge), hipMemcpyDeviceToHost, sh.stream));
      if (agree) {
        ok32.resize(n);
        HIPTRY(hipMemcpyAsync(ok32.data(), ks.ok32.get(), n * sizeof(uint32_t), hipMemcpyDeviceToHost, sh.stream));
        HIPTRY(hipMemcpyAsync(kout.v.data(), ks.kout.get(), (size_t)8 * stride * sizeof(uint64_t), hipMemcpyDeviceToHost,
                              sh.stream));
      }
    }
    HIPTRY(hipStreamSynchronize(sh.stream));
    // with nothing hashed ev[0] .. ev[1] is the gap between two records, no phase: hash_ms stays as it is
    double* const acc[4] = {&g_send_stats.hash_ms, &g_send_stats.comb_ms, &g_send_stats.scalar_ms, &g_send_stats.ladder_ms};
    const int skip = hashing ? 0 : 1;
    if (const int rc = elapsed_phases(acc + skip, b.ev + skip, 4 - skip); rc < 0) return rc;
    for (uint32_t j = 0; j < n && !c.seal; ++j) {
      const size_t row = rows[i0 + j];
      if (sign) {
        c.ok[row] = ok8[j] ? 1 : 0;
        if (ok8[j]) {
          sc_to_be(rs[j].d, c.rs + 64 * row);
          sc_to_be(rs[(size_t)stride + j].d, c.rs + 64 * row + 32);
        }
        continue;
      }
      sc_to_be(pt[j].x.d, c.xy + 64 * row);
      sc_to_be(pt[j].y.d, c.xy + 64 * row + 32);
      c.ok[row] = 1;
      if (agree) {
        c.ok[row] = ok32[j] ? 1 : 0;
        if (ok32[j])
          for (int w = 0; w < 8; ++w)
            for (int q = 0; q < 8; ++q) c.key[64 * row + 8 * w + q] = (uint8_t)(kout.v[(size_t)w * stride + j] >> (56 - 8 * q));
      }
    }
    g_send_stats.rows += n;
    g_send_stats.sets++;
    g_send_stats.launches += launches;
    i0 = i1;
  }
  return 0;
}

int run_rows(const SendCall& c, std::vector<uint32_t>& rows) {
  if (rows.empty()) return 0;
  int rc = init_locked();
  if (rc >= 0) rc = send_run_locked(c, rows);
  return rc > 0 ? 0 : rc;
}

// libcrypto's contexts for a run of blobs on one thread.  The algorithms are fetched once for the process:
// an EVP_aes_256_cbc() / HMAC() call per blob looks them up again every time (OpenSSL 3), which cost more
// than the 200-byte blob's AES and HMAC together and serialised the host's threads on the library's lock.
struct Sealer {
  EVP_CIPHER_CTX* c = EVP_CIPHER_CTX_new();
  EVP_MD_CTX* m = EVP_MD_CTX_new();
  ~Sealer() {
    EVP_CIPHER_CTX_free(c);
    EVP_MD_CTX_free(m);
  }
  static const EVP_CIPHER* aes() {
    static const EVP_CIPHER* a = EVP_CIPHER_fetch(nullptr, "AES-256-CBC", nullptr);
    return a;
  }
  static const EVP_MD* sha() {
    static const EVP_MD* s = EVP_MD_fetch(nullptr, "SHA256", nullptr);
    return s;
  }
  bool ready() const { return c && m && aes() && sha(); }
  bool hash2(const uint8_t* a, size_t al, const uint8_t* b, size_t bl, uint8_t out[32]) {
    unsigned int l = 0;
    return EVP_DigestInit_ex(m, sha(), nullptr) == 1 && EVP_DigestUpdate(m, a, al) == 1 &&
           EVP_DigestUpdate(m, b, bl) == 1 && EVP_DigestFinal_ex(m, out, &l) == 1 && l == 32;
  }
  // HMAC-SHA256 with a 32-byte key: H((K ^ opad) || H((K ^ ipad) || data))
  bool hmac(const uint8_t key[32], const uint8_t* data, size_t len, uint8_t mac[32]) {
    uint8_t pad[64], inner[32];
    for (int i = 0; i < 64; ++i) pad[i] = (i < 32 ? key[i] : 0) ^ 0x36;
    bool good = hash2(pad, 64, data, len, inner);
    for (int i = 0; i < 64; ++i) pad[i] ^= 0x36 ^ 0x5c;
    good = good && hash2(pad, 64, inner, 32, mac);
    OPENSSL_cleanse(pad, sizeof pad);
    return good;
  }
};

// what bmpow_ecies_seal documents; the error text is left in g_err
int64_t ecies_seal(Sealer& sl, const uint8_t* plain, size_t len, const uint8_t* iv, const uint8_t* R, const uint8_t* key,
                   uint8_t* out, size_t out_cap) {
  if (len > 0x7fffffffu - 16) return set_err(BMPOW_E_ARG, "plaintext above 2^31 - 16 bytes");
  if (!sl.ready()) return set_err(BMPOW_E_ARG, "libcrypto has no AES-256-CBC or SHA-256");
  size_t xs = 0, ys = 0;  // leading zero bytes BN_bn2bin drops
  while (xs < 32 && R[xs] == 0) ++xs;
  while (ys < 32 && R[32 + ys] == 0) ++ys;
  const size_t xl = 32 - xs, yl = 32 - ys, clen = 16 * (len / 16 + 1), head = 16 + 2 + 2 + xl + 2 + yl;
  if (out_cap < head + clen + 32) return set_err(BMPOW_E_ARG, "output buffer smaller than the blob");
  uint8_t* p = out;
  std::memcpy(p, iv, 16);
  p += 16;
  *p++ = 0x02, *p++ = 0xCA;  // secp256k1 in pyelliptic's numbering: 714
  *p++ = 0, *p++ = (uint8_t)xl;
  std::memcpy(p, R + xs, xl);
  p += xl;
  *p++ = 0, *p++ = (uint8_t)yl;
  std::memcpy(p, R + 32 + ys, yl);
  p += yl;
  int n1 = 0, n2 = 0;
  const uint8_t none = 0;
  const bool good = EVP_EncryptInit_ex(sl.c, Sealer::aes(), nullptr, key, iv) == 1 &&
                    EVP_EncryptUpdate(sl.c, p, &n1, len ? plain : &none, (int)len) == 1 &&
                    EVP_EncryptFinal_ex(sl.c, p + n1, &n2) == 1 && (size_t)(n1 + n2) == clen &&
                    sl.hmac(key + 32, out, head + clen, p + clen);
  if (!good) return set_err(BMPOW_E_ARG, "libcrypto refused the AES or HMAC pass");
  return (int64_t)(head + clen + 32);
}

}  // namespace
}  // namespace bmhost

using namespace bmhost;

extern "C" {

int bmpow_ec_pubkeys(size_t n, const uint8_t* priv, uint8_t* pub_out, uint8_t* ok) {
  std::lock_guard<FairMutex> lk(g_mu);
  if (n == 0) return 0;
  if (!priv || !pub_out || !ok) return set_err(BMPOW_E_ARG, "null pointer");
  if (n > 0xffffffffull) return set_err(BMPOW_E_ARG, "too many keys");
  WallClock clock{g_send_stats.host_ms};
  std::memset(pub_out, 0, 64 * n);
  std::memset(ok, 0, n);
  std::vector<uint32_t> rows;
  rows.reserve(n);
  for (size_t i = 0; i < n; ++i)
    if (scalar_in_range(priv + 32 * i)) rows.push_back((uint32_t)i);
  SendCall c;
  c.mode = kModePubkeys;
  c.scalars = priv;
  c.xy = pub_out;
  c.ok = ok;
  return run_rows(c, rows);
}

int bmpow_ecdsa_sign_digest(size_t n, const uint8_t* priv, const uint8_t* k, const uint8_t* e, uint8_t* rs_out,
                            uint8_t* ok) {
  std::lock_guard<FairMutex> lk(g_mu);
  if (n == 0) return 0;
  if (!priv || !k || !e || !rs_out || !ok) return set_err(BMPOW_E_ARG, "null pointer");
  if (n > 0xffffffffull) return set_err(BMPOW_E_ARG, "too many rows");
  WallClock clock{g_send_stats.host_ms};
  std::memset(rs_out, 0, 64 * n);
  std::memset(ok, 0, n);
  std::vector<uint32_t> rows;
  rows.reserve(n);
  for (size_t i = 0; i < n; ++i)
    if (scalar_in_range(priv + 32 * i) && scalar_in_range(k + 32 * i)) rows.push_back((uint32_t)i);
  SendCall c;
  c.mode = kModeSign;
  c.scalars = k;
  c.priv = priv;
  c.digests = e;
  c.rs = rs_out;
  c.ok = ok;
  return run_rows(c, rows);
}

int bmpow_sig_der(const uint8_t rs[64], uint8_t out[72], size_t* len) {
  if (!rs || !out || !len) return set_err(BMPOW_E_ARG, "null pointer");
  if (all_zero(rs, 32) || all_zero(rs + 32, 32)) return set_err(BMPOW_E_ARG, "r or s is zero");
  *len = sig_der(rs, out);
  return 0;
}

int bmpow_sig_sign(size_t n, const uint8_t* const* msgs, const uint64_t* msg_lens, const uint8_t* privkeys, int digest,
                   const uint8_t* nonces, uint8_t* sig_out, uint8_t* sig_len) {
  std::lock_guard<FairMutex> lk(g_mu);
  if (n == 0) return 0;
  if (!msgs || !msg_lens || !privkeys || !sig_out || !sig_len) return set_err(BMPOW_E_ARG, "null pointer");
  if (n > 0xffffffffull) return set_err(BMPOW_E_ARG, "too many messages");
  if (digest != BMPOW_SIG_SHA1 && digest != BMPOW_SIG_SHA256) return set_err(BMPOW_E_ARG, "digest is neither SHA-1 nor SHA-256");
  WallClock clock{g_send_stats.host_ms};
  std::memset(sig_out, 0, 72 * n);
  std::memset(sig_len, 0, n);
  for (size_t i = 0; i < n; ++i) {
    if (msg_lens[i] && !msgs[i]) return set_err(BMPOW_E_ARG, "null message pointer");
    if (msg_lens[i] > (1ull << 31)) return set_err(BMPOW_E_ARG, "message above 2^31 bytes");
    if (!scalar_in_range(privkeys + 32 * i)) return set_err(BMPOW_E_ARG, "private key is zero or not below the group order");
    if (nonces && !scalar_in_range(nonces + 32 * i)) return set_err(BMPOW_E_ARG, "nonce is zero or not below the group order");
  }
  Wiped<uint8_t> drawn;
  if (!nonces) {
    drawn.v.resize(32 * n);
    if (!draw_scalars(drawn.v.data(), n)) return set_err(BMPOW_E_ARG, "RAND_bytes failed");
  }
  std::vector<uint8_t> rs(64 * n), ok(n, 0);
  SendCall c;
  c.mode = kModeSign;
  c.scalars = nonces ? nonces : drawn.v.data();
  c.priv = privkeys;
  c.msgs = msgs;
  c.msg_lens = msg_lens;
  c.digest = digest;
  c.rs = rs.data();
  c.ok = ok.data();
  std::vector<uint32_t> rows(n);
  for (size_t i = 0; i < n; ++i) rows[i] = (uint32_t)i;
  if (const int rc = sign_passes(
          rows, nonces ? nullptr : drawn.v.data(), [&](std::vector<uint32_t>& r) { return run_rows(c, r); },
          [&](uint32_t row) { return !ok[row]; });
      rc < 0)
    return rc;
  for (size_t i = 0; i < n; ++i)
    if (ok[i]) sig_len[i] = (uint8_t)sig_der(rs.data() + 64 * i, sig_out + 72 * i);
  return 0;
}

int64_t bmpow_ecies_seal(const uint8_t* plain, size_t len, const uint8_t iv[16], const uint8_t R_xy[64],
                         const uint8_t key[64], uint8_t* out, size_t out_cap) {
  if ((len && !plain) || !iv || !R_xy || !key || !out) return set_err(BMPOW_E_ARG, "null pointer");
  Sealer sl;
  return ecies_seal(sl, plain, len, iv, R_xy, key, out, out_cap);
}

int bmpow_ecies_encrypt(size_t n, const uint8_t* const* plains, const uint64_t* lens, const uint8_t* pubkeys,
                        const uint8_t* ephem, const uint8_t* ivs, uint8_t* const* outs, const uint64_t* out_caps,
                        uint64_t* out_lens) {
  std::lock_guard<FairMutex> lk(g_mu);
  if (n == 0) return 0;
  if (!plains || !lens || !pubkeys || !outs || !out_caps || !out_lens) return set_err(BMPOW_E_ARG, "null pointer");
  if (n > 0xffffffffull) return set_err(BMPOW_E_ARG, "too many plaintexts");
  WallClock clock{g_send_stats.host_ms};
  std::memset(out_lens, 0, n * sizeof(uint64_t));
  for (size_t i = 0; i < n; ++i) {
    if ((lens[i] && !plains[i]) || !outs[i]) return set_err(BMPOW_E_ARG, "null plaintext or output pointer");
    if (lens[i] > 0x7fffffffu - 16) return set_err(BMPOW_E_ARG, "plaintext above 2^31 - 16 bytes");
    if (out_caps[i] < BMPOW_ECIES_BLOB_CAP(lens[i])) return set_err(BMPOW_E_ARG, "output buffer below BMPOW_ECIES_BLOB_CAP");
    if (ephem && !scalar_in_range(ephem + 32 * i))
      return set_err(BMPOW_E_ARG, "ephemeral key is zero or not below the group order");
  }
  Wiped<uint8_t> drawn, key;
  std::vector<uint8_t> iv_drawn;
  if (!ephem) {
    drawn.v.resize(32 * n);
    if (!draw_scalars(drawn.v.data(), n)) return set_err(BMPOW_E_ARG, "RAND_bytes failed");
  }
  if (!ivs) {
    iv_drawn.resize(16 * n);
    if (!draw_bytes(iv_drawn.data(), iv_drawn.size())) return set_err(BMPOW_E_ARG, "RAND_bytes failed");
    ivs = iv_drawn.data();
  }
  // Device mode: the rows up to the protocol's object size are sealed by the kernel behind their ladder;
  // a longer one takes the host's path below, as every row does in host mode.
  const bool device = seal_mode() == 1;
  std::vector<uint8_t> R, ok(n, 0);
  std::vector<uint32_t> rows, sealed;
  rows.reserve(n);
  for (size_t i = 0; i < n; ++i)
    if (coord_in_range(sc_from_be(pubkeys + 64 * i)) && coord_in_range(sc_from_be(pubkeys + 64 * i + 32)))
      (device && lens[i] <= bmseal::kDevicePlain ? sealed : rows).push_back((uint32_t)i);
  SendCall c;
  c.mode = kModeEncrypt;
  c.scalars = ephem ? ephem : drawn.v.data();
  c.pubkeys = pubkeys;
  if (!sealed.empty()) {
    SendCall d = c;
    d.seal = true;
    d.plains = plains, d.lens = lens, d.ivs = ivs, d.outs = outs, d.out_lens = out_lens;
    if (const int rc = run_rows(d, sealed); rc < 0) return rc;
    if (!rows.empty()) g_send_stats.calls--;  // one call, though its rows took two trips through the set loop
  }
  if (rows.empty()) return 0;
  key.v.resize(64 * n);
  R.resize(64 * n);
  c.xy = R.data();
  c.key = key.v.data();
  c.ok = ok.data();
  if (const int rc = run_rows(c, rows); rc < 0) return rc;
  if (device) g_seal_stats.rows_host += rows.size();
  const auto t_seal = std::chrono::steady_clock::now();
  std::atomic<bool> failed{false};
  bmsched::parallel_for(n, 256, [&](size_t a, size_t z) {
    Sealer sl;
    for (size_t i = a; i < z; ++i) {
      if (!ok[i]) continue;
      const int64_t l = ecies_seal(sl, plains[i], lens[i], ivs + 16 * i, R.data() + 64 * i, key.v.data() + 64 * i,
                                   outs[i], out_caps[i]);
      if (l < 0) failed.store(true);
      else out_lens[i] = (uint64_t)l;
    }
  });
  g_send_stats.seal_ms += ms_since(t_seal);
  if (failed.load()) return set_err(BMPOW_E_ARG, "libcrypto refused the AES or HMAC pass");
  return 0;
}

int bmpow_send_get_stats(bmpow_send_stats* out) {
  std::lock_guard<FairMutex> lk(g_mu);
  if (!out) return set_err(BMPOW_E_ARG, "null pointer");
  *out = g_send_stats;
  return 0;
}

void bmpow_send_reset_stats(void) {
  std::lock_guard<FairMutex> lk(g_mu);
  g_send_stats = bmpow_send_stats{};
}

}  // extern "C"
