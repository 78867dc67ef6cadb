// bmpow_host_ecies.hip -- the ECIES trial decryption's host side: payload parsing, key recoding, the
// padded MAC pool, and the bmpow_ecdh / bmpow_ecies_* entry points (include/bmpow_ecies.h).
#include "bmpow_host_ecies.h"

#include <openssl/evp.h>

// ---------------------------------------------------------------------------------------
// One bmpow_ecies_match call: the well-formed objects, sorted by their MAC block count (descending, so a
// wave's 64 lanes iterate alike), go through the device in sets of at most kSetObjects objects and
// kSetPoolBytes of padded MAC blocks.  Per set: upload, one preparation launch (tables of every
// object's point), then for each group of keys one ladder launch and one MAC launch -- at most
// kLaunchPairs (object, key) pairs each, the library's rule of calls of about one engine launch, with
// the abort flag read between them.  The buffers are the call's own (DevBuf owners, released
// when it returns); everything runs on the first shard's device and stream.
// ---------------------------------------------------------------------------------------
namespace bmhost {

constexpr uint64_t kFold = 0x1000003D1ULL;  // 2^256 mod p
constexpr U256 kOrder = {{0xBFD25E8CD0364141ULL, 0xBAAEDCE6AF48A03BULL, 0xFFFFFFFFFFFFFFFEULL, 0xFFFFFFFFFFFFFFFFULL}};
constexpr U256 kPrime = {{0xFFFFFFFEFFFFFC2FULL, 0xFFFFFFFFFFFFFFFFULL, 0xFFFFFFFFFFFFFFFFULL, 0xFFFFFFFFFFFFFFFFULL}};

bool u256_less(const U256& a, const U256& b) {
  for (int i = 3; i >= 0; --i)
    if (a.w[i] != b.w[i]) return a.w[i] < b.w[i];
  return false;
}
bool u256_zero(const U256& a) { return (a.w[0] | a.w[1] | a.w[2] | a.w[3]) == 0; }
U256 u256_sub(const U256& a, const U256& b) {  // a - b mod 2^256
  U256 r;
  unsigned __int128 bw = 0;
  for (int i = 0; i < 4; ++i) {
    const unsigned __int128 t = (unsigned __int128)a.w[i] - b.w[i] - (uint64_t)bw;
    r.w[i] = (uint64_t)t;
    bw = (t >> 64) & 1;
  }
  return r;
}
uint64_t u256_add_small(U256& a, uint64_t v) {  // a += v; returns the carry out
  unsigned __int128 c = v;
  for (int i = 0; i < 4; ++i) {
    c += a.w[i];
    a.w[i] = (uint64_t)c;
    c >>= 64;
  }
  return (uint64_t)c;
}
U256 u256_from_be(const uint8_t* b) {
  U256 r;
  for (int i = 0; i < 4; ++i) r.w[3 - i] = bmsched::load_be64(b + 8 * i);
  return r;
}
void u256_to_be(const U256& a, uint8_t* out) {
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 8; ++j) out[8 * i + j] = (uint8_t)(a.w[3 - i] >> (56 - 8 * j));
}

// The big-endian integer b[0 .. len) mod p (BN_bin2bn takes any length; this OpenSSL reduces the
// coordinate before it checks the curve equation): Horner by bytes, 2^256 folding back as 2^32 + 977.
U256 coord_mod_p(const uint8_t* b, size_t len) {
  while (len && *b == 0) ++b, --len;
  U256 r = {{0, 0, 0, 0}};
  for (size_t i = 0; i < len; ++i) {
    const uint64_t top = r.w[3] >> 56;
    r.w[3] = (r.w[3] << 8) | (r.w[2] >> 56);
    r.w[2] = (r.w[2] << 8) | (r.w[1] >> 56);
    r.w[1] = (r.w[1] << 8) | (r.w[0] >> 56);
    r.w[0] = (r.w[0] << 8) | b[i];
    // a carry out of the fold leaves r < 2^41: the second fold cannot carry
    if (top && u256_add_small(r, top * kFold)) u256_add_small(r, kFold);
  }
  if (!u256_less(r, kPrime)) r = u256_sub(r, kPrime);
  return r;
}

ec::fe fe_from_u256(const U256& a) {
  ec::fe f;
  for (int i = 0; i < 4; ++i) {
    f.d[2 * i] = (uint32_t)a.w[i];
    f.d[2 * i + 1] = (uint32_t)(a.w[i] >> 32);
  }
  return f;
}

// The reference's slicing (ECC.decrypt, _decode_pubkey) never fails on a length by itself; what it
// leaves for a header that reaches into the last 32 bytes is a MAC shorter than 32 bytes or an unpack
// error: never a match.  Well-formed: the header lies inside data[:-32].
bool ecies_parse(const uint8_t* p, size_t len, Parsed& out) {
  if (len < 20) return false;
  const size_t xl = ((size_t)p[18] << 8) | p[19];
  if (len < 22 + xl) return false;
  const size_t yl = ((size_t)p[20 + xl] << 8) | p[21 + xl];
  const size_t off = 22 + xl + yl;
  if (len < off + 32) return false;
  out.x = coord_mod_p(p + 20, xl);
  out.y = coord_mod_p(p + 22 + xl, yl);
  out.body_off = off;
  return true;
}

// The 64 signed odd base-16 digits of a key 1 <= k < n (least significant first), of k itself when it
// is odd and of n - k otherwise: x(k R) = x((n - k) R).  Regular recoding: d_i = (k mod 32) - 16,
// k = (k - d_i) / 16 keeps k odd; the last digit is what is left, an odd number below 16.
void recode_key(const U256& key, int32_t* dig) {
  U256 k = (key.w[0] & 1) ? key : u256_sub(kOrder, key);
  for (int i = 0; i < EC_DIGITS - 1; ++i) {
    const int d = (int)(k.w[0] & 31) - 16;
    dig[i] = d;
    if (d < 0) u256_add_small(k, (uint64_t)(-d));
    else k = u256_sub(k, U256{{(uint64_t)d, 0, 0, 0}});
    k.w[0] = (k.w[0] >> 4) | (k.w[1] << 60);
    k.w[1] = (k.w[1] >> 4) | (k.w[2] << 60);
    k.w[2] = (k.w[2] >> 4) | (k.w[3] << 60);
    k.w[3] >>= 4;
  }
  dig[EC_DIGITS - 1] = (int32_t)k.w[0];
}

bool key_in_range(const U256& k) { return !u256_zero(k) && u256_less(k, kOrder); }

uint32_t mac_blocks(size_t maced_len) { return (uint32_t)((maced_len + 9 + 63) / 64); }

// data || 0x80 || zeros || the bit length of 64 + len as 8 big-endian bytes, into nblk * 64 bytes
void pad_mac_blocks(const uint8_t* data, size_t len, uint8_t* dst, uint32_t nblk) {
  const size_t total = (size_t)nblk * 64;
  std::memcpy(dst, data, len);
  dst[len] = 0x80;
  std::memset(dst + len + 1, 0, total - len - 1 - 8);
  const uint64_t bits = (uint64_t)(64 + len) * 8;
  for (int j = 0; j < 8; ++j) dst[total - 8 + j] = (uint8_t)(bits >> (56 - 8 * j));
}

bmpow_ecies_stats g_ecies_stats{};  // under g_mu

int ecies_events(EciesBufs& b, int dev) {
  for (Event& e : b.ev)
    if (!e) HIPTRY(e.alloc(dev));
  return 0;
}

size_t ecies_set_end(const std::vector<Item>& items, size_t i0, uint64_t& blocks) {
  const SetCut cut = plan_set(items, i0, [](const Item& it) { return it.nblk; }, kSetObjects, kSetPoolBytes);
  blocks = cut.blocks;
  return cut.i1;
}

int ecies_match_set(Shard& sh, EciesBufs& b, EciesStage& h, const Item* items, uint32_t n, uint64_t blocks,
                    const uint8_t* const* payloads, const uint64_t* lens, size_t n_keys, bool want_key_e,
                    bmpow_ecies_stats& st) {
  if (const int rc = ecies_stage_set(sh, b, h, items, n, blocks, payloads, lens, n_keys, want_key_e, st); rc < 0) return rc;
  if (const int rc = ecies_try_keys(sh, b, n, n, n_keys, want_key_e, st); rc < 0) return rc;
  h.match.resize(n);
  HIPTRY(hipMemcpyAsync(h.match.data(), b.match.get(), n * sizeof(int), hipMemcpyDeviceToHost, sh.stream));
  return 0;
}

int ecies_stage_set(Shard& sh, EciesBufs& b, EciesStage& h, const Item* items, uint32_t n, uint64_t blocks,
                    const uint8_t* const* payloads, const uint64_t* lens, size_t n_keys, bool want_key_e,
                    bmpow_ecies_stats& st) {
  if (blocks > 0xffffffffull) return set_err(BMPOW_E_ARG, "payload pool above 2^32 blocks");
  const uint32_t stride = (n + EC_BLOCK - 1) / EC_BLOCK * EC_BLOCK;
  std::vector<ec::ge>& pts = h.pts;
  std::vector<ec_obj>& objs = h.objs;
  std::vector<uint8_t>& pool = h.pool;
  pts.resize(n);
  objs.resize(n);
  pool.resize(blocks * 64);
  uint32_t blk = 0;
  for (uint32_t j = 0; j < n; ++j) {
    const Item& it = items[j];
    pts[j].x = fe_from_u256(it.hdr.x);
    pts[j].y = fe_from_u256(it.hdr.y);
    objs[j].blk = blk;
    objs[j].nblk = it.nblk;
    blk += it.nblk;
  }
  bmsched::parallel_for(n, 1024, [&](size_t a, size_t e) {
    for (size_t j = a; j < e; ++j) {
      const Item& it = items[j];
      const uint8_t* p = payloads[it.orig];
      const size_t maced = lens[it.orig] - 32;
      pad_mac_blocks(p, maced, pool.data() + (size_t)objs[j].blk * 64, it.nblk);
      for (int w = 0; w < 8; ++w)
        objs[j].mac[w] = (uint32_t)p[maced + 4 * w] << 24 | (uint32_t)p[maced + 4 * w + 1] << 16 |
                         (uint32_t)p[maced + 4 * w + 2] << 8 | p[maced + 4 * w + 3];
    }
  });
  const uint32_t kc = (uint32_t)std::max<size_t>(1, std::min<size_t>(n_keys, kLaunchPairs / stride));
  HIPTRY(b.pts.grow(sh.dev, stride));
  HIPTRY(b.tab.grow(sh.dev, (size_t)EC_ENTRIES * stride));
  HIPTRY(b.ok.grow(sh.dev, stride));
  HIPTRY(b.objs.grow(sh.dev, stride));
  HIPTRY(b.match.grow(sh.dev, stride));
  HIPTRY(b.pool.grow(sh.dev, std::max<size_t>(pool.size(), 64) / sizeof(uint4)));
  HIPTRY(b.kout.grow(sh.dev, (size_t)8 * kc * stride));
  if (want_key_e) HIPTRY(b.key_e.grow(sh.dev, (size_t)4 * stride));
  HIPTRY(hipMemcpyAsync(b.pts.get(), pts.data(), n * sizeof(ec::ge), hipMemcpyHostToDevice, sh.stream));
  HIPTRY(hipMemcpyAsync(b.objs.get(), objs.data(), n * sizeof(ec_obj), hipMemcpyHostToDevice, sh.stream));
  HIPTRY(hipMemcpyAsync(b.pool.get(), pool.data(), pool.size(), hipMemcpyHostToDevice, sh.stream));
  HIPTRY(hipMemsetAsync(b.match.get(), 0x7f, (size_t)stride * sizeof(int), sh.stream));
  if (want_key_e) HIPTRY(hipMemsetAsync(b.key_e.get(), 0, (size_t)4 * stride * sizeof(uint64_t), sh.stream));
  if (g_abort.load()) return set_err(BMPOW_E_ABORTED, "aborted");
  HIPTRY(hipEventRecord(b.ev[0].get(), sh.stream));
  HIPTRY(ec_launch_prep(sh.stream, b.pts.get(), n, stride, b.tab.get(), b.ok.get()));
  HIPTRY(hipEventRecord(b.ev[1].get(), sh.stream));
  HIPTRY(hipStreamSynchronize(sh.stream));
  if (const int rc = elapsed(st.prep_ms, b.ev[0], b.ev[1]); rc < 0) return rc;
  return 0;
}

int ecies_try_keys(Shard& sh, EciesBufs& b, uint32_t n, uint32_t n_set, size_t n_keys, bool want_key_e,
                   bmpow_ecies_stats& st) {
  if (n == 0) return 0;
  const uint32_t stride = (n_set + EC_BLOCK - 1) / EC_BLOCK * EC_BLOCK;
  const uint32_t kc = (uint32_t)std::max<size_t>(1, std::min<size_t>(n_keys, kLaunchPairs / stride));  // as staged
  for (size_t k0 = 0; k0 < n_keys; k0 += kc) {
    if (g_abort.load()) return set_err(BMPOW_E_ABORTED, "aborted");
    const uint32_t nk = (uint32_t)std::min<size_t>(kc, n_keys - k0);
    HIPTRY(hipEventRecord(b.ev[0].get(), sh.stream));
    HIPTRY(ec_launch_keys(sh.stream, b.tab.get(), n, stride, b.dig.get() + k0 * EC_DIGITS, nk, b.kout.get()));
    HIPTRY(hipEventRecord(b.ev[1].get(), sh.stream));
    HIPTRY(ec_launch_mac(sh.stream, b.kout.get(), n, stride, nk, b.objs.get(), b.pool.get(), b.ok.get(), (int)k0,
                         b.match.get()));
    if (want_key_e)
      HIPTRY(ec_launch_gather(sh.stream, b.kout.get(), n, stride, nk, (int)k0, b.match.get(), b.key_e.get()));
    HIPTRY(hipEventRecord(b.ev[2].get(), sh.stream));
    HIPTRY(hipStreamSynchronize(sh.stream));
    if (const int rc = elapsed(st.ecdh_ms, b.ev[0], b.ev[1]); rc < 0) return rc;
    if (const int rc = elapsed(st.mac_ms, b.ev[1], b.ev[2]); rc < 0) return rc;
    st.launches++;
    st.pairs += (uint64_t)n * nk;
  }
  return 0;
}

int ecies_match_locked(size_t n_obj, const uint8_t* const* payloads, const uint64_t* lens, size_t n_keys,
                       const uint8_t* privkeys, int32_t* match, uint8_t* key_e_out) {
  const auto t_begin = std::chrono::steady_clock::now();
  std::vector<int32_t> dig(n_keys * EC_DIGITS);
  for (size_t k = 0; k < n_keys; ++k) {
    const U256 key = u256_from_be(privkeys + 32 * k);
    if (!key_in_range(key)) return set_err(BMPOW_E_ARG, "private key is zero or not below the group order");
    recode_key(key, dig.data() + k * EC_DIGITS);
  }
  std::vector<Item> items;
  items.reserve(n_obj);
  for (size_t i = 0; i < n_obj; ++i) {
    if (lens[i] && !payloads[i]) return set_err(BMPOW_E_ARG, "null payload pointer");
    Item it;
    if (!ecies_parse(payloads[i], lens[i], it.hdr)) continue;
    if (lens[i] - 32 > (1ull << 31)) return set_err(BMPOW_E_ARG, "payload above 2^31 bytes");
    it.orig = (uint32_t)i;
    it.nblk = mac_blocks(lens[i] - 32);
    items.push_back(it);
  }
  std::stable_sort(items.begin(), items.end(), [](const Item& a, const Item& b) { return a.nblk > b.nblk; });
  if (items.empty()) return 0;

  Shard& sh = g_shards[0];
  HIPTRY(hipSetDevice(sh.dev));
  EciesBufs b;
  if (const int rc = ecies_events(b, sh.dev); rc < 0) return rc;
  HIPTRY(b.dig.alloc(sh.dev, dig.size()));
  HIPTRY(hipMemcpyAsync(b.dig.get(), dig.data(), dig.size() * sizeof(int32_t), hipMemcpyHostToDevice, sh.stream));
  g_ecies_stats.calls++;

  EciesStage h;
  std::vector<uint64_t> hkeye;
  size_t i0 = 0;
  while (i0 < items.size()) {
    uint64_t blocks = 0;
    const size_t i1 = ecies_set_end(items, i0, blocks);
    const uint32_t n = (uint32_t)(i1 - i0);
    if (const int rc = ecies_match_set(sh, b, h, items.data() + i0, n, blocks, payloads, lens, n_keys, key_e_out != nullptr,
                                       g_ecies_stats);
        rc < 0)
      return rc;
    if (key_e_out) {
      hkeye.resize((size_t)4 * n);
      HIPTRY(hipMemcpyAsync(hkeye.data(), b.key_e.get(), hkeye.size() * sizeof(uint64_t), hipMemcpyDeviceToHost,
                            sh.stream));
    }
    HIPTRY(hipStreamSynchronize(sh.stream));
    for (uint32_t j = 0; j < n; ++j) {
      const int m = h.match[j];
      if (m < 0 || (size_t)m >= n_keys) continue;
      const uint32_t orig = items[i0 + j].orig;
      match[orig] = m;
      if (key_e_out)
        for (int w = 0; w < 4; ++w)
          for (int q = 0; q < 8; ++q) key_e_out[32 * (size_t)orig + 8 * w + q] = (uint8_t)(hkeye[4 * (size_t)j + w] >> (56 - 8 * q));
    }
    g_ecies_stats.objects += n;
    i0 = i1;
  }
  g_ecies_stats.host_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
  return 0;
}

int ecdh_locked(size_t n_all, const uint8_t* priv, const uint8_t* pub, uint8_t* x_out, uint8_t* ok_out) {
  Shard& sh = g_shards[0];
  HIPTRY(hipSetDevice(sh.dev));
  EciesBufs b;
  std::vector<ec::ge> pts;
  std::vector<int32_t> dig;
  std::vector<uint32_t> ok;
  std::vector<uint8_t> host_ok;
  std::vector<ec::fe> xs;
  for (size_t i0 = 0; i0 < n_all; i0 += kSetObjects) {
    if (g_abort.load()) return set_err(BMPOW_E_ABORTED, "aborted");
    const uint32_t n = (uint32_t)std::min(kSetObjects, n_all - i0), stride = (n + EC_BLOCK - 1) / EC_BLOCK * EC_BLOCK;
    pts.assign(n, ec::ge{});
    dig.resize((size_t)n * EC_DIGITS);
    host_ok.assign(n, 1);
    for (uint32_t j = 0; j < n; ++j) {
      const U256 k = u256_from_be(priv + 32 * (i0 + j));
      const U256 x = u256_from_be(pub + 64 * (i0 + j)), y = u256_from_be(pub + 64 * (i0 + j) + 32);
      host_ok[j] = key_in_range(k) && u256_less(x, kPrime) && u256_less(y, kPrime);
      // a refused pair still runs, on a point the device's curve check refuses as well or with the key 1
      recode_key(key_in_range(k) ? k : U256{{1, 0, 0, 0}}, dig.data() + (size_t)j * EC_DIGITS);
      if (u256_less(x, kPrime) && u256_less(y, kPrime)) {
        pts[j].x = fe_from_u256(x);
        pts[j].y = fe_from_u256(y);
      }
    }
    HIPTRY(b.pts.grow(sh.dev, stride));
    HIPTRY(b.tab.grow(sh.dev, (size_t)EC_ENTRIES * stride));
    HIPTRY(b.ok.grow(sh.dev, stride));
    HIPTRY(b.dig.grow(sh.dev, (size_t)stride * EC_DIGITS));
    HIPTRY(b.x.grow(sh.dev, stride));
    HIPTRY(hipMemcpyAsync(b.pts.get(), pts.data(), n * sizeof(ec::ge), hipMemcpyHostToDevice, sh.stream));
    HIPTRY(hipMemcpyAsync(b.dig.get(), dig.data(), dig.size() * sizeof(int32_t), hipMemcpyHostToDevice, sh.stream));
    HIPTRY(ec_launch_prep(sh.stream, b.pts.get(), n, stride, b.tab.get(), b.ok.get()));
    HIPTRY(ec_launch_raw(sh.stream, b.tab.get(), n, stride, b.dig.get(), b.x.get(), b.ok.get()));
    ok.resize(n);
    xs.resize(n);
    HIPTRY(hipMemcpyAsync(ok.data(), b.ok.get(), n * sizeof(uint32_t), hipMemcpyDeviceToHost, sh.stream));
    HIPTRY(hipMemcpyAsync(xs.data(), b.x.get(), n * sizeof(ec::fe), hipMemcpyDeviceToHost, sh.stream));
    HIPTRY(hipStreamSynchronize(sh.stream));
    for (uint32_t j = 0; j < n; ++j) {
      const bool good = host_ok[j] && ok[j];
      ok_out[i0 + j] = good ? 1 : 0;
      uint8_t* out = x_out + 32 * (i0 + j);
      if (!good) {
        std::memset(out, 0, 32);
        continue;
      }
      for (int w = 0; w < 8; ++w)
        for (int q = 0; q < 4; ++q) out[4 * w + q] = (uint8_t)(xs[j].d[7 - w] >> (24 - 8 * q));
    }
  }
  return 0;
}

}  // namespace bmhost

using namespace bmhost;

extern "C" {

int bmpow_ecdh(size_t n, const uint8_t* priv, const uint8_t* pub, uint8_t* x_out, uint8_t* ok) {
  std::lock_guard<FairMutex> lk(g_mu);
  int rc = init_locked();
  if (rc < 0) return rc;
  if (n == 0) return 0;
  if (!priv || !pub || !x_out || !ok) return set_err(BMPOW_E_ARG, "null pointer");
  return ecdh_locked(n, priv, pub, x_out, ok);
}

int bmpow_ecies_parse(const uint8_t* payload, size_t len, uint8_t xy_out[64], size_t* body_off) {
  if ((len && !payload) || !xy_out || !body_off) return set_err(BMPOW_E_ARG, "null pointer");
  Parsed p;
  if (!ecies_parse(payload, len, p)) return 0;
  u256_to_be(p.x, xy_out);
  u256_to_be(p.y, xy_out + 32);
  *body_off = p.body_off;
  return 1;
}

int bmpow_ecies_match(size_t n_obj, const uint8_t* const* payloads, const uint64_t* lens, size_t n_keys,
                      const uint8_t* privkeys, int32_t* match, uint8_t* key_e_out) {
  std::lock_guard<FairMutex> lk(g_mu);
  if (n_obj && (!payloads || !lens || !match)) return set_err(BMPOW_E_ARG, "null pointer");
  if (n_keys && !privkeys) return set_err(BMPOW_E_ARG, "null pointer");
  if (n_obj > 0xffffffffull || n_keys > 0x7fffffffull) return set_err(BMPOW_E_ARG, "too many objects or keys");
  for (size_t i = 0; i < n_obj; ++i) match[i] = -1;
  if (key_e_out) std::memset(key_e_out, 0, 32 * n_obj);
  if (n_obj == 0 || n_keys == 0) return 0;
  const int rc = init_locked();
  if (rc < 0) return rc;
  return ecies_match_locked(n_obj, payloads, lens, n_keys, privkeys, match, key_e_out);
}

int64_t bmpow_ecies_decrypt(const uint8_t* payload, size_t len, const uint8_t key_e[32], uint8_t* out, size_t out_cap) {
  if ((len && !payload) || !key_e || !out) return set_err(BMPOW_E_ARG, "null pointer");
  Parsed p;
  if (!ecies_parse(payload, len, p)) return set_err(BMPOW_E_ARG, "malformed payload");
  const size_t clen = len - 32 - p.body_off;
  if (clen == 0 || clen % 16) return set_err(BMPOW_E_ARG, "ciphertext is empty or no multiple of the block size");
  if (clen > 0x7fffffff) return set_err(BMPOW_E_ARG, "ciphertext above 2^31 bytes");
  if (out_cap < clen) return set_err(BMPOW_E_ARG, "output buffer smaller than the ciphertext");
  EVP_CIPHER_CTX* ctx = EVP_CIPHER_CTX_new();
  if (!ctx) return set_err(BMPOW_E_ARG, "EVP_CIPHER_CTX_new failed");
  std::vector<uint8_t> tmp(clen + 16);
  int n1 = 0, n2 = 0;
  const bool good = EVP_DecryptInit_ex(ctx, EVP_aes_256_cbc(), nullptr, key_e, payload) == 1 &&
                    EVP_DecryptUpdate(ctx, tmp.data(), &n1, payload + p.body_off, (int)clen) == 1 &&
                    EVP_DecryptFinal_ex(ctx, tmp.data() + n1, &n2) == 1;
  EVP_CIPHER_CTX_free(ctx);
  if (!good) return set_err(BMPOW_E_ARG, "bad padding");
  std::memcpy(out, tmp.data(), (size_t)(n1 + n2));
  return n1 + n2;
}

int bmpow_ecies_get_stats(bmpow_ecies_stats* out) {
  std::lock_guard<FairMutex> lk(g_mu);
  if (!out) return set_err(BMPOW_E_ARG, "null pointer");
  *out = g_ecies_stats;
  return 0;
}

void bmpow_ecies_reset_stats(void) {
  std::lock_guard<FairMutex> lk(g_mu);
  g_ecies_stats = bmpow_ecies_stats{};
}

}  // extern "C"
