// bmpow_host_addr.hip -- the address search's host side: comb tables, addr_search_locked, and the
// bmpow_pubkeys, bmpow_fe_probe, bmpow_address_search*, bmpow_addr_* entry points.
#include "bmpow_host.h"

// ---------------------------------------------------------------------------------------
// RIPE-prefix address search (bmpow_addr.hip).  Steps cover contiguous ranges of try indices
// [next, next + S*step), one slice per shard; a hit is reported only after the step that
// covers every smaller try has completed, so the answer is the first k, as the reference's
// sequential loop finds it.  Step sizes ramp up from about the expected number of tries
// (256^null_bytes) so a 1-byte search costs one small launch.
// ---------------------------------------------------------------------------------------
namespace bmhost {

using bmsched::load_be64;

constexpr uint64_t kAddrMaxStep = 1ULL << 22;  // tries per shard per launch (~10 ms)

// The fixed-base comb tables (v * 2^(W i) * G), built on first use: one entry per physical device, which
// the shards of that device share, released with the shard set (addr_release_shards).  The allocation
// holds ec::kWindows extra entries: ar_launch_table's base points.
// c = 0: the 16-bit comb (64 MB), c = 1: the 24-bit comb (10.7 GB).
constexpr int kCombBits[2] = {ec::kCombSmall, ec::kCombLarge};
struct CombTables {
  int dev;
  DevBuf<ec::ge> t[2];
};
std::vector<CombTables> g_comb;

void addr_release_shards() { g_comb.clear(); }

// The device's table c, or null while it is not built.
ec::ge* comb_table(int dev, int c) {
  for (const CombTables& ct : g_comb)
    if (ct.dev == dev) return ct.t[c].get();
  return nullptr;
}

int ensure_table(Shard& sh, int c = 0) {
  if (comb_table(sh.dev, c)) return 0;
  auto it = std::find_if(g_comb.begin(), g_comb.end(), [&](const CombTables& ct) { return ct.dev == sh.dev; });
  if (it == g_comb.end()) it = g_comb.insert(it, CombTables{sh.dev, {}});
  const size_t n = ar_table_entries(kCombBits[c]);
  const hipError_t e = it->t[c].alloc(sh.dev, n);
  if (e != hipSuccess) {
    (void)hipGetLastError();  // an out-of-memory here is reported, not sticky
    return set_err(BMPOW_E_HIP, std::string("comb table allocation: ") + hipGetErrorString(e));
  }
  ec::ge* const t = it->t[c].get();
  HIPTRY(hipMemsetAsync(t, 0, n * sizeof(ec::ge), sh.stream));
  HIPTRY(ar_launch_table(sh.stream, t, kCombBits[c]));
  HIPTRY(hipStreamSynchronize(sh.stream));
  return 0;
}

int addr_comb16_table(Shard& sh, const ec::ge** table) {
  const int rc = ensure_table(sh, 0);
  if (rc < 0) return rc;
  *table = comb_table(sh.dev, 0);
  return 0;
}

// Comb choice for one search: the 24-bit comb when forced (bmpow_addr_set_comb(24)), or in auto
// mode when it is already built on every shard or the search is expected to take >= 2^32 tries
// (4+ null bytes: seconds of work, against ~0.4 s to build the table once per device; judged from
// null_bytes alone, since callers cut long searches into bounded calls); else the 16-bit one.  An
// auto-mode allocation failure falls back to the small comb.
int g_addr_comb = 0;       // 0 auto, 16, 24
int g_addr_last_comb = 0;  // width used by the last search

int addr_pick_comb(int null_bytes) {
  if (g_addr_comb == ec::kCombSmall) return 0;
  bool built = true;
  for (const Shard& sh : g_shards) built = built && comb_table(sh.dev, 1) != nullptr;
  const uint64_t expected = null_bytes >= 8 ? kU64Max : (1ULL << (8 * null_bytes));
  const bool want = g_addr_comb == ec::kCombLarge || built || expected >= (1ULL << 32);
  if (!want) return 0;
  for (Shard& sh : g_shards) {
    const int rc = ensure_table(sh, 1);
    if (rc < 0) {
      if (g_addr_comb == ec::kCombLarge) return rc;
      return 0;
    }
  }
  return 1;
}

void be_words_from_bytes(const uint8_t* b, uint64_t (&w)[4]) {
  for (int i = 0; i < 4; ++i) w[i] = load_be64(b + 8 * i);
}

void bytes_from_be_words(const uint64_t* w, int n, uint8_t* out) {
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < 8; ++j) out[8 * i + j] = (uint8_t)(w[i] >> (56 - 8 * j));
}

void point_bytes(const ec::ge& p, uint8_t* out) {  // 04 || X || Y, big-endian
  out[0] = 0x04;
  for (int i = 0; i < 8; ++i)
    for (int j = 0; j < 4; ++j) {
      out[1 + 4 * i + j] = (uint8_t)(p.x.d[7 - i] >> (24 - 8 * j));
      out[33 + 4 * i + j] = (uint8_t)(p.y.d[7 - i] >> (24 - 8 * j));
    }
}

struct AddrShard {  // one search's buffers on a shard: released when the search returns
  DevBuf<ar_params> d_prm;
  DevBuf<uint8_t> d_seed;
  DevBuf<unsigned long long> d_best;
  DevBuf<ar_result> d_res;
  DevBuf<uint64_t> d_priv;
  DevBuf<uint32_t> d_ok;
};

int addr_search_locked(uint32_t mode, const uint8_t* seed, size_t len, const uint8_t* priv_s, uint64_t start,
                       uint64_t max_tries, int null_bytes, bmpow_address* out) {
  if (null_bytes < 0 || null_bytes > 20) return set_err(BMPOW_E_ARG, "null_bytes must be in [0, 20]");
  if (!out || (len && !seed) || (mode == 1 && !priv_s)) return set_err(BMPOW_E_ARG, "null pointer");
  if (max_tries == 0) return BMPOW_NOT_FOUND;
  if (mode == 0 && start > (kU64Max >> 1)) return set_err(BMPOW_E_ARG, "try index above 2^63 (nonce 2k overflows)");
  ar_params hp;
  std::memset(&hp, 0, sizeof hp);
  hp.total_len = len;
  hp.tail_len = (uint32_t)(len % 128);
  hp.null_bytes = (uint32_t)null_bytes;
  hp.mode = mode;
  const uint64_t nfull = len / 128;
  for (uint32_t i = 0; i < hp.tail_len; ++i) {
    const uint64_t byte = seed[nfull * 128 + i];
    hp.tmpl[i >> 3] |= byte << (56 - 8 * (i & 7));
  }
  uint64_t pw[4] = {0, 0, 0, 0};
  if (mode == 1) be_words_from_bytes(priv_s, pw);
  const size_t S = g_shards.size();
  std::vector<AddrShard> as(S);
  for (size_t s = 0; s < S; ++s) {
    Shard& sh = g_shards[s];
    int rc = ensure_table(sh, 0);
    if (rc < 0) return rc;
    AddrShard& a = as[s];
    HIPTRY(a.d_prm.alloc(sh.dev, 1));
    HIPTRY(a.d_seed.alloc(sh.dev, std::max<size_t>(len, 1)));
    HIPTRY(a.d_best.alloc(sh.dev, 1));
    HIPTRY(a.d_res.alloc(sh.dev, 1));
    HIPTRY(a.d_priv.alloc(sh.dev, 4));
    HIPTRY(a.d_ok.alloc(sh.dev, 1));
    HIPTRY(hipMemcpyAsync(a.d_prm.get(), &hp, sizeof hp, hipMemcpyHostToDevice, sh.stream));
    if (len) HIPTRY(hipMemcpyAsync(a.d_seed.get(), seed, len, hipMemcpyHostToDevice, sh.stream));
    HIPTRY(hipMemsetAsync(a.d_best.get(), 0xFF, sizeof(unsigned long long), sh.stream));
    HIPTRY(ar_launch_midstate(sh.stream, a.d_seed.get(), nfull, (uint64_t*)a.d_prm.get()));  // mid[] is at offset 0
    if (mode == 1) {
      HIPTRY(hipMemcpyAsync(a.d_priv.get(), pw, sizeof pw, hipMemcpyHostToDevice, sh.stream));
      HIPTRY(ar_launch_pubkeys(sh.stream, a.d_priv.get(), 1, comb_table(sh.dev, 0), &a.d_prm.get()->pub_s, a.d_ok.get()));
    }
  }
  if (const int rc = sync_shards(); rc < 0) return rc;
  if (mode == 1) {
    uint32_t ok = 0;
    HIPTRY(hipSetDevice(g_shards[0].dev));
    HIPTRY(hipMemcpy(&ok, as[0].d_ok.get(), sizeof ok, hipMemcpyDeviceToHost));
    if (!ok) return set_err(BMPOW_E_ARG, "signing private key is zero");
  }
  uint64_t end = (kU64Max - start < max_tries) ? kU64Max : start + max_tries;
  // mode 0: k = 2^63 - 1 is the last try there is (its nonce 2k + 1 = 2^64 - 1 is the last a varint
  // holds); a lane above it would derive its keys from the wrapped nonce
  if (mode == 0) end = std::min<uint64_t>(end, 1ULL << 63);
  const int comb = addr_pick_comb(null_bytes);
  if (comb < 0) return comb;
  g_addr_last_comb = kCombBits[comb];
  uint64_t step = 4096;
  for (int b = 0; b < null_bytes && step < kAddrMaxStep; ++b) step = std::min<uint64_t>(step * 256, kAddrMaxStep);
  step = std::max<uint64_t>(step / 4, 4096);
  uint64_t next = start;
  while (next < end) {
    if (g_abort.load()) return set_err(BMPOW_E_ABORTED, "aborted");
    uint64_t lo[64], cnt[64];
    for (size_t s = 0; s < S && s < 64; ++s) {
      lo[s] = next + s * step;
      cnt[s] = lo[s] >= end ? 0 : std::min<uint64_t>(step, end - lo[s]);
      if (lo[s] < next) cnt[s] = 0;  // wrapped
      Shard& sh = g_shards[s];
      HIPTRY(hipSetDevice(sh.dev));
      HIPTRY(hipEventRecord(sh.ev0.get(), sh.stream));
      HIPTRY(ar_launch_search(sh.stream, as[s].d_prm.get(), mode, comb_table(sh.dev, comb), kCombBits[comb], lo[s],
                              (uint32_t)cnt[s], as[s].d_best.get()));
      HIPTRY(hipEventRecord(sh.ev1.get(), sh.stream));
    }
    uint64_t best = kU64Max;
    size_t best_s = 0;
    double mx = 0;
    for (size_t s = 0; s < S && s < 64; ++s) {
      Shard& sh = g_shards[s];
      HIPTRY(hipSetDevice(sh.dev));
      HIPTRY(hipStreamSynchronize(sh.stream));
      float ms = 0;
      HIPTRY(hipEventElapsedTime(&ms, sh.ev0.get(), sh.ev1.get()));
      mx = std::max<double>(mx, ms);
      unsigned long long b = 0;
      HIPTRY(hipMemcpy(&b, as[s].d_best.get(), sizeof b, hipMemcpyDeviceToHost));
      g_stats.addr_tries += cnt[s];
      if (b < best) {
        best = b;
        best_s = s;
      }
    }
    g_stats.addr_kernel_ms += mx;
    g_stats.addr_launches++;
    if (best != kU64Max) {
      Shard& sh = g_shards[best_s];
      HIPTRY(hipSetDevice(sh.dev));
      HIPTRY(ar_launch_resolve(sh.stream, as[best_s].d_prm.get(), comb_table(sh.dev, comb), kCombBits[comb], best,
                               as[best_s].d_res.get()));
      ar_result r;
      HIPTRY(hipMemcpyAsync(&r, as[best_s].d_res.get(), sizeof r, hipMemcpyDeviceToHost, sh.stream));
      HIPTRY(hipStreamSynchronize(sh.stream));
      if (!r.ok) return set_err(BMPOW_E_HIP, "resolve of the found try failed");
      std::memset(out, 0, sizeof *out);
      out->k = r.k;
      for (int i = 0; i < 5; ++i)
        for (int j = 0; j < 4; ++j) out->ripe[4 * i + j] = (uint8_t)(r.ripe[i] >> (8 * j));
      if (mode == 0) bytes_from_be_words(r.priv_s, 4, out->priv_signing);
      else std::memcpy(out->priv_signing, priv_s, 32);
      bytes_from_be_words(r.priv_e, 4, out->priv_encryption);
      point_bytes(r.pub_s, out->pub_signing);
      point_bytes(r.pub_e, out->pub_encryption);
      return BMPOW_FOUND;
    }
    const uint64_t span = step * std::min<size_t>(S, 64);
    next = (kU64Max - next < span) ? end : next + span;
    step = std::min<uint64_t>(step * 2, kAddrMaxStep);
  }
  return BMPOW_NOT_FOUND;
}

}  // namespace bmhost

using namespace bmhost;

extern "C" {

int bmpow_pubkeys(size_t n, const uint8_t* privkeys, uint8_t* pubkeys_out) {
  std::lock_guard<FairMutex> lk(g_mu);
  int rc = init_locked();
  if (rc < 0) return rc;
  if (n == 0) return 0;
  if (!privkeys || !pubkeys_out) return set_err(BMPOW_E_ARG, "null pointer");
  if (n > 0xffffffffULL) return set_err(BMPOW_E_ARG, "too many keys");
  if (g_abort.load()) return set_err(BMPOW_E_ABORTED, "aborted");
  Shard& sh = g_shards[0];
  rc = ensure_table(sh, 0);
  if (rc < 0) return rc;
  std::vector<uint64_t> w(4 * n);
  for (size_t i = 0; i < n; ++i) {
    uint64_t k[4];
    be_words_from_bytes(privkeys + 32 * i, k);
    for (int j = 0; j < 4; ++j) w[4 * i + j] = k[j];
  }
  std::vector<ec::ge> pubs(n);
  std::vector<uint32_t> ok(n);
  DevBuf<uint64_t> d_w;  // the call's buffers: released when it returns
  DevBuf<ec::ge> d_p;
  DevBuf<uint32_t> d_ok;
  HIPTRY(hipSetDevice(sh.dev));
  hipError_t e = d_w.alloc(sh.dev, w.size());
  if (e == hipSuccess) e = d_p.alloc(sh.dev, n);
  if (e == hipSuccess) e = d_ok.alloc(sh.dev, n);
  if (e == hipSuccess) e = hipMemcpyAsync(d_w.get(), w.data(), w.size() * sizeof(uint64_t), hipMemcpyHostToDevice, sh.stream);
  if (e == hipSuccess) e = ar_launch_pubkeys(sh.stream, d_w.get(), (uint32_t)n, comb_table(sh.dev, 0), d_p.get(), d_ok.get());
  if (e == hipSuccess) e = hipMemcpyAsync(pubs.data(), d_p.get(), n * sizeof(ec::ge), hipMemcpyDeviceToHost, sh.stream);
  if (e == hipSuccess) e = hipMemcpyAsync(ok.data(), d_ok.get(), n * sizeof(uint32_t), hipMemcpyDeviceToHost, sh.stream);
  if (e == hipSuccess) e = hipStreamSynchronize(sh.stream);
  if (e != hipSuccess) return set_err(BMPOW_E_HIP, std::string("bmpow_pubkeys: ") + hipGetErrorString(e));
  for (size_t i = 0; i < n; ++i) {
    if (ok[i]) point_bytes(pubs[i], pubkeys_out + 65 * i);
    else std::memset(pubkeys_out + 65 * i, 0, 65);
  }
  return 0;
}

int bmpow_fe_probe(int op, size_t n, const uint32_t* a, const uint32_t* b, uint32_t* out) {
  std::lock_guard<FairMutex> lk(g_mu);
  int rc = init_locked();
  if (rc < 0) return rc;
  if (n == 0) return 0;
  if (!a || !b || !out) return set_err(BMPOW_E_ARG, "null pointer");
  if (op < 0 || op > 6) return set_err(BMPOW_E_ARG, "fe probe op must be 0..6");
  if (n > (1u << 24)) return set_err(BMPOW_E_ARG, "too many operands");
  Shard& sh = g_shards[0];
  const size_t bytes = n * sizeof(ec::fe);
  DevBuf<ec::fe> d_a, d_b, d_o;  // the call's buffers: released when it returns
  HIPTRY(hipSetDevice(sh.dev));
  hipError_t e = d_a.alloc(sh.dev, n);
  if (e == hipSuccess) e = d_b.alloc(sh.dev, n);
  if (e == hipSuccess) e = d_o.alloc(sh.dev, n);
  if (e == hipSuccess) e = hipMemcpyAsync(d_a.get(), a, bytes, hipMemcpyHostToDevice, sh.stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_b.get(), b, bytes, hipMemcpyHostToDevice, sh.stream);
  if (e == hipSuccess) e = ar_launch_fe_probe(sh.stream, op, d_a.get(), d_b.get(), d_o.get(), (uint32_t)n);
  if (e == hipSuccess) e = hipMemcpyAsync(out, d_o.get(), bytes, hipMemcpyDeviceToHost, sh.stream);
  if (e == hipSuccess) e = hipStreamSynchronize(sh.stream);
  if (e != hipSuccess) return set_err(BMPOW_E_HIP, std::string("bmpow_fe_probe: ") + hipGetErrorString(e));
  return 0;
}

int bmpow_address_search(const uint8_t* passphrase, size_t len, uint64_t start, uint64_t max_tries, int null_bytes,
                         bmpow_address* out) {
  std::lock_guard<FairMutex> lk(g_mu);
  int rc = init_locked();
  if (rc < 0) return rc;
  return addr_search_locked(0, passphrase, len, nullptr, start, max_tries, null_bytes, out);
}

int bmpow_address_search_random(const uint8_t priv_signing[32], const uint8_t* seed, size_t seed_len, uint64_t start,
                                uint64_t max_tries, int null_bytes, bmpow_address* out) {
  std::lock_guard<FairMutex> lk(g_mu);
  int rc = init_locked();
  if (rc < 0) return rc;
  return addr_search_locked(1, seed, seed_len, priv_signing, start, max_tries, null_bytes, out);
}

int bmpow_addr_set_comb(int wbits) {
  std::lock_guard<FairMutex> lk(g_mu);
  if (wbits != 0 && wbits != ec::kCombSmall && wbits != ec::kCombLarge)
    return set_err(BMPOW_E_ARG, "comb width must be 0 (auto), 16 or 24");
  const int prev = g_addr_comb;
  g_addr_comb = wbits;
  return prev;
}

int bmpow_addr_last_comb(void) {
  std::lock_guard<FairMutex> lk(g_mu);
  return g_addr_last_comb;
}

}  // extern "C"
