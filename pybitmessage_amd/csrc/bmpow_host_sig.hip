// bmpow_host_sig.hip -- the signature verification's host side: the padded message pool and the
// bmpow_sig_* / bmpow_ecdsa_verify_digest entry points (include/bmpow_sig.h); the strict DER parser and the
// range checks are bmpow_host_scalar.h's.
#include "bmpow_host.h"

#include "../../include/bmpow_sig.h"
#include "bmpow_host_scalar.h"
#include "bmpow_host_sig.h"

// ---------------------------------------------------------------------------------------
// One call: the signatures that parse and whose key coordinates are below p, sorted by their message's
// block count (descending, so a wave's 64 lanes hash alike), go through the device in sets of at most
// kSigSetObjects signatures and kSigSetPoolBytes of padded blocks.  Per set: upload, then the phases
// one launch each -- hash, scalars, key tables (ec_prep_kernel), ladder, combs -- with the abort flag
// read between sets.  The buffers are the call's own (DevBuf owners, released when it returns);
// everything runs on the first shard's device and stream.
// ---------------------------------------------------------------------------------------
namespace bmhost {

int SigBufs::grow(Shard& sh, uint32_t stride, uint64_t pool_chunks) {
  HIPTRY(sigs.grow(sh.dev, stride));
  HIPTRY(pool.grow(sh.dev, pool_chunks));
  HIPTRY(e.grow(sh.dev, (size_t)2 * stride));
  HIPTRY(u1.grow(sh.dev, (size_t)2 * stride));
  HIPTRY(dig.grow(sh.dev, (size_t)SG_DIGITS * stride));
  HIPTRY(flip.grow(sh.dev, stride));
  HIPTRY(tinf.grow(sh.dev, stride));
  HIPTRY(verdict.grow(sh.dev, stride));
  HIPTRY(pts.grow(sh.dev, stride));
  HIPTRY(tab.grow(sh.dev, (size_t)EC_ENTRIES * stride));
  HIPTRY(ok.grow(sh.dev, stride));
  HIPTRY(T.grow(sh.dev, stride));
  return 0;
}

int sig_launch_verify(Shard& sh, SigBufs& b, const ec::ge* comb, uint32_t n, uint32_t stride, int nhash, const Event& mid) {
  HIPTRY(sg_launch_scalars(sh.stream, b.sigs.get(), b.e.get(), n, stride, nhash, b.u1.get(), b.dig.get(), b.flip.get()));
  HIPTRY(hipEventRecord(mid.get(), sh.stream));
  HIPTRY(ec_launch_prep(sh.stream, b.pts.get(), n, stride, b.tab.get(), b.ok.get()));
  HIPTRY(sg_launch_ladder(sh.stream, b.tab.get(), n, stride, b.dig.get(), b.flip.get(), b.T.get(), b.tinf.get()));
  HIPTRY(sg_launch_comb(sh.stream, comb, b.sigs.get(), b.u1.get(), b.T.get(), b.tinf.get(), b.ok.get(), n, stride, nhash,
                        b.verdict.get()));
  return 0;
}

namespace {

using sn::sc;

ec::fe fe_from_sc(const sc& a) {
  ec::fe f;
  for (int i = 0; i < 8; ++i) f.d[i] = a.d[i];
  return f;
}

bmpow_sig_stats g_sig_stats{};  // under g_mu

struct SigItem {  // a signature that goes to the device
  uint32_t orig;
  uint32_t nblk;  // 0: the digest is given
  sc r, s, x, y;
};

// msgs / msg_lens: the messages (nhash == 2), or null with digests[32 i ..] given (nhash == 1)
int sig_run_locked(std::vector<SigItem>& items, int nhash, const uint8_t* const* msgs, const uint64_t* msg_lens,
                   const uint8_t* digests, uint8_t* verdict) {
  std::stable_sort(items.begin(), items.end(), [](const SigItem& a, const SigItem& b) { return a.nblk > b.nblk; });
  Shard& sh = g_shards[0];
  HIPTRY(hipSetDevice(sh.dev));
  const ec::ge* comb = nullptr;
  if (const int rc = addr_comb16_table(sh, &comb); rc < 0) return rc;
  SigBufs b;
  for (Event& e : b.ev) HIPTRY(e.alloc(sh.dev));
  g_sig_stats.calls++;

  std::vector<sg_sig> sigs;
  std::vector<ec::ge> pts;
  std::vector<sc> e;
  std::vector<uint8_t> pool, out;
  size_t i0 = 0;
  while (i0 < items.size()) {
    if (g_abort.load()) return set_err(BMPOW_E_ABORTED, "aborted");
    const auto [i1, blocks] =
        plan_set(items, i0, [](const SigItem& it) { return it.nblk; }, kSigSetObjects, kSigSetPoolBytes);
    if (blocks > 0xffffffffull) return set_err(BMPOW_E_ARG, "message pool above 2^32 blocks");
    const uint32_t n = (uint32_t)(i1 - i0), stride = (n + SG_BLOCK - 1) / SG_BLOCK * SG_BLOCK;
    sigs.resize(n);
    pts.resize(n);
    pool.resize(blocks * 64);
    uint32_t blk = 0;
    for (uint32_t j = 0; j < n; ++j) {
      const SigItem& it = items[i0 + j];
      sigs[j].r = it.r;
      sigs[j].s = it.s;
      sigs[j].blk = blk;
      sigs[j].nblk = it.nblk;
      blk += it.nblk;
      pts[j].x = fe_from_sc(it.x);
      pts[j].y = fe_from_sc(it.y);
    }
    if (nhash == 2) {
      bmsched::parallel_for(n, 1024, [&](size_t a, size_t z) {
        for (size_t j = a; j < z; ++j) {
          const SigItem& it = items[i0 + j];
          pad_blocks(msgs[it.orig], msg_lens[it.orig], pool.data() + (size_t)sigs[j].blk * 64, it.nblk);
        }
      });
    } else {
      e.resize(n);
      for (uint32_t j = 0; j < n; ++j) e[j] = sc_from_be(digests + 32 * (size_t)items[i0 + j].orig);
    }
    if (const int rc = b.grow(sh, stride, std::max<size_t>(pool.size(), 64) / sizeof(uint4)); rc < 0) return rc;
    HIPTRY(hipMemcpyAsync(b.sigs.get(), sigs.data(), n * sizeof(sg_sig), hipMemcpyHostToDevice, sh.stream));
    HIPTRY(hipMemcpyAsync(b.pts.get(), pts.data(), n * sizeof(ec::ge), hipMemcpyHostToDevice, sh.stream));
    if (nhash == 2) {
      if (!pool.empty())
        HIPTRY(hipMemcpyAsync(b.pool.get(), pool.data(), pool.size(), hipMemcpyHostToDevice, sh.stream));
    } else {
      HIPTRY(hipMemcpyAsync(b.e.get(), e.data(), n * sizeof(sc), hipMemcpyHostToDevice, sh.stream));
    }
    HIPTRY(hipEventRecord(b.ev[0].get(), sh.stream));
    if (nhash == 2) HIPTRY(sg_launch_hash(sh.stream, b.sigs.get(), b.pool.get(), n, stride, b.e.get()));
    HIPTRY(hipEventRecord(b.ev[1].get(), sh.stream));
    if (const int rc = sig_launch_verify(sh, b, comb, n, stride, nhash, b.ev[2]); rc < 0) return rc;
    HIPTRY(hipEventRecord(b.ev[3].get(), sh.stream));
    out.resize(n);
    HIPTRY(hipMemcpyAsync(out.data(), b.verdict.get(), n, hipMemcpyDeviceToHost, sh.stream));
    HIPTRY(hipStreamSynchronize(sh.stream));
    double* const acc[3] = {&g_sig_stats.hash_ms, &g_sig_stats.scalar_ms, &g_sig_stats.curve_ms};
    if (const int rc = elapsed_phases(acc, b.ev, 3); rc < 0) return rc;
    for (uint32_t j = 0; j < n; ++j) verdict[items[i0 + j].orig] = out[j] <= (uint8_t)nhash ? out[j] : 0;
    g_sig_stats.uploaded += n;
    g_sig_stats.ladders += n;
    g_sig_stats.launches += nhash == 2 ? 5 : 4;
    i0 = i1;
  }
  return 0;
}

// the key's coordinates into it.x, it.y; false for one that is not below p
bool take_key(const uint8_t* pub, SigItem& it) {
  it.x = sc_from_be(pub);
  it.y = sc_from_be(pub + 32);
  return coord_in_range(it.x) && coord_in_range(it.y);
}

}  // namespace
}  // namespace bmhost

using namespace bmhost;

extern "C" {

int bmpow_sig_parse(const uint8_t* sig, size_t len, uint8_t rs_out[64]) {
  if ((len && !sig) || !rs_out) return set_err(BMPOW_E_ARG, "null pointer");
  return sig_parse(sig, len, rs_out) ? 1 : 0;
}

int bmpow_ecdsa_verify_digest(size_t n, const uint8_t* pub, const uint8_t* rs, const uint8_t* e, uint8_t* ok) {
  std::lock_guard<FairMutex> lk(g_mu);
  if (n == 0) return 0;
  if (!pub || !rs || !e || !ok) return set_err(BMPOW_E_ARG, "null pointer");
  if (n > 0xffffffffull) return set_err(BMPOW_E_ARG, "too many signatures");
  const auto t_begin = std::chrono::steady_clock::now();
  std::memset(ok, 0, n);
  std::vector<SigItem> items;
  items.reserve(n);
  for (size_t i = 0; i < n; ++i) {
    SigItem it;
    it.orig = (uint32_t)i;
    it.nblk = 0;
    it.r = sc_from_be(rs + 64 * i);
    it.s = sc_from_be(rs + 64 * i + 32);
    if (!scalar_in_range(it.r) || !scalar_in_range(it.s) || !take_key(pub + 64 * i, it)) continue;
    items.push_back(it);
  }
  int rc = 0;
  if (!items.empty()) {
    rc = init_locked();
    if (rc >= 0) rc = sig_run_locked(items, 1, nullptr, nullptr, e, ok);
    if (rc > 0) rc = 0;
  }
  g_sig_stats.submitted += n;
  g_sig_stats.host_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
  return rc;
}

int bmpow_sig_verify(size_t n, const uint8_t* const* msgs, const uint64_t* msg_lens, const uint8_t* const* sigs,
                     const uint64_t* sig_lens, const uint8_t* pubkeys, uint8_t* verdict) {
  std::lock_guard<FairMutex> lk(g_mu);
  if (n == 0) return 0;
  if (!msgs || !msg_lens || !sigs || !sig_lens || !pubkeys || !verdict) return set_err(BMPOW_E_ARG, "null pointer");
  if (n > 0xffffffffull) return set_err(BMPOW_E_ARG, "too many signatures");
  const auto t_begin = std::chrono::steady_clock::now();
  std::memset(verdict, 0, n);
  std::vector<SigItem> items;
  items.reserve(n);
  for (size_t i = 0; i < n; ++i) {
    if ((msg_lens[i] && !msgs[i]) || (sig_lens[i] && !sigs[i])) return set_err(BMPOW_E_ARG, "null message or signature pointer");
    if (msg_lens[i] > (1ull << 31)) return set_err(BMPOW_E_ARG, "message above 2^31 bytes");
    SigItem it;
    uint8_t rs[64];
    if (!sig_parse(sigs[i], sig_lens[i], rs) || !take_key(pubkeys + 64 * i, it)) continue;
    it.orig = (uint32_t)i;
    it.nblk = msg_blocks(msg_lens[i]);
    it.r = sc_from_be(rs);
    it.s = sc_from_be(rs + 32);
    items.push_back(it);
  }
  int rc = 0;
  if (!items.empty()) {
    rc = init_locked();
    if (rc >= 0) rc = sig_run_locked(items, 2, msgs, msg_lens, nullptr, verdict);
    if (rc > 0) rc = 0;
  }
  g_sig_stats.submitted += n;
  g_sig_stats.host_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
  return rc;
}

int bmpow_sig_get_stats(bmpow_sig_stats* out) {
  std::lock_guard<FairMutex> lk(g_mu);
  if (!out) return set_err(BMPOW_E_ARG, "null pointer");
  *out = g_sig_stats;
  return 0;
}

void bmpow_sig_reset_stats(void) {
  std::lock_guard<FairMutex> lk(g_mu);
  g_sig_stats = bmpow_sig_stats{};
}

}  // extern "C"
