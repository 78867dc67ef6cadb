// bmpow_host_verify.hip -- receive-side verification: the sessions (bmpow_vbatch_*) and the one-shot
// entry points (bmpow_pow_values, bmpow_verify_batch*, bmpow_pow_sufficient).
#include "bmpow_host_vbatch.h"  // struct bmpow_vbatch; vbatch_build / vbatch_release_plan, shared with the intake

namespace bmhost {

using bmsched::Span;

constexpr uint64_t kVStageBytes = 64ull << 20;  // pinned staging chunk (x2 per shard)

// One-shot verification (bmpow_verify_batch*, bmpow_pow_values), per shard (indexed like g_shards):
// buffers kept across calls (grow-only), so a flood pays neither allocation nor first-touch page faults;
// two pinned staging chunks let the padding of chunk c+1 overlap the DMA of chunk c
struct VerifyShard {
  PinBuf<uint8_t> h_vstage[2];
  Event ev_vstage[2];
  DevBuf<uint4> d_vpool;
  DevBuf<bv_obj> d_vobj;
  DevBuf<uint64_t> d_vpow;
  PinBuf<uint64_t> h_vpow;  // pinned
  DevBuf<uint32_t> d_vbins;  // work bins of the binned verification kernel (grow-only)
};
std::vector<VerifyShard> g_verify;

void verify_release_shards() { g_verify.clear(); }

// One-shot path: the part's pool goes up through the shard's two pinned staging chunks, padding of
// chunk c+1 overlapping the DMA of chunk c; device buffers are the shard's, reused across calls.
int vbatch_upload_transient(bmpow_vbatch::Part& pt, const std::vector<Span>& objs) {
  const std::vector<bv_obj>& ho = pt.ho;
  Shard& sh = g_shards[pt.shard];
  if (g_verify.size() != g_shards.size()) g_verify.resize(g_shards.size());
  VerifyShard& vs = g_verify[pt.shard];
  const size_t m = pt.orig.size();
  if (m > vs.h_vpow.cap() || !vs.h_vpow) {  // allocated last of the three: its capacity is theirs
    vs.d_vobj.reset(), vs.d_vpow.reset(), vs.h_vpow.reset();
    const size_t cap = std::max<size_t>(m, 4096);
    HIPTRY(vs.d_vobj.alloc(sh.dev, cap));
    HIPTRY(vs.d_vpow.alloc(sh.dev, cap));
    HIPTRY(vs.h_vpow.alloc(sh.dev, cap, hipHostMallocDefault));
  }
  HIPTRY(vs.d_vpool.grow(sh.dev, std::max<size_t>(pt.blocks * 128, 16) / sizeof(uint4)));
  for (int c = 0; c < 2; ++c) {
    if (!vs.h_vstage[c]) HIPTRY(vs.h_vstage[c].alloc(sh.dev, kVStageBytes, hipHostMallocDefault));
    if (!vs.ev_vstage[c]) HIPTRY(vs.ev_vstage[c].alloc(sh.dev, hipEventDisableTiming));
  }
  pt.d_obj = vs.d_vobj.get();  // plain pointers into the shard's owners (pt.own stays empty)
  pt.d_pool = vs.d_vpool.get();
  pt.d_pow = vs.d_vpow.get();
  pt.h_pow = vs.h_vpow.get();
  // chunks of whole objects; an object larger than a chunk is padded in pageable memory on its own
  size_t j = 0;
  int c = 0;
  bool used[2] = {false, false};
  std::unique_ptr<uint8_t[]> big;
  while (j < m) {
    const uint64_t blk0 = ho[j].blk;
    size_t j1 = j;
    uint64_t bytes = 0;
    while (j1 < m && (j1 == j || bytes + (uint64_t)ho[j1].nblk * 128 <= kVStageBytes)) {
      bytes += (uint64_t)ho[j1].nblk * 128;
      ++j1;
    }
    uint8_t* dst;
    if (bytes > kVStageBytes) {
      big.reset(new uint8_t[bytes]);
      dst = big.get();
    } else {
      if (used[c]) HIPTRY(hipEventSynchronize(vs.ev_vstage[c].get()));  // its previous DMA is done
      dst = vs.h_vstage[c].get();
    }
    bmsched::pad_range(objs, pt, j, j1, blk0, dst);
    HIPTRY(hipMemcpyAsync((uint8_t*)pt.d_pool + blk0 * 128, dst, bytes, hipMemcpyHostToDevice, sh.stream));
    if (dst == big.get()) {
      HIPTRY(hipStreamSynchronize(sh.stream));
      big.reset();
    } else {
      HIPTRY(hipEventRecord(vs.ev_vstage[c].get(), sh.stream));
      used[c] = true;
      c ^= 1;
    }
    j = j1;
  }
  if (!pt.bins.empty()) {
    HIPTRY(vs.d_vbins.grow(sh.dev, pt.bins.size()));
    pt.d_bins = vs.d_vbins.get();
    HIPTRY(hipMemcpyAsync(pt.d_bins, pt.bins.data(), pt.bins.size() * sizeof(uint32_t), hipMemcpyHostToDevice,
                          sh.stream));
  }
  // the descriptors last: the padding pass filled their nonces (one pass over the objects' memory)
  HIPTRY(hipMemcpyAsync(pt.d_obj, ho.data(), m * sizeof(bv_obj), hipMemcpyHostToDevice, sh.stream));
  HIPTRY(hipStreamSynchronize(sh.stream));
  return 0;
}

// The binned kernel balances the SIMDs of a flood with at least a few waves per SIMD; a smaller
// one runs one wave per group in sorted order.  BMPOW_VBINNED=0/1 forces either (A/B runs).
bool verify_binned(size_t m, size_t nbins) {
  if (nbins == 0) return false;
  if (const char* e = std::getenv("BMPOW_VBINNED")) return std::atoi(e) != 0;
  return (m + BV_BLOCK - 1) / BV_BLOCK >= 2 * nbins;
}

std::vector<bmsched::VPart> g_vplan;  // under g_mu

// Hand a one-shot batch's plan vectors back to g_vplan before the batch is freed.
void vbatch_release_plan(bmpow_vbatch* vb) {
  g_vplan.resize(std::max(g_vplan.size(), vb->parts.size()));
  for (size_t i = 0; i < vb->parts.size(); ++i) std::swap(static_cast<bmsched::VPart&>(vb->parts[i]), g_vplan[i]);
}

int vbatch_build(bmpow_vbatch* vb, const std::vector<Span>& objs, bool transient) {
  vb->n = objs.size();
  vb->generation = g_generation;
  // the plan's vectors live in g_vplan between calls (swapped into the parts here, back by
  // vbatch_release_plan): a flood's descriptors are tens of MB, and fresh pages cost more than
  // the planning
  std::vector<bmsched::VPart>& plan = g_vplan;
  if (bmsched::plan_verify(objs, g_shards.size(), plan, vb->blocks) < 0)
    return set_err(BMPOW_E_ARG, "too many objects, an object too large, or a payload pool above 2^32 blocks");
  vb->parts.resize(plan.size());
  for (size_t i = 0; i < plan.size(); ++i) {
    bmsched::VPart& pt = vb->parts[i];
    std::swap(pt, plan[i]);
    const size_t nbins = 4 * (size_t)g_shards[pt.shard].cus;
    if (verify_binned(pt.orig.size(), nbins)) bmsched::plan_bins(pt, nbins);
  }
  for (auto& pt : vb->parts) {
    Shard& sh = g_shards[pt.shard];
    HIPTRY(hipSetDevice(sh.dev));
    const size_t m = pt.orig.size();
    if (transient) {
      const int rc = vbatch_upload_transient(pt, objs);
      if (rc < 0) return rc;
      continue;
    }
    // padding is a memory-bound copy of every payload: spread it over host threads
    std::unique_ptr<uint8_t[]> pool(new uint8_t[pt.blocks * 128]);  // pad_into writes every byte
    bmsched::pad_range(objs, pt, 0, m, 0, pool.get());
    HIPTRY(pt.own.obj.alloc(sh.dev, m));
    HIPTRY(pt.own.pool.alloc(sh.dev, std::max<size_t>(pt.blocks * 128, 16) / sizeof(uint4)));
    HIPTRY(pt.own.pow.alloc(sh.dev, m));
    HIPTRY(pt.own.h_pow.alloc(sh.dev, m, hipHostMallocDefault));
    pt.d_obj = pt.own.obj.get(), pt.d_pool = pt.own.pool.get(), pt.d_pow = pt.own.pow.get(), pt.h_pow = pt.own.h_pow.get();
    HIPTRY(hipMemcpy(pt.d_obj, pt.ho.data(), m * sizeof(bv_obj), hipMemcpyHostToDevice));
    HIPTRY(hipMemcpy(pt.d_pool, pool.get(), pt.blocks * 128, hipMemcpyHostToDevice));
    if (!pt.bins.empty()) {
      HIPTRY(pt.own.bins.alloc(sh.dev, pt.bins.size()));
      pt.d_bins = pt.own.bins.get();
      HIPTRY(hipMemcpy(pt.d_bins, pt.bins.data(), pt.bins.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
  }
  return 0;
}

int vbatch_run_locked(bmpow_vbatch* vb, uint64_t* pow_out) {
  if (g_abort.load()) return set_err(BMPOW_E_ABORTED, "aborted");  // process-wide, as for every other device call
  for (auto& pt : vb->parts) {
    Shard& sh = g_shards[pt.shard];
    HIPTRY(hipSetDevice(sh.dev));
    HIPTRY(hipEventRecord(sh.ev0.get(), sh.stream));
    if (pt.d_bins)
      HIPTRY(bv_launch_pow_binned(sh.stream, pt.d_obj, (uint32_t)pt.orig.size(), pt.d_pool, pt.d_pow, pt.d_bins,
                                  (uint32_t)pt.nbins));
    else
      HIPTRY(bv_launch_pow(sh.stream, pt.d_obj, (uint32_t)pt.orig.size(), pt.d_pool, pt.d_pow));
    HIPTRY(hipEventRecord(sh.ev1.get(), sh.stream));
    HIPTRY(hipMemcpyAsync(pt.h_pow, pt.d_pow, pt.orig.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, sh.stream));
  }
  double mx = 0;
  for (auto& pt : vb->parts) {
    Shard& sh = g_shards[pt.shard];
    HIPTRY(hipSetDevice(sh.dev));
    HIPTRY(hipStreamSynchronize(sh.stream));
    float ms = 0;
    HIPTRY(hipEventElapsedTime(&ms, sh.ev0.get(), sh.ev1.get()));
    mx = std::max<double>(mx, ms);
    g_stats.verify_launches++;
    if (pow_out)
      for (size_t j = 0; j < pt.orig.size(); ++j) pow_out[pt.orig[j]] = pt.h_pow[j];
  }
  g_stats.verify_kernel_ms += mx;
  g_stats.verify_objects += vb->n;
  g_stats.verify_blocks += vb->blocks;
  return 0;
}

int spans_from(size_t n, const uint8_t* objs, const uint64_t* offsets, std::vector<Span>& out) {
  if (n && (!objs || !offsets)) return set_err(BMPOW_E_ARG, "null pointer");
  out.resize(n);
  for (size_t i = 0; i < n; ++i) {
    if (offsets[i + 1] < offsets[i] + 8) return set_err(BMPOW_E_ARG, "object shorter than its 8-byte nonce");
    out[i] = {objs + offsets[i], offsets[i + 1] - offsets[i]};
  }
  return 0;
}

using bmsched::pow_sufficient;

}  // namespace bmhost

using namespace bmhost;

extern "C" {

bmpow_vbatch* bmpow_vbatch_create(size_t n, const uint8_t* objs, const uint64_t* offsets) {
  std::lock_guard<FairMutex> lk(g_mu);
  if (init_locked() < 0) return nullptr;
  std::vector<Span> spans;
  if (spans_from(n, objs, offsets, spans) < 0) return nullptr;
  bmpow_vbatch* vb = new bmpow_vbatch();
  if (vbatch_build(vb, spans) < 0) {
    delete vb;
    return nullptr;
  }
  return vb;
}

int bmpow_vbatch_run(bmpow_vbatch* vb, uint64_t* pow_out) {
  std::lock_guard<FairMutex> lk(g_mu);
  if (!vb) return set_err(BMPOW_E_STATE, "null verification batch");
  if (vb->generation != g_generation) return set_err(BMPOW_E_STATE, "device set changed under a live batch");
  return vbatch_run_locked(vb, pow_out);
}

void bmpow_vbatch_destroy(bmpow_vbatch* vb) {
  std::lock_guard<FairMutex> lk(g_mu);
  if (!vb) return;
  delete vb;
}

int bmpow_pow_values(size_t n, const uint8_t* objs, const uint64_t* offsets, uint64_t* pow_out) {
  std::lock_guard<FairMutex> lk(g_mu);
  int rc = init_locked();
  if (rc < 0) return rc;
  if (n == 0) return 0;
  if (!pow_out) return set_err(BMPOW_E_ARG, "null pointer");
  std::vector<Span> spans;
  rc = spans_from(n, objs, offsets, spans);
  if (rc < 0) return rc;
  bmpow_vbatch vb;
  rc = vbatch_build(&vb, spans, true);
  if (rc == 0) rc = vbatch_run_locked(&vb, pow_out);
  vbatch_release_plan(&vb);
  return rc;
}

// shared by both verify entry points (internal linkage despite the extern "C" block)
static int verify_spans_locked(size_t n, const uint8_t* const* ptrs, const uint64_t* lens, const uint64_t* ntpb,
                               const uint64_t* extra, const int64_t* recv_time, uint8_t* ok_out) {
  // scratch kept across calls under g_mu (a flood's worth of fresh pages costs several ms)
  static std::vector<Span> spans;
  static std::vector<size_t> idx;
  static std::vector<uint64_t> pow, eol;
  spans.clear();
  idx.clear();
  spans.reserve(n);
  idx.reserve(n);
  for (size_t i = 0; i < n; ++i) {
    if ((ntpb && ntpb[i] >= (1ULL << 62)) || (extra && extra[i] >= (1ULL << 62)))
      return set_err(BMPOW_E_ARG, "nonceTrialsPerByte / payloadLengthExtraBytes above 2^62");
    if (lens[i] < 16) {
      ok_out[i] = 2;  // the reference's unpack('>Q', data[8:16]) raises struct.error
      continue;
    }
    if (!ptrs[i]) return set_err(BMPOW_E_ARG, "null object pointer");
    spans.push_back({ptrs[i], lens[i]});
    idx.push_back(i);
  }
  using clk = std::chrono::steady_clock;
  auto ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
  const clk::time_point t0 = clk::now();
  pow.resize(spans.size());
  eol.resize(spans.size());
  if (!spans.empty()) {
    bmpow_vbatch vb;
    int rc = vbatch_build(&vb, spans, true);
    const clk::time_point t1 = clk::now();
    if (rc == 0) rc = vbatch_run_locked(&vb, pow.data());
    g_stats.verify_host_build_ms += ms(t0, t1);
    g_stats.verify_host_run_ms += ms(t1, clk::now());
    for (const auto& pt : vb.parts)  // expiresTime, read by the padding pass
      for (size_t j = 0; j < pt.orig.size(); ++j) eol[pt.orig[j]] = pt.eol[j];
    vbatch_release_plan(&vb);
    if (rc < 0) return rc;
  }
  const clk::time_point t2 = clk::now();
  const int64_t now = (int64_t)std::time(nullptr);
  bmsched::parallel_for(spans.size(), 32768, [&](size_t a, size_t b) {
    for (size_t j = a; j < b; ++j) {
      const size_t i = idx[j];
      const int64_t recv = (recv_time && recv_time[i]) ? recv_time[i] : now;
      ok_out[i] = (uint8_t)pow_sufficient(pow[j], spans[j].len, ntpb ? ntpb[i] : 0, extra ? extra[i] : 0, recv, eol[j]);
    }
  });
  g_stats.verify_host_verdict_ms += ms(t2, clk::now());
  return 0;
}

int bmpow_verify_batch(size_t n, const uint8_t* objs, const uint64_t* offsets, const uint64_t* ntpb,
                       const uint64_t* extra, const int64_t* recv_time, uint8_t* ok_out) {
  std::lock_guard<FairMutex> lk(g_mu);
  int rc = init_locked();
  if (rc < 0) return rc;
  if (n == 0) return 0;
  if (!objs || !offsets || !ok_out) return set_err(BMPOW_E_ARG, "null pointer");
  std::vector<const uint8_t*> ptrs(n);
  std::vector<uint64_t> lens(n);
  for (size_t i = 0; i < n; ++i) {
    if (offsets[i + 1] < offsets[i]) return set_err(BMPOW_E_ARG, "offsets are not ascending");
    ptrs[i] = objs + offsets[i];
    lens[i] = offsets[i + 1] - offsets[i];
  }
  return verify_spans_locked(n, ptrs.data(), lens.data(), ntpb, extra, recv_time, ok_out);
}

int bmpow_verify_batch_ptrs(size_t n, const uint8_t* const* objs, const uint64_t* lens, const uint64_t* ntpb,
                            const uint64_t* extra, const int64_t* recv_time, uint8_t* ok_out) {
  std::lock_guard<FairMutex> lk(g_mu);
  int rc = init_locked();
  if (rc < 0) return rc;
  if (n == 0) return 0;
  if (!objs || !lens || !ok_out) return set_err(BMPOW_E_ARG, "null pointer");
  return verify_spans_locked(n, objs, lens, ntpb, extra, recv_time, ok_out);
}

int bmpow_pow_sufficient(uint64_t pow, uint64_t len, uint64_t ntpb, uint64_t extra, int64_t recv_time,
                         uint64_t expires) {
  if (ntpb >= (1ULL << 62) || extra >= (1ULL << 62)) return set_err(BMPOW_E_ARG, "difficulty above 2^62");
  return pow_sufficient(pow, len, ntpb, extra, recv_time ? recv_time : (int64_t)std::time(nullptr), expires);
}

}  // extern "C"
