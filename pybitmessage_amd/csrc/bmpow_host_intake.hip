// bmpow_host_intake.hip -- batched object intake (include/bmpow_intake.h): the header walk and the
// reference's per-object checks on the host, and the one-shot run of the intake kernels
// (bmpow_intake.hip) over the verification's pool, plan and bins.
#include "bmpow_host_vbatch.h"

#include "bmpow_host_intake.h"  // intake_header, intake_status
#include "bmpow_intake_kernels.h"

namespace bmhost {

using bmsched::Span;

// What the intake adds per shard to the one-shot verification's buffers (indexed like g_shards,
// grow-only): each sorted object's length up, its 32-byte hash back.  POW values come back through the
// verification's own d_vpow / h_vpow (the part's pointers).
struct IntakeShard {
  PinBuf<uint32_t> h_len;
  DevBuf<uint32_t> d_len;
  DevBuf<uint4> d_inv;  // 2 per object
  PinBuf<uint8_t> h_inv;  // 32 per object
  Event ev0, ev1;  // around the launch (the shard's own pair belongs to the verification's stats)
};
std::vector<IntakeShard> g_intake;
bmpow_intake_stats g_intake_stats{};  // under g_mu

void intake_release_shards() { g_intake.clear(); }

using clk = std::chrono::steady_clock;
static double ms_between(clk::time_point a, clk::time_point b) {
  return std::chrono::duration<double, std::milli>(b - a).count();
}

// Both hash chains of every span: inv_of(i) -> 32 bytes for span i's hash, pow_out[i] (may be null).
// Under g_mu, devices initialised.
template <class InvOf>
int intake_run_locked(const std::vector<Span>& spans, InvOf&& inv_of, uint64_t* pow_out) {
  if (spans.empty()) return 0;
  if (g_abort.load()) return set_err(BMPOW_E_ABORTED, "aborted");  // process-wide, as for every other device call
  for (const Span& s : spans)
    if (s.len > 0xffffff00ULL) return set_err(BMPOW_E_ARG, "object of 4 GiB or more");
  const clk::time_point t0 = clk::now();
  bmpow_vbatch vb;
  int rc = vbatch_build(&vb, spans, true);
  auto run = [&]() -> int {
    if (g_intake.size() != g_shards.size()) g_intake.resize(g_shards.size());
    for (auto& pt : vb.parts) {
      Shard& sh = g_shards[pt.shard];
      IntakeShard& is = g_intake[pt.shard];
      HIPTRY(hipSetDevice(sh.dev));
      const size_t m = pt.orig.size();
      if (m > is.h_inv.cap() / 32 || !is.h_inv) {  // allocated last of the four: its capacity is theirs
        is.h_len.reset(), is.d_len.reset(), is.d_inv.reset(), is.h_inv.reset();
        const size_t cap = std::max<size_t>(m, 4096);
        HIPTRY(is.h_len.alloc(sh.dev, cap, hipHostMallocDefault));
        HIPTRY(is.d_len.alloc(sh.dev, cap));
        HIPTRY(is.d_inv.alloc(sh.dev, 2 * cap));
        HIPTRY(is.h_inv.alloc(sh.dev, 32 * cap, hipHostMallocDefault));
      }
      if (!is.ev0) HIPTRY(is.ev0.alloc(sh.dev));
      if (!is.ev1) HIPTRY(is.ev1.alloc(sh.dev));
      uint32_t* hl = is.h_len.get();
      bmsched::parallel_for(m, 65536, [&](size_t a, size_t b) {
        for (size_t j = a; j < b; ++j) hl[j] = (uint32_t)spans[pt.orig[j]].len;
      });
      HIPTRY(hipMemcpyAsync(is.d_len.get(), hl, m * sizeof(uint32_t), hipMemcpyHostToDevice, sh.stream));
    }
    const clk::time_point t1 = clk::now();
    g_intake_stats.host_build_ms += ms_between(t0, t1);
    for (auto& pt : vb.parts) {
      Shard& sh = g_shards[pt.shard];
      IntakeShard& is = g_intake[pt.shard];
      const uint32_t m = (uint32_t)pt.orig.size();
      HIPTRY(hipSetDevice(sh.dev));
      HIPTRY(hipEventRecord(is.ev0.get(), sh.stream));
      if (pt.d_bins)
        HIPTRY(bi_launch_binned(sh.stream, pt.d_obj, is.d_len.get(), m, pt.d_pool, pt.d_pow, is.d_inv.get(), pt.d_bins,
                                (uint32_t)pt.nbins));
      else
        HIPTRY(bi_launch(sh.stream, pt.d_obj, is.d_len.get(), m, pt.d_pool, pt.d_pow, is.d_inv.get()));
      HIPTRY(hipEventRecord(is.ev1.get(), sh.stream));
      HIPTRY(hipMemcpyAsync(is.h_inv.get(), is.d_inv.get(), (size_t)m * 32, hipMemcpyDeviceToHost, sh.stream));
      if (pow_out)
        HIPTRY(hipMemcpyAsync(pt.h_pow, pt.d_pow, (size_t)m * sizeof(uint64_t), hipMemcpyDeviceToHost, sh.stream));
    }
    double mx = 0;
    for (auto& pt : vb.parts) {
      Shard& sh = g_shards[pt.shard];
      IntakeShard& is = g_intake[pt.shard];
      HIPTRY(hipSetDevice(sh.dev));
      HIPTRY(hipStreamSynchronize(sh.stream));
      float ms = 0;
      HIPTRY(hipEventElapsedTime(&ms, is.ev0.get(), is.ev1.get()));
      mx = std::max<double>(mx, ms);
      g_intake_stats.launches++;
      const uint8_t* hi = is.h_inv.get();
      bmsched::parallel_for(pt.orig.size(), 32768, [&](size_t a, size_t b) {
        for (size_t j = a; j < b; ++j) {
          const size_t i = pt.orig[j];
          std::memcpy(inv_of(i), hi + 32 * j, 32);
          if (pow_out) pow_out[i] = pt.h_pow[j];
        }
      });
    }
    g_intake_stats.kernel_ms += mx;
    g_intake_stats.calls++;
    g_intake_stats.objects += vb.n;
    g_intake_stats.blocks += vb.blocks;
    g_intake_stats.host_run_ms += ms_between(t1, clk::now());
    return 0;
  };
  if (rc == 0) rc = run();
  vbatch_release_plan(&vb);
  return rc;
}

}  // namespace bmhost

using namespace bmhost;

extern "C" {

int bmpow_inventory_hashes(size_t n, const uint8_t* const* objs, const uint64_t* lens, uint8_t* inv_out) {
  std::lock_guard<FairMutex> lk(g_mu);
  int rc = init_locked();
  if (rc < 0) return rc;
  if (n == 0) return 0;
  if (!objs || !lens || !inv_out) return set_err(BMPOW_E_ARG, "null pointer");
  static std::vector<Span> spans;  // scratch kept across calls under g_mu
  spans.resize(n);
  for (size_t i = 0; i < n; ++i) {
    if (lens[i] < 8) return set_err(BMPOW_E_ARG, "object shorter than its 8-byte nonce");
    if (!objs[i]) return set_err(BMPOW_E_ARG, "null object pointer");
    spans[i] = {objs[i], lens[i]};
  }
  return intake_run_locked(spans, [&](size_t i) { return inv_out + 32 * i; }, nullptr);
}

int bmpow_intake_header(const uint8_t* obj, size_t len, bmpow_intake_rec* out) {
  if (!out) return set_err(BMPOW_E_ARG, "null pointer");
  return intake_header(obj, len, out);
}

int bmpow_intake_status(const bmpow_intake_rec* rec, size_t len, int pow_ok, int64_t now, const uint64_t* streams,
                        size_t n_streams) {
  return intake_status(rec, len, pow_ok, now, n_streams ? streams : nullptr, streams ? n_streams : 0);
}

int bmpow_intake_batch(size_t n, const uint8_t* const* objs, const uint64_t* lens, const bmpow_intake_params* prm,
                       bmpow_intake_rec* out) {
  std::lock_guard<FairMutex> lk(g_mu);
  int rc = init_locked();
  if (rc < 0) return rc;
  if (n == 0) return 0;
  if (!objs || !lens || !prm || !out) return set_err(BMPOW_E_ARG, "null pointer");
  if (prm->n_streams && !prm->streams) return set_err(BMPOW_E_ARG, "null stream list");
  if (prm->ntpb >= (1ULL << 62) || prm->extra >= (1ULL << 62))
    return set_err(BMPOW_E_ARG, "nonceTrialsPerByte / payloadLengthExtraBytes above 2^62");
  for (size_t i = 0; i < n; ++i)
    if (lens[i] && !objs[i]) return set_err(BMPOW_E_ARG, "null object pointer");
  const int64_t now = prm->now ? prm->now : (int64_t)std::time(nullptr);
  const int64_t recv = prm->recv_time ? prm->recv_time : now;
  // the header walk: which objects go up at all (the reference raises before it hashes for the PoW;
  // its constructor's inventory hash of such an object is never used)
  const clk::time_point t0 = clk::now();
  bmsched::parallel_for(n, 32768, [&](size_t a, size_t b) {
    for (size_t i = a; i < b; ++i) {
      bmpow_intake_rec& r = out[i];
      if (!intake_header(objs[i], lens[i], &r))
        r.status = BMPOW_INTAKE_MALFORMED;
      else if (lens[i] - r.payload_offset > BMPOW_INTAKE_MAX_PAYLOAD)
        r.status = BMPOW_INTAKE_TOO_LARGE;
    }
  });
  static std::vector<Span> spans;  // scratch kept across calls under g_mu
  static std::vector<size_t> idx;
  static std::vector<uint64_t> pow;
  spans.clear();
  idx.clear();
  spans.reserve(n);
  idx.reserve(n);
  for (size_t i = 0; i < n; ++i)
    if (out[i].status == BMPOW_INTAKE_OK) {
      spans.push_back({objs[i], lens[i]});
      idx.push_back(i);
    }
  pow.resize(spans.size());
  g_intake_stats.host_status_ms += ms_between(t0, clk::now());
  rc = intake_run_locked(spans, [&](size_t j) { return out[idx[j]].inv; }, pow.data());
  if (rc < 0) return rc;
  const clk::time_point t2 = clk::now();
  bmsched::parallel_for(spans.size(), 32768, [&](size_t a, size_t b) {
    for (size_t j = a; j < b; ++j) {
      const size_t i = idx[j];
      bmpow_intake_rec& r = out[i];
      r.pow = pow[j];
      const int ok = bmsched::pow_sufficient(pow[j], lens[i], prm->ntpb, prm->extra, recv, r.expires);
      r.status = intake_status(&r, lens[i], ok, now, prm->streams, prm->n_streams);
    }
  });
  g_intake_stats.host_status_ms += ms_between(t2, clk::now());
  return 0;
}

int bmpow_intake_get_stats(bmpow_intake_stats* out) {
  if (!out) return set_err(BMPOW_E_ARG, "null pointer");
  std::lock_guard<FairMutex> lk(g_mu);
  *out = g_intake_stats;
  return 0;
}

void bmpow_intake_reset_stats(void) {
  std::lock_guard<FairMutex> lk(g_mu);
  g_intake_stats = bmpow_intake_stats{};
}

}  // extern "C"
