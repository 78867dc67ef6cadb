// bmpow_host_ident.hip -- the sender identification's host side: the bmpow_ident_* entry points
// (include/bmpow_ident.h) over the kernels of bmpow_ident.hip.
#include "bmpow_host.h"

#include "../../include/bmpow_ident.h"
#include "bmpow_ident_kernels.h"

// ---------------------------------------------------------------------------------------
// One call: the rows go through the device in sets of at most kIdentSetRows, each set one upload, one
// launch and one download of the records straight into the caller's array, with the abort flag read
// between sets.  The buffers are the call's own (DevBuf owners, released when it returns); everything
// runs on the first shard's device and stream.
// ---------------------------------------------------------------------------------------
namespace bmhost {
namespace {

constexpr size_t kIdentSetRows = 1u << 18;  // as the signature and ECIES sets: 4,096 waves

bmpow_ident_stats g_ident_stats{};  // under g_mu

struct IdentBufs {  // one call's buffers on the device
  DevBuf<uint4> in;  // 8 per row (keys) or the ripes' 5 words per row, rounded up
  DevBuf<uint64_t> versions, streams;
  DevBuf<bmpow_ident_rec> out;
  Event ev0, ev1;
};

// in: n rows of in_bytes each (128: keys, 20: ripes)
int ident_run_locked(size_t n, const uint8_t* in, size_t in_bytes, const uint64_t* versions, const uint64_t* streams,
                     bmpow_ident_rec* out) {
  Shard& sh = g_shards[0];
  HIPTRY(hipSetDevice(sh.dev));
  IdentBufs b;
  HIPTRY(b.ev0.alloc(sh.dev));
  HIPTRY(b.ev1.alloc(sh.dev));
  const size_t cap = std::min(n, kIdentSetRows);
  HIPTRY(b.in.alloc(sh.dev, (cap * in_bytes + sizeof(uint4) - 1) / sizeof(uint4)));
  HIPTRY(b.versions.alloc(sh.dev, cap));
  HIPTRY(b.streams.alloc(sh.dev, cap));
  HIPTRY(b.out.alloc(sh.dev, cap));
  g_ident_stats.calls++;
  for (size_t i0 = 0; i0 < n; i0 += kIdentSetRows) {
    if (g_abort.load()) return set_err(BMPOW_E_ABORTED, "aborted");
    const uint32_t m = (uint32_t)std::min(kIdentSetRows, n - i0);
    HIPTRY(hipMemcpyAsync(b.in.get(), in + i0 * in_bytes, m * in_bytes, hipMemcpyHostToDevice, sh.stream));
    HIPTRY(hipMemcpyAsync(b.versions.get(), versions + i0, m * sizeof(uint64_t), hipMemcpyHostToDevice, sh.stream));
    HIPTRY(hipMemcpyAsync(b.streams.get(), streams + i0, m * sizeof(uint64_t), hipMemcpyHostToDevice, sh.stream));
    HIPTRY(hipEventRecord(b.ev0.get(), sh.stream));
    if (in_bytes == 128)
      HIPTRY(id_launch_derive(sh.stream, b.in.get(), b.versions.get(), b.streams.get(), m, b.out.get()));
    else
      HIPTRY(id_launch_from_ripe(sh.stream, reinterpret_cast<const uint32_t*>(b.in.get()), b.versions.get(),
                                 b.streams.get(), m, b.out.get()));
    HIPTRY(hipEventRecord(b.ev1.get(), sh.stream));
    HIPTRY(hipMemcpyAsync(out + i0, b.out.get(), m * sizeof(bmpow_ident_rec), hipMemcpyDeviceToHost, sh.stream));
    HIPTRY(hipStreamSynchronize(sh.stream));
    float ms = 0;
    HIPTRY(hipEventElapsedTime(&ms, b.ev0.get(), b.ev1.get()));
    g_ident_stats.kernel_ms += ms;
    g_ident_stats.sets++;
    g_ident_stats.launches++;
  }
  return 0;
}

int ident_call(size_t n, const uint8_t* in, size_t in_bytes, const uint64_t* versions, const uint64_t* streams,
               bmpow_ident_rec* out) {
  std::lock_guard<FairMutex> lk(g_mu);
  if (n == 0) return 0;
  if (!in || !versions || !streams || !out) return set_err(BMPOW_E_ARG, "null pointer");
  if (n > 0xffffffffull) return set_err(BMPOW_E_ARG, "too many rows");
  const auto t_begin = std::chrono::steady_clock::now();
  int rc = init_locked();
  if (rc >= 0) rc = ident_run_locked(n, in, in_bytes, versions, streams, out);
  if (rc > 0) rc = 0;
  g_ident_stats.rows += n;
  g_ident_stats.host_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
  return rc;
}

}  // namespace
}  // namespace bmhost

using namespace bmhost;

extern "C" {

int bmpow_ident_derive(size_t n, const uint8_t* keys128, const uint64_t* versions, const uint64_t* streams,
                       bmpow_ident_rec* out) {
  return ident_call(n, keys128, 128, versions, streams, out);
}

int bmpow_ident_from_ripe(size_t n, const uint8_t* ripes20, const uint64_t* versions, const uint64_t* streams,
                          bmpow_ident_rec* out) {
  return ident_call(n, ripes20, 20, versions, streams, out);
}

int bmpow_ident_get_stats(bmpow_ident_stats* out) {
  std::lock_guard<FairMutex> lk(g_mu);
  if (!out) return set_err(BMPOW_E_ARG, "null pointer");
  *out = g_ident_stats;
  return 0;
}

void bmpow_ident_reset_stats(void) {
  std::lock_guard<FairMutex> lk(g_mu);
  g_ident_stats = bmpow_ident_stats{};
}

}  // extern "C"
