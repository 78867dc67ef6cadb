// bmpow_host_seal.hip -- the host side of the seal kernels (bmpow_seal.hip): one set's pack, upload, launch,
// download and scatter, written once (round_trip) for the seal and the CBC kernel; the entry points bmpow_ecies_seal_batch, bmpow_aes256_cbc, bmpow_seal_plan and the
// mode knob and counters (include/bmpow_send.h, include/bmpow_ecies.h).
#include "bmpow_host_seal.h"

#include "../../include/bmpow_ecies.h"

// ---------------------------------------------------------------------------------------
// A call's rows are sorted by block count, descending (a wave's 64 lanes iterate alike), and cut into sets
// by bmseal::plan_slots: at most kSealSetRows rows and kSealSetPoolBytes of pool.  Per set the host's
// threads copy the inputs into a staging pool (bmsched::parallel_for), one upload, one launch, one
// download of the pool, and the threads copy the outputs out again; the abort flag is read between sets.
// A row's slot is its own, so packing and scattering never share a byte.  Everything runs on the first
// shard's device and stream.
// ---------------------------------------------------------------------------------------
namespace bmhost {

bmpow_seal_stats g_seal_stats{};

namespace {

std::atomic<int>& mode_cell() {  // BMPOW_SEAL=host|device, read once
  static std::atomic<int> m{[] {
    const char* e = std::getenv("BMPOW_SEAL");
    return e && std::strcmp(e, "device") == 0 ? 1 : (e && std::strcmp(e, "host") == 0 ? 0 : BMPOW_SEAL_DEFAULT);
  }()};
  return m;
}

// One set's trip through a kernel of bmpow_seal.hip, for n rows over pool_bytes of the pool: the host's
// threads pack (pack(j) fills row j's sl_row, IV and key and its slot of the staging pool), one upload, the
// launch, one download, and the threads scatter (scatter(j, len) copies row j's result out; false for a
// length the host's own arithmetic excludes, and `never` is then the call's error).  The stream is drained on
// return; the four times and the counters go to g_seal_stats.
template <class Pack, class Launch, class Scatter>
int round_trip(Shard& sh, SealIo& io, uint32_t n, uint64_t pool_bytes, const char* never, Pack pack, Launch launch,
               Scatter scatter) {
  auto t0 = std::chrono::steady_clock::now();
  uint8_t* hp = io.host.get();
  bmsched::parallel_for(n, 1024, [&](size_t a, size_t z) {
    for (size_t j = a; j < z; ++j) pack(j);
  });
  g_seal_stats.pack_ms += ms_since(t0);
  HIPTRY(hipEventRecord(io.ev[0].get(), sh.stream));
  HIPTRY(hipMemcpyAsync(io.pool.get(), hp, pool_bytes, hipMemcpyHostToDevice, sh.stream));
  HIPTRY(hipMemcpyAsync(io.rows.get(), io.hrows.data(), n * sizeof(sl_row), hipMemcpyHostToDevice, sh.stream));
  HIPTRY(hipMemcpyAsync(io.iv.get(), io.hiv.data(), (size_t)16 * n, hipMemcpyHostToDevice, sh.stream));
  if (io.keys) HIPTRY(hipMemcpyAsync(io.keys.get(), io.hkeys.v.data(), (size_t)32 * n, hipMemcpyHostToDevice, sh.stream));
  HIPTRY(hipEventRecord(io.ev[1].get(), sh.stream));
  HIPTRY(launch());
  HIPTRY(hipEventRecord(io.ev[2].get(), sh.stream));
  HIPTRY(hipMemcpyAsync(hp, io.pool.get(), pool_bytes, hipMemcpyDeviceToHost, sh.stream));
  HIPTRY(hipMemcpyAsync(io.hlen.data(), io.out_len.get(), n * sizeof(int32_t), hipMemcpyDeviceToHost, sh.stream));
  HIPTRY(hipEventRecord(io.ev[3].get(), sh.stream));
  HIPTRY(hipStreamSynchronize(sh.stream));
  double* const acc[3] = {&g_seal_stats.copy_ms, &g_seal_stats.seal_kernel_ms, &g_seal_stats.copy_ms};
  if (const int rc = elapsed_phases(acc, io.ev, 3); rc < 0) return rc;
  t0 = std::chrono::steady_clock::now();
  std::atomic<bool> bad{false};
  bmsched::parallel_for(n, 1024, [&](size_t a, size_t z) {
    for (size_t j = a; j < z; ++j)
      if (!scatter(j, io.hlen[j])) bad.store(true);
  });
  g_seal_stats.scatter_ms += ms_since(t0);
  if (bad.load()) return set_err(BMPOW_E_HIP, never);
  g_seal_stats.rows_device += n;
  g_seal_stats.sets++;
  g_seal_stats.launches++;
  return 0;
}

}  // namespace

int seal_mode() { return mode_cell().load(std::memory_order_relaxed); }

int SealIo::init(int dev, size_t max_rows, uint64_t max_pool, bool with_keys) {
  const size_t stride = round_up((uint32_t)max_rows, SL_BLOCK);
  HIPTRY(pool.alloc(dev, max_pool));
  if (with_keys) HIPTRY(keys.alloc(dev, 2 * stride));
  HIPTRY(rows.alloc(dev, stride));
  HIPTRY(iv.alloc(dev, stride));
  HIPTRY(out_len.alloc(dev, stride));
  for (Event& e : ev) HIPTRY(e.alloc(dev));
  host.alloc(max_pool);
  if (with_keys) hkeys.v.resize(32 * max_rows);
  hrows.resize(max_rows);
  hiv.resize(16 * max_rows);
  hlen.resize(max_rows);
  return 0;
}

int seal_set(Shard& sh, SealIo& io, const SealSet& s, const uint64_t* kout, const ec::ge* pt, const uint32_t* ok) {
  if (s.pool_bytes > io.host.bytes || s.stride > io.rows.cap() || s.n > io.hrows.size())
    return set_err(BMPOW_E_ARG, "seal set above the call's buffers");
  uint8_t* hp = io.host.get();
  return round_trip(
      sh, io, s.n, s.pool_bytes, "the seal kernel returned a length above the blob's bound",
      [&](size_t j) {
        const size_t row = s.row[j];
        io.hrows[j] = sl_row{(uint32_t)(s.off[j] / 16), (uint32_t)s.lens[row]};
        std::memcpy(io.hiv.data() + 16 * j, s.ivs + 16 * row, 16);
        if (s.lens[row]) std::memcpy(hp + s.off[j] + SL_PLAIN_AT, s.plains[row], s.lens[row]);
      },
      [&] {
        return sl_launch_seal(sh.stream, kout, pt, ok, io.iv.get(), io.rows.get(), io.pool.get(), s.n, s.stride,
                              reinterpret_cast<uint32_t*>(io.out_len.get()));
      },
      [&](size_t j, int32_t len) {
        const size_t row = s.row[j];
        const uint64_t l = (uint32_t)len;
        if (l > BMPOW_ECIES_BLOB_CAP(s.lens[row])) return false;  // never: the kernel's lengths follow the host's
        if (l) std::memcpy(s.outs[row], hp + s.off[j], l);
        s.out_lens[row] = l;
        return true;
      });
}

namespace {

struct KeyBufs {  // bmpow_ecies_seal_batch: the keys and points as the send kernels would have left them
  WipeDevBuf<uint64_t> kout;
  DevBuf<ec::ge> pt;
  Wiped<uint64_t> hkout;
  std::vector<ec::ge> hpt;
};

int seal_batch_locked(const std::vector<uint32_t>& order, const uint8_t* const* plains, const uint64_t* lens,
                      const uint8_t* ivs, const uint8_t* R_xy, const uint8_t* keys, uint8_t* const* outs,
                      uint64_t* out_lens) {
  const size_t n = order.size();
  bmseal::SlotPlan p;
  p.slot.resize(n);
  for (size_t i = 0; i < n; ++i) p.slot[i] = bmseal::seal_slot_bytes(lens[order[i]]);
  if (!p.plan(kSealSetRows, kSealSetPoolBytes)) return set_err(BMPOW_E_ARG, "seal plan refused");
  Shard& sh = g_shards[0];
  HIPTRY(hipSetDevice(sh.dev));
  SealIo io;
  if (const int rc = io.init(sh.dev, p.sets.max_rows, p.sets.max_pool); rc < 0) return rc;
  KeyBufs kb;
  const uint32_t cap_stride = round_up((uint32_t)p.sets.max_rows, SL_BLOCK);
  HIPTRY(kb.kout.alloc(sh.dev, (size_t)8 * cap_stride));
  HIPTRY(kb.pt.alloc(sh.dev, cap_stride));
  kb.hkout.v.resize((size_t)8 * cap_stride);
  kb.hpt.resize(cap_stride);
  g_seal_stats.calls++;
  for (size_t k = 0; k < p.sets.count(); ++k) {
    if (g_abort.load()) return set_err(BMPOW_E_ABORTED, "aborted");
    const size_t i0 = p.sets.begin[k], i1 = p.sets.begin[k + 1];
    SealSet s;
    s.n = (uint32_t)(i1 - i0);
    s.stride = round_up(s.n, SL_BLOCK);
    s.row = order.data() + i0;
    s.off = p.off.data() + i0;
    s.pool_bytes = p.pool_bytes(k);
    s.plains = plains, s.lens = lens, s.ivs = ivs, s.outs = outs, s.out_lens = out_lens;
    for (uint32_t j = 0; j < s.n; ++j) {
      const size_t row = order[i0 + j];
      for (int w = 0; w < 8; ++w) kb.hkout.v[(size_t)w * s.stride + j] = bmsched::load_be64(keys + 64 * row + 8 * w);
      kb.hpt[j] = ge_from_be(R_xy + 64 * row);
    }
    HIPTRY(hipMemcpyAsync(kb.kout.get(), kb.hkout.v.data(), (size_t)8 * s.stride * sizeof(uint64_t), hipMemcpyHostToDevice,
                          sh.stream));
    HIPTRY(hipMemcpyAsync(kb.pt.get(), kb.hpt.data(), s.n * sizeof(ec::ge), hipMemcpyHostToDevice, sh.stream));
    if (const int rc = seal_set(sh, io, s, kb.kout.get(), kb.pt.get(), nullptr); rc < 0) return rc;
  }
  return 0;
}

int cbc_locked(const std::vector<uint32_t>& order, int decrypt, const uint8_t* keys, const uint8_t* ivs,
               const uint8_t* const* in, const uint64_t* in_lens, uint8_t* const* out, int64_t* out_lens) {
  const size_t n = order.size();
  bmseal::SlotPlan p;
  p.slot.resize(n);
  for (size_t i = 0; i < n; ++i) p.slot[i] = decrypt ? in_lens[order[i]] : bmseal::cbc_len(in_lens[order[i]]);
  if (!p.plan(kSealSetRows, kSealSetPoolBytes)) return set_err(BMPOW_E_ARG, "CBC plan refused");
  Shard& sh = g_shards[0];
  HIPTRY(hipSetDevice(sh.dev));
  SealIo io;
  if (const int rc = io.init(sh.dev, p.sets.max_rows, p.sets.max_pool, true); rc < 0) return rc;
  uint8_t* hp = io.host.get();
  g_seal_stats.calls++;
  for (size_t k = 0; k < p.sets.count(); ++k) {
    if (g_abort.load()) return set_err(BMPOW_E_ABORTED, "aborted");
    const size_t i0 = p.sets.begin[k];
    const uint32_t m = (uint32_t)(p.sets.begin[k + 1] - i0), stride = round_up(m, SL_BLOCK);
    const int rc = round_trip(
        sh, io, m, p.pool_bytes(k), "the CBC kernel returned a length above the slot",
        [&](size_t j) {
          const size_t row = order[i0 + j];
          io.hrows[j] = sl_row{(uint32_t)(p.off[i0 + j] / 16), (uint32_t)in_lens[row]};
          std::memcpy(io.hkeys.v.data() + 32 * j, keys + 32 * row, 32);
          std::memcpy(io.hiv.data() + 16 * j, ivs + 16 * row, 16);
          if (in_lens[row]) std::memcpy(hp + p.off[i0 + j], in[row], in_lens[row]);
        },
        [&] {
          return sl_launch_cbc(sh.stream, decrypt, io.keys.get(), io.iv.get(), io.rows.get(), io.pool.get(), m, stride,
                               io.out_len.get());
        },
        [&](size_t j, int32_t l) {
          const size_t row = order[i0 + j];
          if (l > (int64_t)p.slot[i0 + j]) return false;  // never: the kernel's lengths follow the host's
          if (l > 0) std::memcpy(out[row], hp + p.off[i0 + j], (size_t)l);
          out_lens[row] = l < 0 ? -1 : l;
          return true;
        });
    if (rc < 0) return rc;
  }
  return 0;
}

}  // namespace
}  // namespace bmhost

using namespace bmhost;

extern "C" {

int bmpow_ecies_seal_batch(size_t n, const uint8_t* const* plains, const uint64_t* lens, const uint8_t* ivs,
                           const uint8_t* R_xy, const uint8_t* keys, uint8_t* const* outs, const uint64_t* out_caps,
                           uint64_t* out_lens) {
  std::lock_guard<FairMutex> lk(g_mu);
  if (n == 0) return 0;
  if (!plains || !lens || !ivs || !R_xy || !keys || !outs || !out_caps || !out_lens) return set_err(BMPOW_E_ARG, "null pointer");
  if (n > 0xffffffffull) return set_err(BMPOW_E_ARG, "too many plaintexts");
  std::memset(out_lens, 0, n * sizeof(uint64_t));
  std::vector<uint32_t> order, big;
  order.reserve(n);
  for (size_t i = 0; i < n; ++i) {
    if ((lens[i] && !plains[i]) || !outs[i]) return set_err(BMPOW_E_ARG, "null plaintext or output pointer");
    if (lens[i] > bmseal::kMaxPlain) return set_err(BMPOW_E_ARG, "plaintext above 2^31 - 16 bytes");
    if (out_caps[i] < BMPOW_ECIES_BLOB_CAP(lens[i])) return set_err(BMPOW_E_ARG, "output buffer below BMPOW_ECIES_BLOB_CAP");
    (lens[i] > bmseal::kDevicePlain ? big : order).push_back((uint32_t)i);
  }
  if (g_abort.load()) return set_err(BMPOW_E_ABORTED, "aborted");
  if (!order.empty()) {
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return lens[a] / 16 > lens[b] / 16; });
    int rc = init_locked();
    if (rc >= 0) rc = seal_batch_locked(order, plains, lens, ivs, R_xy, keys, outs, out_lens);
    if (rc < 0) return rc;
  }
  for (uint32_t i : big) {  // above the protocol's object size: the host's sealer, the same bytes
    const int64_t l = bmpow_ecies_seal(plains[i], lens[i], ivs + 16 * (size_t)i, R_xy + 64 * (size_t)i, keys + 64 * (size_t)i,
                                       outs[i], out_caps[i]);
    if (l < 0) return (int)l;
    out_lens[i] = (uint64_t)l;
    g_seal_stats.rows_host++;
  }
  return 0;
}

int bmpow_aes256_cbc(size_t n, int decrypt, const uint8_t* keys, const uint8_t* ivs, const uint8_t* const* in,
                     const uint64_t* in_lens, uint8_t* const* out, const uint64_t* out_caps, int64_t* out_lens) {
  std::lock_guard<FairMutex> lk(g_mu);
  if (n == 0) return 0;
  if (!keys || !ivs || !in || !in_lens || !out || !out_caps || !out_lens) return set_err(BMPOW_E_ARG, "null pointer");
  if (n > 0xffffffffull) return set_err(BMPOW_E_ARG, "too many messages");
  std::vector<uint32_t> order;
  order.reserve(n);
  for (size_t i = 0; i < n; ++i) {
    out_lens[i] = -1;
    if ((in_lens[i] && !in[i]) || !out[i]) return set_err(BMPOW_E_ARG, "null input or output pointer");
    if (in_lens[i] > bmseal::kMaxPlain) return set_err(BMPOW_E_ARG, "message above 2^31 - 16 bytes");
    if (decrypt && (in_lens[i] == 0 || in_lens[i] % 16)) continue;  // where the reference's decrypt raises
    if (out_caps[i] < (decrypt ? in_lens[i] : bmseal::cbc_len(in_lens[i])))
      return set_err(BMPOW_E_ARG, "output buffer smaller than the padded message");
    order.push_back((uint32_t)i);
  }
  if (g_abort.load()) return set_err(BMPOW_E_ABORTED, "aborted");
  if (order.empty()) return 0;
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return in_lens[a] / 16 > in_lens[b] / 16; });
  int rc = init_locked();
  if (rc >= 0) rc = cbc_locked(order, decrypt ? 1 : 0, keys, ivs, in, in_lens, out, out_lens);
  return rc > 0 ? 0 : rc;
}

int64_t bmpow_seal_plan(size_t n, const uint64_t* lens, uint64_t max_rows, uint64_t max_bytes, uint32_t* set_out,
                        uint64_t* off_out) {
  const int64_t sets = bmseal::plan_seal(n, lens, max_rows, max_bytes, set_out, off_out);
  if (sets < 0) return set_err(BMPOW_E_ARG, "null pointer, a zero limit or a length above 2^31 - 16 bytes");
  return sets;
}

int bmpow_send_set_seal(int mode) {
  std::atomic<int>& m = mode_cell();
  if (mode != 0 && mode != 1) return m.load();
  return m.exchange(mode);
}

int bmpow_seal_get_stats(bmpow_seal_stats* out) {
  std::lock_guard<FairMutex> lk(g_mu);
  if (!out) return set_err(BMPOW_E_ARG, "null pointer");
  *out = g_seal_stats;
  return 0;
}

void bmpow_seal_reset_stats(void) {
  std::lock_guard<FairMutex> lk(g_mu);
  g_seal_stats = bmpow_seal_stats{};
}

}  // extern "C"
