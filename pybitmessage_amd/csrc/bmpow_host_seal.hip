// bmpow_host_seal.hip -- the host side of the seal kernels (bmpow_seal.hip): one set's pack, upload, launch,
// download and scatter; the entry points bmpow_ecies_seal_batch, bmpow_aes256_cbc, bmpow_seal_plan and the
// mode knob and counters (include/bmpow_send.h, include/bmpow_ecies.h).
#include "bmpow_host_seal.h"

#include <openssl/crypto.h>

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

template <class T>
void wipe_dev(const DevBuf<T>& b) {
  if (b && !bmown::g_exiting.load(std::memory_order_relaxed) && hipSetDevice(b.dev()) == hipSuccess)
    (void)hipMemset(b.get(), 0, b.cap() * sizeof(T));
}

double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

int elapsed(double& acc, const Event& a, const Event& b) {
  float ms = 0;
  HIPTRY(hipEventElapsedTime(&ms, a.get(), b.get()));
  acc += ms;
  return 0;
}

uint32_t round_up(uint32_t n, uint32_t q) { return (n + q - 1) / q * q; }

// the sets of a planned call: [begin, end) of each, and the largest pool
struct Sets {
  std::vector<size_t> begin;  // begin[k] .. begin[k + 1]
  uint64_t max_pool = 16;
  size_t max_rows = 0;
};

Sets cut_sets(const std::vector<uint32_t>& set, const std::vector<uint64_t>& off, const std::vector<uint64_t>& slots) {
  Sets s;
  const size_t n = set.size();
  for (size_t i = 0; i < n; ++i) {
    if (i == 0 || set[i] != set[i - 1]) s.begin.push_back(i);
    s.max_pool = std::max(s.max_pool, off[i] + slots[i]);
  }
  s.begin.push_back(n);
  for (size_t k = 0; k + 1 < s.begin.size(); ++k) s.max_rows = std::max(s.max_rows, s.begin[k + 1] - s.begin[k]);
  return s;
}

}  // namespace

int seal_mode() { return mode_cell().load(std::memory_order_relaxed); }

int SealIo::init(int dev, size_t max_rows, uint64_t max_pool) {
  const size_t stride = round_up((uint32_t)max_rows, SL_BLOCK);
  HIPTRY(pool.alloc(dev, max_pool));
  HIPTRY(rows.alloc(dev, stride));
  HIPTRY(iv.alloc(dev, stride));
  HIPTRY(out_len.alloc(dev, stride));
  for (Event& e : ev) HIPTRY(e.alloc(dev));
  host.reset(new uint8_t[max_pool]);
  host_bytes = max_pool;
  return 0;
}

SealIo::~SealIo() {
  wipe_dev(pool);
  if (host) OPENSSL_cleanse(host.get(), host_bytes);
}

int seal_set(Shard& sh, SealIo& io, const SealSet& s, const uint64_t* kout, const ec::ge* pt, const uint32_t* ok) {
  if (s.pool_bytes > io.host_bytes || s.stride > io.rows.cap()) return set_err(BMPOW_E_ARG, "seal set above the call's buffers");
  auto t0 = std::chrono::steady_clock::now();
  io.hrows.resize(s.n);
  io.hiv.resize((size_t)16 * s.n);
  io.hlen.resize(s.n);
  uint8_t* hp = io.host.get();
  bmsched::parallel_for(s.n, 1024, [&](size_t a, size_t z) {
    for (size_t j = a; j < z; ++j) {
      const size_t row = s.row[j];
      io.hrows[j] = sl_row{(uint32_t)(s.off[j] / 16), (uint32_t)s.lens[row]};
      std::memcpy(io.hiv.data() + 16 * j, s.ivs + 16 * row, 16);
      if (s.lens[row]) std::memcpy(hp + s.off[j] + SL_PLAIN_AT, s.plains[row], s.lens[row]);
    }
  });
  g_seal_stats.pack_ms += ms_since(t0);
  HIPTRY(hipEventRecord(io.ev[0].get(), sh.stream));
  HIPTRY(hipMemcpyAsync(io.pool.get(), hp, s.pool_bytes, hipMemcpyHostToDevice, sh.stream));
  HIPTRY(hipMemcpyAsync(io.rows.get(), io.hrows.data(), s.n * sizeof(sl_row), hipMemcpyHostToDevice, sh.stream));
  HIPTRY(hipMemcpyAsync(io.iv.get(), io.hiv.data(), (size_t)16 * s.n, hipMemcpyHostToDevice, sh.stream));
  HIPTRY(hipEventRecord(io.ev[1].get(), sh.stream));
  HIPTRY(sl_launch_seal(sh.stream, kout, pt, ok, io.iv.get(), io.rows.get(), io.pool.get(), s.n, s.stride, io.out_len.get()));
  HIPTRY(hipEventRecord(io.ev[2].get(), sh.stream));
  HIPTRY(hipMemcpyAsync(hp, io.pool.get(), s.pool_bytes, hipMemcpyDeviceToHost, sh.stream));
  HIPTRY(hipMemcpyAsync(io.hlen.data(), io.out_len.get(), s.n * sizeof(uint32_t), hipMemcpyDeviceToHost, sh.stream));
  HIPTRY(hipEventRecord(io.ev[3].get(), sh.stream));
  HIPTRY(hipStreamSynchronize(sh.stream));
  if (const int rc = elapsed(g_seal_stats.copy_ms, io.ev[0], io.ev[1]); rc < 0) return rc;
  if (const int rc = elapsed(g_seal_stats.seal_kernel_ms, io.ev[1], io.ev[2]); rc < 0) return rc;
  if (const int rc = elapsed(g_seal_stats.copy_ms, io.ev[2], io.ev[3]); rc < 0) return rc;
  t0 = std::chrono::steady_clock::now();
  std::atomic<bool> bad{false};
  bmsched::parallel_for(s.n, 1024, [&](size_t a, size_t z) {
    for (size_t j = a; j < z; ++j) {
      const size_t row = s.row[j];
      const uint64_t l = io.hlen[j];
      if (l > BMPOW_ECIES_BLOB_CAP(s.lens[row])) {  // never: the kernel's lengths follow the host's
        bad.store(true);
        continue;
      }
      if (l) std::memcpy(s.outs[row], hp + s.off[j], l);
      s.out_lens[row] = l;
    }
  });
  g_seal_stats.scatter_ms += ms_since(t0);
  if (bad.load()) return set_err(BMPOW_E_HIP, "the seal kernel returned a length above the blob's bound");
  g_seal_stats.rows_device += s.n;
  g_seal_stats.sets++;
  g_seal_stats.launches++;
  return 0;
}

namespace {

struct KeyBufs {  // bmpow_ecies_seal_batch: the keys and points as the send kernels would have left them
  DevBuf<uint64_t> kout;
  DevBuf<ec::ge> pt;
  std::vector<uint64_t> hkout;
  std::vector<ec::ge> hpt;
  ~KeyBufs() {
    wipe_dev(kout);
    if (!hkout.empty()) OPENSSL_cleanse(hkout.data(), hkout.size() * sizeof(uint64_t));
  }
};

int seal_batch_locked(const std::vector<uint32_t>& order, const uint8_t* const* plains, const uint64_t* lens,
                      const uint8_t* ivs, const uint8_t* R_xy, const uint8_t* keys, uint8_t* const* outs,
                      uint64_t* out_lens) {
  const size_t n = order.size();
  std::vector<uint64_t> slots(n), off(n);
  std::vector<uint32_t> set(n);
  for (size_t i = 0; i < n; ++i) slots[i] = bmseal::seal_slot_bytes(lens[order[i]]);
  if (bmseal::plan_slots(n, slots.data(), kSealSetRows, kSealSetPoolBytes, set.data(), off.data()) < 0)
    return set_err(BMPOW_E_ARG, "seal plan refused");
  const Sets sets = cut_sets(set, off, slots);
  Shard& sh = g_shards[0];
  HIPTRY(hipSetDevice(sh.dev));
  SealIo io;
  if (const int rc = io.init(sh.dev, sets.max_rows, sets.max_pool); rc < 0) return rc;
  KeyBufs kb;
  const uint32_t cap_stride = round_up((uint32_t)sets.max_rows, SL_BLOCK);
  HIPTRY(kb.kout.alloc(sh.dev, (size_t)8 * cap_stride));
  HIPTRY(kb.pt.alloc(sh.dev, cap_stride));
  kb.hkout.resize((size_t)8 * cap_stride);
  kb.hpt.resize(cap_stride);
  g_seal_stats.calls++;
  for (size_t k = 0; k + 1 < sets.begin.size(); ++k) {
    if (g_abort.load()) return set_err(BMPOW_E_ABORTED, "aborted");
    const size_t i0 = sets.begin[k], i1 = sets.begin[k + 1];
    SealSet s;
    s.n = (uint32_t)(i1 - i0);
    s.stride = round_up(s.n, SL_BLOCK);
    s.row = order.data() + i0;
    s.off = off.data() + i0;
    s.pool_bytes = off[i1 - 1] + slots[i1 - 1];
    s.plains = plains, s.lens = lens, s.ivs = ivs, s.outs = outs, s.out_lens = out_lens;
    for (uint32_t j = 0; j < s.n; ++j) {
      const size_t row = order[i0 + j];
      for (int w = 0; w < 8; ++w) kb.hkout[(size_t)w * s.stride + j] = bmsched::load_be64(keys + 64 * row + 8 * w);
      const uint8_t* q = R_xy + 64 * row;
      for (int i = 0; i < 8; ++i) {  // little-endian limbs of the big-endian coordinates
        const uint8_t *x = q + 28 - 4 * i, *y = q + 60 - 4 * i;
        kb.hpt[j].x.d[i] = (uint32_t)x[0] << 24 | (uint32_t)x[1] << 16 | (uint32_t)x[2] << 8 | x[3];
        kb.hpt[j].y.d[i] = (uint32_t)y[0] << 24 | (uint32_t)y[1] << 16 | (uint32_t)y[2] << 8 | y[3];
      }
    }
    HIPTRY(hipMemcpyAsync(kb.kout.get(), kb.hkout.data(), (size_t)8 * s.stride * sizeof(uint64_t), hipMemcpyHostToDevice,
                          sh.stream));
    HIPTRY(hipMemcpyAsync(kb.pt.get(), kb.hpt.data(), s.n * sizeof(ec::ge), hipMemcpyHostToDevice, sh.stream));
    if (const int rc = seal_set(sh, io, s, kb.kout.get(), kb.pt.get(), nullptr); rc < 0) return rc;
  }
  return 0;
}

struct CbcBufs {
  DevBuf<uint8_t> pool;
  DevBuf<uint4> keys, iv;
  DevBuf<sl_row> rows;
  DevBuf<int32_t> out_len;
  Event ev[4];
  std::unique_ptr<uint8_t[]> host;
  size_t host_bytes = 0;
  std::vector<uint8_t> hkeys, hiv;
  std::vector<sl_row> hrows;
  std::vector<int32_t> hlen;
  ~CbcBufs() {
    wipe_dev(pool);
    wipe_dev(keys);
    if (host) OPENSSL_cleanse(host.get(), host_bytes);
    if (!hkeys.empty()) OPENSSL_cleanse(hkeys.data(), hkeys.size());
  }
};

int cbc_locked(const std::vector<uint32_t>& order, int decrypt, const uint8_t* keys, const uint8_t* ivs,
               const uint8_t* const* in, const uint64_t* in_lens, uint8_t* const* out, int64_t* out_lens) {
  const size_t n = order.size();
  std::vector<uint64_t> slots(n), off(n);
  std::vector<uint32_t> set(n);
  for (size_t i = 0; i < n; ++i) slots[i] = decrypt ? in_lens[order[i]] : bmseal::cbc_len(in_lens[order[i]]);
  if (bmseal::plan_slots(n, slots.data(), kSealSetRows, kSealSetPoolBytes, set.data(), off.data()) < 0)
    return set_err(BMPOW_E_ARG, "CBC plan refused");
  const Sets sets = cut_sets(set, off, slots);
  Shard& sh = g_shards[0];
  HIPTRY(hipSetDevice(sh.dev));
  CbcBufs b;
  const uint32_t cap_stride = round_up((uint32_t)sets.max_rows, SL_BLOCK);
  HIPTRY(b.pool.alloc(sh.dev, sets.max_pool));
  HIPTRY(b.keys.alloc(sh.dev, (size_t)2 * cap_stride));
  HIPTRY(b.iv.alloc(sh.dev, cap_stride));
  HIPTRY(b.rows.alloc(sh.dev, cap_stride));
  HIPTRY(b.out_len.alloc(sh.dev, cap_stride));
  for (Event& e : b.ev) HIPTRY(e.alloc(sh.dev));
  b.host.reset(new uint8_t[sets.max_pool]);
  b.host_bytes = sets.max_pool;
  uint8_t* hp = b.host.get();
  g_seal_stats.calls++;
  for (size_t k = 0; k + 1 < sets.begin.size(); ++k) {
    if (g_abort.load()) return set_err(BMPOW_E_ABORTED, "aborted");
    const size_t i0 = sets.begin[k], i1 = sets.begin[k + 1];
    const uint32_t m = (uint32_t)(i1 - i0), stride = round_up(m, SL_BLOCK);
    const uint64_t pool_bytes = off[i1 - 1] + slots[i1 - 1];
    auto t0 = std::chrono::steady_clock::now();
    b.hkeys.resize((size_t)32 * m);
    b.hiv.resize((size_t)16 * m);
    b.hrows.resize(m);
    b.hlen.resize(m);
    bmsched::parallel_for(m, 1024, [&](size_t a, size_t z) {
      for (size_t j = a; j < z; ++j) {
        const size_t row = order[i0 + j];
        b.hrows[j] = sl_row{(uint32_t)(off[i0 + j] / 16), (uint32_t)in_lens[row]};
        std::memcpy(b.hkeys.data() + 32 * j, keys + 32 * row, 32);
        std::memcpy(b.hiv.data() + 16 * j, ivs + 16 * row, 16);
        if (in_lens[row]) std::memcpy(hp + off[i0 + j], in[row], in_lens[row]);
      }
    });
    g_seal_stats.pack_ms += ms_since(t0);
    HIPTRY(hipEventRecord(b.ev[0].get(), sh.stream));
    HIPTRY(hipMemcpyAsync(b.pool.get(), hp, pool_bytes, hipMemcpyHostToDevice, sh.stream));
    HIPTRY(hipMemcpyAsync(b.keys.get(), b.hkeys.data(), (size_t)32 * m, hipMemcpyHostToDevice, sh.stream));
    HIPTRY(hipMemcpyAsync(b.iv.get(), b.hiv.data(), (size_t)16 * m, hipMemcpyHostToDevice, sh.stream));
    HIPTRY(hipMemcpyAsync(b.rows.get(), b.hrows.data(), m * sizeof(sl_row), hipMemcpyHostToDevice, sh.stream));
    HIPTRY(hipEventRecord(b.ev[1].get(), sh.stream));
    HIPTRY(sl_launch_cbc(sh.stream, decrypt, b.keys.get(), b.iv.get(), b.rows.get(), b.pool.get(), m, stride, b.out_len.get()));
    HIPTRY(hipEventRecord(b.ev[2].get(), sh.stream));
    HIPTRY(hipMemcpyAsync(hp, b.pool.get(), pool_bytes, hipMemcpyDeviceToHost, sh.stream));
    HIPTRY(hipMemcpyAsync(b.hlen.data(), b.out_len.get(), m * sizeof(int32_t), hipMemcpyDeviceToHost, sh.stream));
    HIPTRY(hipEventRecord(b.ev[3].get(), sh.stream));
    HIPTRY(hipStreamSynchronize(sh.stream));
    if (const int rc = elapsed(g_seal_stats.copy_ms, b.ev[0], b.ev[1]); rc < 0) return rc;
    if (const int rc = elapsed(g_seal_stats.seal_kernel_ms, b.ev[1], b.ev[2]); rc < 0) return rc;
    if (const int rc = elapsed(g_seal_stats.copy_ms, b.ev[2], b.ev[3]); rc < 0) return rc;
    t0 = std::chrono::steady_clock::now();
    std::atomic<bool> bad{false};
    bmsched::parallel_for(m, 1024, [&](size_t a, size_t z) {
      for (size_t j = a; j < z; ++j) {
        const size_t row = order[i0 + j];
        const int32_t l = b.hlen[j];
        if (l > (int64_t)slots[i0 + j]) {  // never: the kernel's lengths follow the host's
          bad.store(true);
          continue;
        }
        if (l > 0) std::memcpy(out[row], hp + off[i0 + j], (size_t)l);
        out_lens[row] = l < 0 ? -1 : l;
      }
    });
    g_seal_stats.scatter_ms += ms_since(t0);
    if (bad.load()) return set_err(BMPOW_E_HIP, "the CBC kernel returned a length above the slot");
    g_seal_stats.rows_device += m;
    g_seal_stats.sets++;
    g_seal_stats.launches++;
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
