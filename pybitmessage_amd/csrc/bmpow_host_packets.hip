// bmpow_host_packets.hip -- packet framing (include/bmpow_packets.h): the walk over the connection buffers'
// headers on host threads (bmpow_packets_fmt.h), the row plan, one upload of the raw bytes, the run of the
// packet kernels (bmpow_packets.hip) on shard 0's stream with the longest payloads hashed on host threads
// meanwhile, and the verdicts: per packet the reference's status, per `object` packet the intake's record
// (bmpow_host_intake.h: the same header walk and checks bmpow_intake_batch runs), per connection where the
// reference's state machine would stand.
#include "bmpow_host_intake.h"

#include <openssl/sha.h>

#include "../../include/bmpow_packets.h"
#include "bmpow_packets_fmt.h"
#include "bmpow_packets_kernels.h"

namespace bmhost {

using bmsched::Span;

constexpr uint64_t kPkStageBytes = 32ull << 20;  // pinned staging chunk (x2)
constexpr uint32_t kEmptySum = 0xcf83e135u;      // SHA512(b'')[:4]

// The call's buffers on shard 0 (grow-only, kept across calls, released with the shard set): the raw bytes go
// up through two pinned staging chunks, the copy into chunk c+1 overlapping the DMA of chunk c.
struct PacketShard {
  PinBuf<uint8_t> h_stage[2];
  Event ev_stage[2];
  DevBuf<uint4> d_arena, d_pool;
  PinBuf<pk_row> h_rows;
  DevBuf<pk_row> d_rows;
  DevBuf<bv_obj> d_obj;
  DevBuf<uint64_t> d_pow;
  PinBuf<uint64_t> h_pow;
  DevBuf<uint4> d_inv;  // 2 per object row
  PinBuf<uint8_t> h_inv;  // 32 per object row
  DevBuf<uint32_t> d_sum;  // per row
  PinBuf<uint32_t> h_sum;
  DevBuf<uint32_t> d_bins;
  Event ev[4];  // around pack, object, sum
};
std::unique_ptr<PacketShard> g_packets;
bmpow_packets_stats g_packets_stats{};  // under g_mu

void packets_release_shards() { g_packets.reset(); }

namespace {

using clk = std::chrono::steady_clock;
double ms_between(clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }

// hold n elements, with a quarter to spare when the buffer has to be made anew
template <class B>
hipError_t hold(B& b, int dev, size_t n, size_t least, unsigned flags = 0) {
  if (b && n <= b.cap()) return hipSuccess;
  return b.alloc(dev, std::max(n + n / 4, least), flags);
}

enum Kind : uint8_t { kNone, kEmpty, kObject, kSum, kHost };

// Arena bytes [o0, o1) from the buffers (base[c] = where buffer c starts; base[n_conn] = the arena's size).
void copy_range(size_t n_conn, const uint8_t* const* bufs, const std::vector<uint64_t>& base, uint64_t o0, uint64_t o1,
                uint8_t* dst) {
  size_t c = (size_t)(std::upper_bound(base.begin(), base.begin() + (ptrdiff_t)n_conn + 1, o0) - base.begin()) - 1;
  for (uint64_t o = o0; o < o1 && c < n_conn; ++c) {
    const uint64_t end = std::min(base[c + 1], o1);
    if (end > o) std::memcpy(dst + (o - o0), bufs[c] + (o - base[c]), end - o);
    o = std::max(o, end);
  }
}

// Hash and judge recs[0, n), framed from bufs (recs[i].conn, .offset): computed, the full status, and for the
// valid object packets the intake record under prm.  Under g_mu, devices initialised.
int run_recs_locked(size_t n_conn, const uint8_t* const* bufs, const std::vector<uint64_t>& base, bmpow_packet_rec* recs,
                    size_t n, const bmpow_intake_params* prm) {
  if (n == 0) return 0;
  if (g_abort.load()) return set_err(BMPOW_E_ABORTED, "aborted");  // process-wide, as for every other device call
  const int64_t now = prm->now ? prm->now : (int64_t)std::time(nullptr);
  const int64_t recv = prm->recv_time ? prm->recv_time : now;
  const uint64_t total = base[n_conn];
  auto payload = [&](const bmpow_packet_rec& r) { return bufs[r.conn] + r.offset + BMPOW_PKT_HEADER; };

  // which kernel, if any, hashes each packet; the objects' header walk
  const clk::time_point t0 = clk::now();
  static std::vector<uint8_t> kind;  // scratch kept across calls under g_mu
  static std::vector<uint32_t> obj_idx, sum_idx, host_idx;
  static std::vector<Span> obj_spans, sum_spans;
  static std::vector<bmsched::VPart> plan_o, plan_s;
  kind.resize(n);
  bmsched::parallel_for(n, 32768, [&](size_t a, size_t b) {
    for (size_t i = a; i < b; ++i) {
      bmpow_packet_rec& r = recs[i];
      std::memset(&r.intake, 0, sizeof(r.intake));
      if (r.status & BMPOW_PKT_TOO_LONG) {
        kind[i] = kNone;
        continue;
      }
      bool object = false;
      if (r.command == BMPOW_PKT_OBJECT && !(r.status & BMPOW_PKT_NOT_ESTABLISHED)) {
        if (!intake_header(payload(r), r.length, &r.intake))
          r.intake.status = BMPOW_INTAKE_MALFORMED;
        else if (r.length - r.intake.payload_offset > BMPOW_INTAKE_MAX_PAYLOAD)
          r.intake.status = BMPOW_INTAKE_TOO_LARGE;
        else
          object = true;
      }
      kind[i] = object ? kObject : r.length == 0 ? kEmpty : r.length > BMPOW_PKT_MAX_DEVICE ? kHost : kSum;
    }
  });
  obj_idx.clear(), sum_idx.clear(), host_idx.clear(), obj_spans.clear(), sum_spans.clear();
  uint64_t n_empty = 0;
  for (size_t i = 0; i < n; ++i) {
    switch (kind[i]) {
      case kObject: obj_idx.push_back((uint32_t)i), obj_spans.push_back({payload(recs[i]), recs[i].length}); break;
      // plan_verify reads a span's length only, as nonce || payload: the whole payload is this row's
      case kSum: sum_idx.push_back((uint32_t)i), sum_spans.push_back({nullptr, (uint64_t)recs[i].length + 8}); break;
      case kHost: host_idx.push_back((uint32_t)i); break;
      case kEmpty: recs[i].computed = kEmptySum, ++n_empty; break;
      default: break;
    }
  }
  const clk::time_point t1 = clk::now();
  g_packets_stats.host_frame_ms += ms_between(t0, t1);

  // the plan: each kind sorted by block count as the verification's parts are, the object rows' blocks first
  const size_t n_obj = obj_idx.size(), n_sum = sum_idx.size(), n_rows = n_obj + n_sum;
  uint64_t blocks_o = 0, blocks_s = 0;
  if (bmsched::plan_verify(obj_spans, 1, plan_o, blocks_o) < 0 || bmsched::plan_verify(sum_spans, 1, plan_s, blocks_s) < 0 ||
      blocks_o + blocks_s > 0xffffffffULL)
    return set_err(BMPOW_E_ARG, "too many packets or a payload pool above 2^32 blocks");
  Shard& sh = g_shards[0];
  if (!g_packets) g_packets.reset(new PacketShard());
  PacketShard& ps = *g_packets;
  const size_t nbins = 4 * (size_t)sh.cus;
  const bool binned = n_obj && verify_binned(n_obj, nbins);
  if (binned) bmsched::plan_bins(plan_o[0], nbins);
  HIPTRY(hipSetDevice(sh.dev));
  if (n_rows) {
    HIPTRY(hold(ps.h_rows, sh.dev, n_rows, 4096, hipHostMallocDefault));
    HIPTRY(hold(ps.d_rows, sh.dev, n_rows, 4096));
    HIPTRY(hold(ps.d_sum, sh.dev, n_rows, 4096));
    HIPTRY(hold(ps.h_sum, sh.dev, n_rows, 4096, hipHostMallocDefault));
    HIPTRY(hold(ps.d_obj, sh.dev, n_obj, 4096));
    HIPTRY(hold(ps.d_pow, sh.dev, n_obj, 4096));
    HIPTRY(hold(ps.h_pow, sh.dev, n_obj, 4096, hipHostMallocDefault));
    HIPTRY(hold(ps.d_inv, sh.dev, 2 * n_obj, 8192));
    HIPTRY(hold(ps.h_inv, sh.dev, 32 * n_obj, 32 * 4096, hipHostMallocDefault));
    HIPTRY(hold(ps.d_arena, sh.dev, (size_t)((total + 15) / 16 + 1), 4096));
    HIPTRY(hold(ps.d_pool, sh.dev, (size_t)(blocks_o + blocks_s) * 8, 4096));
    for (int c = 0; c < 2; ++c) {
      if (!ps.h_stage[c]) HIPTRY(ps.h_stage[c].alloc(sh.dev, kPkStageBytes, hipHostMallocDefault));
      if (!ps.ev_stage[c]) HIPTRY(ps.ev_stage[c].alloc(sh.dev, hipEventDisableTiming));
    }
    for (Event& e : ps.ev)
      if (!e) HIPTRY(e.alloc(sh.dev));
    pk_row* rows = ps.h_rows.get();
    auto fill = [&](const bmsched::VPart& pt, const std::vector<uint32_t>& idx, size_t row0, uint64_t blk0, uint32_t k) {
      bmsched::parallel_for(idx.size(), 65536, [&](size_t a, size_t b) {
        for (size_t j = a; j < b; ++j) {
          const bmpow_packet_rec& r = recs[idx[pt.orig[j]]];
          rows[row0 + j] = pk_row{(uint32_t)(base[r.conn] + r.offset + BMPOW_PKT_HEADER), r.length,
                                  (uint32_t)(blk0 + pt.ho[j].blk), k};
        }
      });
    };
    if (n_obj) fill(plan_o[0], obj_idx, 0, 0, PK_OBJECT);
    if (n_sum) fill(plan_s[0], sum_idx, n_obj, blocks_o, PK_SUM);
    // the raw bytes, chunk by chunk through the staging
    bool used[2] = {false, false};
    int c = 0;
    for (uint64_t o = 0; o < total; o += kPkStageBytes, c ^= 1) {
      const uint64_t sz = std::min(kPkStageBytes, total - o);
      if (used[c]) HIPTRY(hipEventSynchronize(ps.ev_stage[c].get()));  // its previous DMA is done
      uint8_t* dst = ps.h_stage[c].get();
      bmsched::parallel_for((size_t)sz, 1u << 20, [&](size_t a, size_t b) { copy_range(n_conn, bufs, base, o + a, o + b, dst + a); });
      HIPTRY(hipMemcpyAsync((uint8_t*)ps.d_arena.get() + o, dst, sz, hipMemcpyHostToDevice, sh.stream));
      HIPTRY(hipEventRecord(ps.ev_stage[c].get(), sh.stream));
      used[c] = true;
    }
    HIPTRY(hipMemcpyAsync(ps.d_rows.get(), rows, n_rows * sizeof(pk_row), hipMemcpyHostToDevice, sh.stream));
    if (binned) {
      const std::vector<uint32_t>& bins = plan_o[0].bins;
      HIPTRY(hold(ps.d_bins, sh.dev, bins.size(), 4096));
      HIPTRY(hipMemcpyAsync(ps.d_bins.get(), bins.data(), bins.size() * sizeof(uint32_t), hipMemcpyHostToDevice, sh.stream));
    }
  }
  const clk::time_point t2 = clk::now();
  g_packets_stats.host_build_ms += ms_between(t1, t2);

  // pack, object, sum on the shard's stream; the longest payloads on host threads meanwhile
  if (n_rows) {
    const uint64_t pool_blocks = blocks_o + blocks_s;
    HIPTRY(hipEventRecord(ps.ev[0].get(), sh.stream));
    HIPTRY(pk_launch_pack(sh.stream, ps.d_rows.get(), (uint32_t)n_rows, (uint32_t)n_obj, ps.d_arena.get(), total,
                          ps.d_pool.get(), pool_blocks, ps.d_obj.get()));
    HIPTRY(hipEventRecord(ps.ev[1].get(), sh.stream));
    if (binned)
      HIPTRY(pk_launch_object_binned(sh.stream, ps.d_rows.get(), ps.d_obj.get(), (uint32_t)n_obj, ps.d_pool.get(),
                                     pool_blocks, ps.d_pow.get(), ps.d_inv.get(), ps.d_sum.get(), ps.d_bins.get(),
                                     (uint32_t)nbins));
    else
      HIPTRY(pk_launch_object(sh.stream, ps.d_rows.get(), ps.d_obj.get(), (uint32_t)n_obj, ps.d_pool.get(), pool_blocks,
                              ps.d_pow.get(), ps.d_inv.get(), ps.d_sum.get()));
    HIPTRY(hipEventRecord(ps.ev[2].get(), sh.stream));
    HIPTRY(pk_launch_sum(sh.stream, ps.d_rows.get() + n_obj, (uint32_t)n_sum, ps.d_pool.get(), pool_blocks,
                         ps.d_sum.get() + n_obj));
    HIPTRY(hipEventRecord(ps.ev[3].get(), sh.stream));
    HIPTRY(hipMemcpyAsync(ps.h_sum.get(), ps.d_sum.get(), n_rows * sizeof(uint32_t), hipMemcpyDeviceToHost, sh.stream));
    if (n_obj) {
      HIPTRY(hipMemcpyAsync(ps.h_pow.get(), ps.d_pow.get(), n_obj * sizeof(uint64_t), hipMemcpyDeviceToHost, sh.stream));
      HIPTRY(hipMemcpyAsync(ps.h_inv.get(), ps.d_inv.get(), n_obj * 32, hipMemcpyDeviceToHost, sh.stream));
    }
  }
  bmsched::parallel_for(host_idx.size(), 1, [&](size_t a, size_t b) {
    for (size_t j = a; j < b; ++j) {
      bmpow_packet_rec& r = recs[host_idx[j]];
      uint8_t md[SHA512_DIGEST_LENGTH];
      SHA512(payload(r), r.length, md);
      r.computed = pkf::load_be32(md);
    }
  });
  if (n_rows) {
    HIPTRY(hipStreamSynchronize(sh.stream));
    double* const acc[3] = {&g_packets_stats.pack_ms, &g_packets_stats.object_ms, &g_packets_stats.sum_ms};
    if (const int rc = elapsed_phases(acc, ps.ev, 3); rc < 0) return rc;
  }
  const clk::time_point t3 = clk::now();
  g_packets_stats.host_run_ms += ms_between(t2, t3);

  // the results' way back, and the objects' verdicts exactly as bmpow_intake_batch reaches them
  auto good = [](bmpow_packet_rec& r) {
    if (r.computed != r.checksum) r.status |= BMPOW_PKT_BAD_CHECKSUM;  // :109-111
    return r.status == BMPOW_PKT_OK;
  };
  if (n_sum)
    bmsched::parallel_for(n_sum, 32768, [&](size_t a, size_t b) {
      for (size_t j = a; j < b; ++j) recs[sum_idx[plan_s[0].orig[j]]].computed = ps.h_sum[n_obj + j];
    });
  if (n_obj)
    bmsched::parallel_for(n_obj, 32768, [&](size_t a, size_t b) {
      for (size_t j = a; j < b; ++j) {
        bmpow_packet_rec& r = recs[obj_idx[plan_o[0].orig[j]]];
        r.computed = ps.h_sum[j];
        if (r.computed != r.checksum) continue;  // judged below
        r.intake.pow = ps.h_pow[j];
        std::memcpy(r.intake.inv, ps.h_inv.get() + 32 * j, 32);
        const int ok = bmsched::pow_sufficient(r.intake.pow, r.length, prm->ntpb, prm->extra, recv, r.intake.expires);
        r.intake.status = intake_status(&r.intake, r.length, ok, now, prm->streams, prm->n_streams);
      }
    });
  bmsched::parallel_for(n, 32768, [&](size_t a, size_t b) {
    for (size_t i = a; i < b; ++i)
      if (kind[i] != kNone && !good(recs[i])) std::memset(&recs[i].intake, 0, sizeof(recs[i].intake));
  });
  g_packets_stats.host_status_ms += ms_between(t3, clk::now());
  g_packets_stats.calls++;
  g_packets_stats.object_rows += n_obj;
  g_packets_stats.sum_rows += n_sum;
  g_packets_stats.host_rows += host_idx.size();
  g_packets_stats.empty_rows += n_empty;
  g_packets_stats.blocks += blocks_o + blocks_s;
  return 0;
}

int check_params(const bmpow_intake_params* prm) {
  if (!prm) return set_err(BMPOW_E_ARG, "null pointer");
  if (prm->n_streams && !prm->streams) return set_err(BMPOW_E_ARG, "null stream list");
  if (prm->ntpb >= (1ULL << 62) || prm->extra >= (1ULL << 62))
    return set_err(BMPOW_E_ARG, "nonceTrialsPerByte / payloadLengthExtraBytes above 2^62");
  return 0;
}

// base[c] = the arena offset of buffer c, base[n] = the arena's size (below 2^32)
int arena_of(size_t n, const uint8_t* const* bufs, const uint64_t* lens, std::vector<uint64_t>& base) {
  base.resize(n + 1);
  uint64_t total = 0;
  for (size_t c = 0; c < n; ++c) {
    if (lens[c] && !bufs[c]) return set_err(BMPOW_E_ARG, "null buffer pointer");
    base[c] = total;
    if (lens[c] >= (1ULL << 32) || (total += lens[c]) >= (1ULL << 32))
      return set_err(BMPOW_E_ARG, "the buffers hold 4 GiB or more in all");
  }
  base[n] = total;
  return 0;
}

}  // namespace

}  // namespace bmhost

using namespace bmhost;

extern "C" {

int64_t bmpow_packets_frame(const uint8_t* buf, uint64_t len, uint32_t conn_flags, bmpow_packet_rec* recs, size_t cap,
                            bmpow_packet_conn* conn) {
  if (!conn || (len && !buf) || (cap && !recs)) return set_err(BMPOW_E_ARG, "null pointer");
  if (len >= (1ULL << 32)) return set_err(BMPOW_E_ARG, "a buffer of 4 GiB or more");
  uint64_t consumed = 0, k = 0;
  uint32_t close = 0;
  const uint64_t n = pkf::walk(buf, len, conn_flags, (conn_flags & BMPOW_PKT_CONN_ALL) != 0, &consumed, &close,
                               [&](const bmpow_packet_rec& r) {
                                 if (k < cap) recs[k] = r;
                                 ++k;
                               });
  *conn = bmpow_packet_conn{consumed, 0, (uint32_t)n, close, 0};
  return (int64_t)n;
}

int64_t bmpow_packets_count(size_t n_conn, const uint8_t* const* bufs, const uint64_t* lens, const uint32_t* conn_flags) {
  if (n_conn == 0) return 0;
  if (!bufs || !lens || !conn_flags) return set_err(BMPOW_E_ARG, "null pointer");
  std::vector<uint64_t> base;
  if (const int rc = arena_of(n_conn, bufs, lens, base); rc < 0) return rc;
  std::atomic<uint64_t> total{0};
  bmsched::parallel_for(n_conn, 1, [&](size_t a, size_t b) {
    uint64_t n = 0, consumed;
    uint32_t close;
    for (size_t c = a; c < b; ++c) n += pkf::walk(bufs[c], lens[c], conn_flags[c], true, &consumed, &close, [](const bmpow_packet_rec&) {});
    total += n;
  });
  return (int64_t)total.load();
}

uint32_t bmpow_packets_row_blocks(int object, uint64_t len) {
  return len > 0xffffff00ULL ? 0u : pkf::row_blocks(object ? PK_OBJECT : PK_SUM, (uint32_t)len);
}

int64_t bmpow_packets_batch(size_t n_conn, const uint8_t* const* bufs, const uint64_t* lens, const uint32_t* conn_flags,
                            const bmpow_intake_params* prm, bmpow_packet_rec* recs, size_t cap, bmpow_packet_conn* conns) {
  std::lock_guard<FairMutex> lk(g_mu);
  int rc = init_locked();
  if (rc < 0) return rc;
  if (n_conn == 0) return 0;
  if (!bufs || !lens || !conn_flags || !conns || (cap && !recs)) return set_err(BMPOW_E_ARG, "null pointer");
  if ((rc = check_params(prm)) < 0) return rc;
  static std::vector<uint64_t> base;  // scratch kept across calls under g_mu
  if ((rc = arena_of(n_conn, bufs, lens, base)) < 0) return rc;
  // every packet that has all its bytes, whatever its checksum will say
  const clk::time_point t0 = clk::now();
  static std::vector<uint64_t> count;
  count.assign(n_conn, 0);
  auto walk_all = [&](size_t c, bmpow_packet_rec* out) {
    uint64_t consumed = 0, k = 0;
    uint32_t close = 0;
    const uint64_t n = pkf::walk(bufs[c], lens[c], conn_flags[c], true, &consumed, &close, [&](const bmpow_packet_rec& r) {
      if (!out) return;
      out[k] = r;
      out[k++].conn = (uint32_t)c;
    });
    if (out) conns[c].consumed = consumed, conns[c].close = close;
    return n;
  };
  bmsched::parallel_for(n_conn, 1, [&](size_t a, size_t b) {
    for (size_t c = a; c < b; ++c) count[c] = walk_all(c, nullptr);
  });
  uint64_t n = 0;
  for (size_t c = 0; c < n_conn; ++c) {
    conns[c] = bmpow_packet_conn{0, (uint32_t)n, (uint32_t)count[c], 0, 0};
    n += count[c];
  }
  if (n > cap) return set_err(BMPOW_E_ARG, "the record array holds fewer packets than the buffers frame");
  bmsched::parallel_for(n_conn, 1, [&](size_t a, size_t b) {
    for (size_t c = a; c < b; ++c) walk_all(c, recs + conns[c].first);
  });
  g_packets_stats.host_frame_ms += ms_between(t0, clk::now());
  if ((rc = run_recs_locked(n_conn, bufs, base, recs, (size_t)n, prm)) < 0) return rc;
  // where each connection stands: its records up to the first that closes it (:119-156), moved together
  const clk::time_point t1 = clk::now();
  uint64_t w = 0;
  for (size_t c = 0; c < n_conn; ++c) {
    bmpow_packet_conn& cn = conns[c];
    const bool datagram = (conn_flags[c] & BMPOW_PKT_CONN_DATAGRAM) != 0;
    const uint64_t first = cn.first, all = cn.count;
    cn.first = (uint32_t)w;
    uint64_t k = 0;
    while (k < all) {
      const bmpow_packet_rec& r = recs[first + k];
      if (w != first + k) recs[w] = r;
      ++w, ++k;
      const uint32_t end = pkf::after_packet(recs[w - 1], datagram);
      if (end == BMPOW_PKT_OPEN) continue;
      cn.close = end;
      cn.consumed = (uint64_t)recs[w - 1].offset + (end == BMPOW_PKT_HANDSHAKE ? BMPOW_PKT_HEADER + (uint64_t)recs[w - 1].length : 0);
      break;
    }
    cn.count = (uint32_t)k;
  }
  g_packets_stats.packets += w;
  g_packets_stats.host_status_ms += ms_between(t1, clk::now());
  return (int64_t)w;
}

int bmpow_packets_ack_batch(size_t n, const uint8_t* const* acks, const uint64_t* lens, const bmpow_intake_params* prm,
                            uint8_t* valid_out, bmpow_intake_rec* intake_out) {
  std::lock_guard<FairMutex> lk(g_mu);
  int rc = init_locked();
  if (rc < 0) return rc;
  if (n == 0) return 0;
  if (!acks || !lens || !valid_out) return set_err(BMPOW_E_ARG, "null pointer");
  if ((rc = check_params(prm)) < 0) return rc;
  static std::vector<uint64_t> base;  // scratch kept across calls under g_mu
  if ((rc = arena_of(n, acks, lens, base)) < 0) return rc;
  // class_objectProcessor.py:1022-1046: what needs no hash
  static std::vector<bmpow_packet_rec> recs;
  recs.clear();
  for (size_t i = 0; i < n; ++i) {
    valid_out[i] = 0;
    if (intake_out) std::memset(intake_out + i, 0, sizeof(*intake_out));
    if (lens[i] < BMPOW_PKT_HEADER || pkf::load_be32(acks[i]) != BMPOW_PKT_MAGIC) continue;
    bmpow_packet_rec r{};
    r.conn = (uint32_t)i;
    pkf::header_into(acks[i], true, &r);
    if (r.length != lens[i] - BMPOW_PKT_HEADER || r.status != BMPOW_PKT_OK) continue;
    recs.push_back(r);
  }
  if ((rc = run_recs_locked(n, acks, base, recs.data(), recs.size(), prm)) < 0) return rc;
  for (const bmpow_packet_rec& r : recs) {
    // :1048-1053: the checksum, then the command in exactly the spelling "object"
    if (r.status != BMPOW_PKT_OK || r.command != BMPOW_PKT_OBJECT || !r.exact) continue;
    valid_out[r.conn] = 1;
    if (intake_out) intake_out[r.conn] = r.intake;
  }
  g_packets_stats.packets += recs.size();
  return 0;
}

int bmpow_packets_get_stats(bmpow_packets_stats* out) {
  if (!out) return set_err(BMPOW_E_ARG, "null pointer");
  std::lock_guard<FairMutex> lk(g_mu);
  *out = g_packets_stats;
  return 0;
}

void bmpow_packets_reset_stats(void) {
  std::lock_guard<FairMutex> lk(g_mu);
  g_packets_stats = bmpow_packets_stats{};
}

}  // extern "C"
