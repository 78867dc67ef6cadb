// bmpow_host_proc.hip -- the object processor's dispatch (include/bmpow_proc.h): the dispatcher object with the
// host-authoritative watch set and my addresses, their flattening into the tables of bmpow_proc_fmt.h and the
// upload where they changed, the O(1)-per-object plan of what a batch uploads, the round trip of the proc_*
// kernels (bmpow_proc.hip) on shard 0's stream, the scatter of the device rows back to input order, and the
// host-only walk.
#include "bmpow_host.h"

#include <map>
#include <random>
#include <unordered_map>

#include "../../include/bmpow_proc.h"
#include "bmpow_proc_fmt.h"
#include "bmpow_proc_kernels.h"

static_assert(sizeof(pc_rec) == sizeof(bmpow_proc_rec) && sizeof(pc_rec) == 72, "the record's layout");
static_assert(offsetof(pc_rec, status) == offsetof(bmpow_proc_rec, status) &&
                  offsetof(pc_rec, host_class) == offsetof(bmpow_proc_rec, host_class) &&
                  offsetof(pc_rec, ack_first) == offsetof(bmpow_proc_rec, ack_first),
              "the record's layout");
static_assert(sizeof(pc_addr) == sizeof(bmpow_proc_address) && sizeof(pc_addr) == 80 &&
                  offsetof(pc_addr, stream) == offsetof(bmpow_proc_address, stream) &&
                  offsetof(pc_addr, chan) == offsetof(bmpow_proc_address, chan),
              "the address row's layout");
static_assert(PC_ROUTE_UNKNOWN_TYPE == BMPOW_PROC_ROUTE_UNKNOWN_TYPE && PC_ROUTE_ONIONPEER == BMPOW_PROC_ROUTE_ONIONPEER &&
                  PC_ACK_FOUND_EARLIER == BMPOW_PROC_ACK_FOUND_EARLIER && PC_ACK_NOT_WATCHED == BMPOW_PROC_ACK_NOT_WATCHED &&
                  PC_TOO_LONG == BMPOW_PROC_TOO_LONG && PC_MALFORMED == BMPOW_PROC_MALFORMED &&
                  PC_SHORT_TAG == BMPOW_PROC_SHORT_TAG && PC_SENT_RECENTLY == BMPOW_PROC_SENT_RECENTLY &&
                  PC_SEND_V2 == BMPOW_PROC_SEND_V2 && PC_SEND_V4 == BMPOW_PROC_SEND_V4 && PC_NO_HOST == BMPOW_PROC_NO_HOST &&
                  PC_RAISES == BMPOW_PROC_RAISES && PC_PEER == BMPOW_PROC_PEER && PC_HOST_V6 == BMPOW_PROC_HOST_V6 &&
                  PC_NONE == BMPOW_PROC_NO_ROW,
              "the record's values");

// One dispatcher.  Every field under g_mu.
struct bmpow_proc {
  uint64_t generation = ~0ULL;  // g_generation of the shard set the tables were allocated under
  int dev = -1;
  bool host_only = false;
  uint64_t seed = 0;
  // the authoritative copies
  std::unordered_map<std::string, uint32_t> watch;  // key -> aux
  std::map<uint32_t, uint64_t> lengths;             // key length -> keys of that length
  std::vector<pc_addr> addrs;
  bool watch_dirty = true, addrs_dirty = true;  // changed since the last upload
  // what the device holds: the watch set flattened in flat's order, the address rows and their indexes
  std::vector<std::string> flat;
  uint32_t w_log2 = 3, a_log2 = 1;
  uint64_t w_pool_bytes = 0;
  bmown::DevBuf<uint64_t> d_tags, d_kpool;
  bmown::DevBuf<uint32_t> d_slot_entry, d_first, d_by_ripe, d_by_tag;
  bmown::DevBuf<pcf::pc_entry> d_entries;
  bmown::DevBuf<pc_addr> d_addrs;
  bmpow_proc_stats st{};
};

namespace bmhost {

constexpr uint64_t kProcMaxRows = 1ull << 30;
constexpr uint32_t kProcRowsPerLaunch = 1u << 20;

// The calls' buffers on shard 0 (grow-only, kept across calls, released with the shard set).
struct ProcScratch {
  DevBuf<uint64_t> d_pool;  // the uploaded object bytes, whole words
  DevBuf<pc_row> d_rows;
  DevBuf<uint32_t> d_ack_entry;
  DevBuf<pc_ack> d_ack;
  DevBuf<pc_rec> d_recs;
  Event ev[3];
};
std::unique_ptr<ProcScratch> g_proc;

void proc_release_shards() { g_proc.reset(); }

namespace {

using clk = std::chrono::steady_clock;
double ms_since(clk::time_point a) { return std::chrono::duration<double, std::milli>(clk::now() - a).count(); }

template <class B>
hipError_t hold(B& b, int dev, size_t n) {
  if (b && n <= b.cap()) return hipSuccess;
  return b.alloc(dev, std::max(n + n / 4, (size_t)1024));
}

// Under g_mu: a device dispatcher is of this shard set (devices initialised first); a host-only one always is.
int check_proc(const bmpow_proc* d) {
  if (!d) return set_err(BMPOW_E_ARG, "null dispatcher");
  if (d->host_only) return 0;
  if (const int rc = init_locked(); rc < 0) return rc;
  if (d->generation != g_generation || g_shards.empty() || d->dev != g_shards[0].dev)
    return set_err(BMPOW_E_STATE, "device set changed under a live dispatcher");
  return 0;
}

// keys[offs[i] .. offs[i + 1]) as n strings' bounds, checked
int check_keys(size_t n, const uint8_t* keys, const uint64_t* offs) {
  if (n == 0) return 0;
  if (!offs) return set_err(BMPOW_E_ARG, "null pointer");
  for (size_t i = 0; i < n; ++i) {
    if (offs[i + 1] < offs[i] || offs[i + 1] - offs[i] >= (1ull << 31)) return set_err(BMPOW_E_ARG, "key offsets out of order, or a key of 2 GiB or more");
    if (offs[i + 1] > offs[i] && !keys) return set_err(BMPOW_E_ARG, "null pointer");
  }
  return 0;
}
std::string key_at(const uint8_t* keys, const uint64_t* offs, size_t i) {
  return offs[i + 1] > offs[i] ? std::string(reinterpret_cast<const char*>(keys + offs[i]), (size_t)(offs[i + 1] - offs[i])) : std::string();
}

void drop_key(bmpow_proc& d, std::unordered_map<std::string, uint32_t>::iterator it) {
  const uint32_t len = (uint32_t)it->first.size();
  auto l = d.lengths.find(len);
  if (l != d.lengths.end() && --l->second == 0) d.lengths.erase(l);
  d.watch.erase(it);
  d.watch_dirty = true;
}

// The watch set flattened and uploaded: the keys back to back, the entries, and the index built by the probe
// rule of pcf::watch_find.
int upload_watch(bmpow_proc& d, hipStream_t stream) {
  static std::vector<uint64_t> tags, pool;  // scratch kept across calls under g_mu
  static std::vector<uint32_t> slot_entry;
  static std::vector<pcf::pc_entry> entries;
  const size_t n = d.watch.size();
  d.flat.clear();
  d.flat.reserve(n);
  uint64_t bytes = 0;
  for (const auto& kv : d.watch) {
    d.flat.push_back(kv.first);
    bytes += kv.first.size();
  }
  if (bytes >= (1ull << 32) || n >= (1ull << 30)) return set_err(BMPOW_E_ARG, "a watch set of 4 GiB of keys or 2^30 keys or more");
  d.w_log2 = pcf::watch_log2_for(n);
  d.w_pool_bytes = bytes;
  if (n == 0) {
    d.watch_dirty = false;
    return 0;
  }
  const uint32_t slots = 1u << d.w_log2;
  tags.assign(slots, 0), slot_entry.assign(slots, PC_NONE), entries.resize(n), pool.assign((size_t)((bytes + 7) / 8) + 1, 0);
  uint8_t* pb = reinterpret_cast<uint8_t*>(pool.data());
  uint32_t at = 0;
  for (size_t e = 0; e < n; ++e) {
    const std::string& k = d.flat[e];
    if (!k.empty()) std::memcpy(pb + at, k.data(), k.size());
    entries[e] = pcf::pc_entry{at, (uint32_t)k.size(), d.watch[k]};
    at += (uint32_t)k.size();
    const uint64_t mix = pcf::watch_mix_of(d.seed, reinterpret_cast<const uint8_t*>(k.data()), (uint32_t)k.size());
    pcf::watch_place(tags.data(), slot_entry.data(), d.w_log2, mix, (uint32_t)e);
  }
  HIPTRY(hold(d.d_tags, d.dev, slots));
  HIPTRY(hold(d.d_slot_entry, d.dev, slots));
  HIPTRY(hold(d.d_entries, d.dev, n));
  HIPTRY(hold(d.d_first, d.dev, n));
  HIPTRY(hold(d.d_kpool, d.dev, pool.size()));
  HIPTRY(hipMemcpyAsync(d.d_tags.get(), tags.data(), slots * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
  HIPTRY(hipMemcpyAsync(d.d_slot_entry.get(), slot_entry.data(), slots * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
  HIPTRY(hipMemcpyAsync(d.d_entries.get(), entries.data(), n * sizeof(pcf::pc_entry), hipMemcpyHostToDevice, stream));
  HIPTRY(hipMemcpyAsync(d.d_kpool.get(), pool.data(), pool.size() * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
  HIPTRY(hipStreamSynchronize(stream));  // the statics above are the next upload's as well
  d.watch_dirty = false;
  d.st.table_uploads++;
  return 0;
}

int upload_addrs(bmpow_proc& d, hipStream_t stream) {
  static std::vector<uint32_t> by_ripe, by_tag;  // scratch kept across calls under g_mu
  const uint32_t n = (uint32_t)d.addrs.size();
  d.a_log2 = pcf::addr_log2_for(n);
  if (n == 0) {
    d.addrs_dirty = false;
    return 0;
  }
  const uint32_t slots = 1u << d.a_log2;
  by_ripe.resize(slots), by_tag.resize(slots);
  if (!pcf::fill_index(d.addrs.data(), n, d.a_log2, by_ripe.data(), by_tag.data()))
    return set_err(BMPOW_E_STATE, "two address rows with one ripe or tag");  // never: set_addresses refused them
  HIPTRY(hold(d.d_addrs, d.dev, n));
  HIPTRY(hold(d.d_by_ripe, d.dev, slots));
  HIPTRY(hold(d.d_by_tag, d.dev, slots));
  HIPTRY(hipMemcpyAsync(d.d_addrs.get(), d.addrs.data(), n * sizeof(pc_addr), hipMemcpyHostToDevice, stream));
  HIPTRY(hipMemcpyAsync(d.d_by_ripe.get(), by_ripe.data(), slots * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
  HIPTRY(hipMemcpyAsync(d.d_by_tag.get(), by_tag.data(), slots * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
  HIPTRY(hipStreamSynchronize(stream));
  d.addrs_dirty = false;
  d.st.table_uploads++;
  return 0;
}

uint32_t route_of(uint32_t type) {
  return type <= 3 ? type : type == PC_TYPE_ONIONPEER ? (uint32_t)PC_ROUTE_ONIONPEER : (uint32_t)PC_ROUTE_UNKNOWN_TYPE;
}

pc_rec blank(uint32_t type) {
  pc_rec r{};
  r.route = route_of(type);
  r.ack = PC_ACK_NOT_CHECKED;
  r.ack_first = r.address = PC_NONE;
  return r;
}

// the verdict fields of a walked row into the object's record (route and the ack fields stay)
void take_verdict(pc_rec& to, const pc_rec& from) {
  to.version = from.version, to.stream = from.stream, to.port = from.port;
  to.status = from.status, to.key_off = from.key_off, to.key_len = from.key_len, to.address = from.address;
  to.host_off = from.host_off, to.host_len = from.host_len, to.host_class = from.host_class;
}

int64_t clock_now() { return (int64_t)std::time(nullptr); }

}  // namespace

}  // namespace bmhost

using namespace bmhost;

extern "C" {

bmpow_proc* bmpow_proc_create(uint64_t seed, int host_only) {
  std::lock_guard<FairMutex> lk(g_mu);
  if (!host_only && init_locked() < 0) return nullptr;
  std::unique_ptr<bmpow_proc> d(new bmpow_proc());
  while (seed == 0) {
    std::random_device rd;
    seed = ((uint64_t)rd() << 32) | rd();
  }
  d->seed = seed;
  d->host_only = host_only != 0;
  if (!host_only) {
    d->generation = g_generation;
    d->dev = g_shards[0].dev;
  }
  return d.release();
}

void bmpow_proc_destroy(bmpow_proc* d) {
  if (!d) return;
  std::lock_guard<FairMutex> lk(g_mu);
  // of the live shard set: whatever the stream still runs on the tables ends first
  if (!d->host_only && d->generation == g_generation && !g_shards.empty() && hipSetDevice(g_shards[0].dev) == hipSuccess)
    (void)hipStreamSynchronize(g_shards[0].stream);
  delete d;
}

int bmpow_proc_stats_get(bmpow_proc* d, bmpow_proc_stats* out) {
  if (!out) return set_err(BMPOW_E_ARG, "null pointer");
  std::lock_guard<FairMutex> lk(g_mu);
  if (const int rc = check_proc(d); rc < 0) return rc;
  *out = d->st;
  out->seed = d->seed;
  out->watch_len = d->watch.size();
  out->watch_slots = 1ull << pcf::watch_log2_for(d->watch.size());
  out->watch_lengths = d->lengths.size();
  out->addresses = d->addrs.size();
  return 0;
}

int bmpow_proc_stats_reset(bmpow_proc* d) {
  std::lock_guard<FairMutex> lk(g_mu);
  if (const int rc = check_proc(d); rc < 0) return rc;
  d->st = bmpow_proc_stats{};
  return 0;
}

int bmpow_proc_watch_add(bmpow_proc* d, size_t n, const uint8_t* keys, const uint64_t* offs, const uint32_t* aux,
                         uint8_t* added_out) {
  std::lock_guard<FairMutex> lk(g_mu);
  int rc = check_proc(d);
  if (rc < 0 || (rc = check_keys(n, keys, offs)) < 0) return rc;
  for (size_t i = 0; i < n; ++i) {
    const auto ins = d->watch.insert_or_assign(key_at(keys, offs, i), aux ? aux[i] : 0u);
    if (ins.second) d->lengths[(uint32_t)ins.first->first.size()]++;
    if (added_out) added_out[i] = ins.second;
  }
  if (n) d->watch_dirty = true;
  return 0;
}

int bmpow_proc_watch_discard(bmpow_proc* d, size_t n, const uint8_t* keys, const uint64_t* offs, uint8_t* present_out) {
  std::lock_guard<FairMutex> lk(g_mu);
  int rc = check_proc(d);
  if (rc < 0 || (rc = check_keys(n, keys, offs)) < 0) return rc;
  for (size_t i = 0; i < n; ++i) {
    const auto it = d->watch.find(key_at(keys, offs, i));
    if (present_out) present_out[i] = it != d->watch.end();
    if (it != d->watch.end()) drop_key(*d, it);
  }
  return 0;
}

int bmpow_proc_watch_contains(bmpow_proc* d, size_t n, const uint8_t* keys, const uint64_t* offs, uint8_t* present_out,
                              uint32_t* aux_out) {
  std::lock_guard<FairMutex> lk(g_mu);
  int rc = check_proc(d);
  if (rc < 0 || (rc = check_keys(n, keys, offs)) < 0) return rc;
  if (n && !present_out) return set_err(BMPOW_E_ARG, "null pointer");
  for (size_t i = 0; i < n; ++i) {
    const auto it = d->watch.find(key_at(keys, offs, i));
    present_out[i] = it != d->watch.end();
    if (aux_out) aux_out[i] = it != d->watch.end() ? it->second : 0u;
  }
  return 0;
}

int64_t bmpow_proc_watch_len(bmpow_proc* d) {
  std::lock_guard<FairMutex> lk(g_mu);
  if (const int rc = check_proc(d); rc < 0) return rc;
  return (int64_t)d->watch.size();
}

int bmpow_proc_watch_clear(bmpow_proc* d) {
  std::lock_guard<FairMutex> lk(g_mu);
  if (const int rc = check_proc(d); rc < 0) return rc;
  d->watch.clear(), d->lengths.clear();
  d->watch_dirty = true;
  return 0;
}

uint64_t bmpow_proc_watch_slot(uint64_t seed, uint32_t log2_slots, const uint8_t* key, size_t len) {
  if ((len && !key) || log2_slots < 3 || log2_slots > 31 || len >= (1ull << 31)) return 0;
  return pcf::watch_slot(pcf::watch_mix_of(seed, key, (uint32_t)len), log2_slots);
}

int bmpow_proc_set_addresses(bmpow_proc* d, size_t n, const bmpow_proc_address* rows) {
  std::lock_guard<FairMutex> lk(g_mu);
  if (const int rc = check_proc(d); rc < 0) return rc;
  if (n && !rows) return set_err(BMPOW_E_ARG, "null pointer");
  if (n >= (1ull << 24)) return set_err(BMPOW_E_ARG, "2^24 addresses or more");
  std::vector<pc_addr> next(n);
  if (n) std::memcpy(next.data(), rows, n * sizeof(pc_addr));
  for (pc_addr& a : next) {
    if (a.chan > 1) return set_err(BMPOW_E_ARG, "chan is 0 or 1");
    a.reserved = 0;
  }
  const uint32_t log2 = pcf::addr_log2_for((uint32_t)n);
  std::vector<uint32_t> by_ripe(1u << log2), by_tag(1u << log2);
  if (!pcf::fill_index(next.data(), (uint32_t)n, log2, by_ripe.data(), by_tag.data()))
    return set_err(BMPOW_E_ARG, "two address rows with one ripe or one tag");
  d->addrs.swap(next);
  d->addrs_dirty = true;
  return 0;
}

int bmpow_proc_walk(uint32_t type, const uint8_t* obj, uint64_t len, size_t n_addresses, const bmpow_proc_address* addresses,
                    int64_t now, bmpow_proc_rec* rec_out) {
  if (!rec_out || (len && !obj) || (n_addresses && !addresses)) return set_err(BMPOW_E_ARG, "null pointer");
  if (len >= (1ull << 32)) return set_err(BMPOW_E_ARG, "an object of 4 GiB or more");
  if (n_addresses >= (1ull << 24)) return set_err(BMPOW_E_ARG, "2^24 addresses or more");
  pc_rec r = blank(type);
  uint64_t head[PC_GETPUBKEY_MAX / 8 + 1] = {0};  // the bytes a verdict can depend on, aligned as the pool is
  if (r.route == PC_ROUTE_GETPUBKEY) {
    const uint32_t avail = len > PC_GETPUBKEY_MAX ? 0 : (uint32_t)len;
    if (avail) std::memcpy(head, obj, avail);
    std::vector<pc_addr> rows(n_addresses);
    if (n_addresses) std::memcpy(rows.data(), addresses, n_addresses * sizeof(pc_addr));
    const uint32_t log2 = pcf::addr_log2_for((uint32_t)n_addresses);
    std::vector<uint32_t> by_ripe(1u << log2), by_tag(1u << log2);
    if (!pcf::fill_index(rows.data(), (uint32_t)n_addresses, log2, by_ripe.data(), by_tag.data()))
      return set_err(BMPOW_E_ARG, "two address rows with one ripe or one tag");
    const pcf::AddrTable t{rows.data(), by_ripe.data(), by_tag.data(), (uint32_t)n_addresses, log2};
    pcf::walk_getpubkey(pcf::Bytes{head, avail, 0, avail, (uint32_t)len}, t, now ? now : clock_now(), &r);
  } else if (r.route == PC_ROUTE_ONIONPEER) {
    const uint32_t avail = (uint32_t)std::min<uint64_t>(len, PC_ONION_HEAD);
    if (avail) std::memcpy(head, obj, avail);
    pcf::walk_onion(pcf::Bytes{head, avail, 0, avail, (uint32_t)len}, &r);
  }
  std::memcpy(rec_out, &r, sizeof(r));
  return 0;
}

int bmpow_proc_batch(bmpow_proc* d, size_t n, const uint8_t* const* objs, const uint64_t* lens, const uint32_t* types,
                     const bmpow_proc_params* params, bmpow_proc_rec* recs_out) {
  std::lock_guard<FairMutex> lk(g_mu);
  int rc = check_proc(d);
  if (rc < 0) return rc;
  if (d->host_only) return set_err(BMPOW_E_STATE, "a host-only dispatcher has no device to run a batch on");
  if (g_abort.load()) return set_err(BMPOW_E_ABORTED, "aborted");
  if (n == 0) return 0;
  if (!objs || !lens || !types || !recs_out) return set_err(BMPOW_E_ARG, "null pointer");
  if (n > kProcMaxRows) return set_err(BMPOW_E_ARG, "more than 2^30 objects");
  const clk::time_point t0 = clk::now();
  const int64_t now = params && params->now ? params->now : clock_now();
  const uint32_t per_launch = params && params->rows_per_launch ? params->rows_per_launch : kProcRowsPerLaunch;

  // the plan: O(1) per object.  Rows by class, each with the bytes a verdict can depend on.
  static std::vector<uint32_t> src[3];  // scratch kept across calls under g_mu
  static std::vector<pc_row> rows;
  static std::vector<uint64_t> staged;
  static std::vector<pc_ack> h_ack;
  static std::vector<pc_rec> h_recs;
  static std::vector<uint32_t> h_first;
  for (auto& v : src) v.clear();
  pc_rec* out = reinterpret_cast<pc_rec*>(recs_out);
  for (size_t i = 0; i < n; ++i) {
    if ((lens[i] && !objs[i]) || lens[i] >= (1ull << 32)) return set_err(BMPOW_E_ARG, "a null object or one of 4 GiB or more");
    pc_rec r = blank(types[i]);
    if (lens[i] >= 32) {  // checkackdata :133-139
      r.ack = PC_ACK_NOT_WATCHED;
      if (d->lengths.count((uint32_t)(lens[i] - 16))) src[PC_ROW_ACK].push_back((uint32_t)i);
    }
    if (r.route == PC_ROUTE_GETPUBKEY) {
      if (lens[i] > PC_GETPUBKEY_MAX) r.status = PC_TOO_LONG;  // :179-182, before any byte is read
      else src[PC_ROW_GETPUBKEY].push_back((uint32_t)i);
    } else if (r.route == PC_ROUTE_ONIONPEER) {
      src[PC_ROW_ONION].push_back((uint32_t)i);
    }
    out[i] = r;
  }
  const size_t n_ack = src[0].size(), n_rows = n_ack + src[1].size() + src[2].size();
  d->st.calls++, d->st.rows += n;
  if (n_rows == 0) {
    d->st.host_ms += ms_since(t0);
    return 0;
  }
  rows.resize(n_rows);
  uint64_t total = 0;
  {
    size_t r = 0;
    for (uint32_t kind = 0; kind < 3; ++kind)
      for (const uint32_t i : src[kind]) {
        const uint64_t len = lens[i];
        const uint64_t piece = kind == PC_ROW_ACK ? len - 16 : kind == PC_ROW_GETPUBKEY ? len : std::min<uint64_t>(len, PC_ONION_HEAD);
        if (total + piece >= (1ull << 32)) return set_err(BMPOW_E_ARG, "the batch uploads 4 GiB or more");
        rows[r++] = pc_row{(uint32_t)total, (uint32_t)piece, (uint32_t)(kind == PC_ROW_ACK ? len - 16 : len), kind};
        total += piece;
      }
  }
  staged.assign((size_t)((total + 7) / 8) + 1, 0);  // pieces back to back, no padding between them
  {
    uint8_t* pb = reinterpret_cast<uint8_t*>(staged.data());
    size_t r = 0;
    for (uint32_t kind = 0; kind < 3; ++kind)
      for (const uint32_t i : src[kind]) {
        if (rows[r].avail) std::memcpy(pb + rows[r].off, objs[i] + (kind == PC_ROW_ACK ? 16 : 0), rows[r].avail);
        ++r;
      }
  }

  Shard& sh = g_shards[0];
  HIPTRY(hipSetDevice(sh.dev));
  if (!g_proc) g_proc.reset(new ProcScratch());
  ProcScratch& sc = *g_proc;
  for (Event& e : sc.ev)
    if (!e) HIPTRY(e.alloc(sh.dev));
  if (d->watch_dirty && (rc = upload_watch(*d, sh.stream)) < 0) return rc;
  if (d->addrs_dirty && (rc = upload_addrs(*d, sh.stream)) < 0) return rc;
  const uint32_t w_n = (uint32_t)d->flat.size(), a_n = (uint32_t)d->addrs.size();
  if (n_ack && w_n == 0) return set_err(BMPOW_E_STATE, "ack candidates against an empty watch set");  // never
  HIPTRY(hold(sc.d_pool, sh.dev, staged.size()));
  HIPTRY(hold(sc.d_rows, sh.dev, n_rows));
  HIPTRY(hold(sc.d_ack_entry, sh.dev, std::max(n_ack, (size_t)1)));
  HIPTRY(hold(sc.d_ack, sh.dev, std::max(n_ack, (size_t)1)));
  HIPTRY(hold(sc.d_recs, sh.dev, std::max(n_rows - n_ack, (size_t)1)));
  HIPTRY(hipMemcpyAsync(sc.d_pool.get(), staged.data(), staged.size() * sizeof(uint64_t), hipMemcpyHostToDevice, sh.stream));
  HIPTRY(hipMemcpyAsync(sc.d_rows.get(), rows.data(), n_rows * sizeof(pc_row), hipMemcpyHostToDevice, sh.stream));
  if (w_n) HIPTRY(hipMemsetAsync(d->d_first.get(), 0xff, w_n * sizeof(uint32_t), sh.stream));  // per call; kept across its launches

  pc_call c{};
  c.pool = sc.d_pool.get(), c.pool_bytes = total;
  c.rows = sc.d_rows.get(), c.n_rows = (uint32_t)n_rows, c.n_ack = (uint32_t)n_ack;
  if (w_n)
    c.watch = pcf::WatchTable{d->d_tags.get(), d->d_slot_entry.get(), d->d_entries.get(), d->d_kpool.get(), d->w_pool_bytes,
                              d->seed, w_n, d->w_log2};
  if (a_n) c.addrs = pcf::AddrTable{d->d_addrs.get(), d->d_by_ripe.get(), d->d_by_tag.get(), a_n, d->a_log2};
  c.now = now;
  c.first = w_n ? d->d_first.get() : nullptr;
  c.ack_entry = sc.d_ack_entry.get();
  c.recs = sc.d_recs.get();

  HIPTRY(hipEventRecord(sc.ev[0].get(), sh.stream));
  for (uint64_t begin = 0; begin < n_rows; begin += per_launch) {
    HIPTRY(pc_launch_rows(sh.stream, c, (uint32_t)begin, (uint32_t)std::min<uint64_t>(begin + per_launch, n_rows)));
    d->st.launches++;
  }
  HIPTRY(hipEventRecord(sc.ev[1].get(), sh.stream));
  if (n_ack) {
    HIPTRY(pc_launch_ack_finish(sh.stream, c, sc.d_ack.get()));
    d->st.launches++;
  }
  HIPTRY(hipEventRecord(sc.ev[2].get(), sh.stream));
  h_ack.resize(n_ack), h_recs.resize(n_rows - n_ack), h_first.resize(w_n);
  if (n_ack) {
    HIPTRY(hipMemcpyAsync(h_ack.data(), sc.d_ack.get(), n_ack * sizeof(pc_ack), hipMemcpyDeviceToHost, sh.stream));
    HIPTRY(hipMemcpyAsync(h_first.data(), d->d_first.get(), w_n * sizeof(uint32_t), hipMemcpyDeviceToHost, sh.stream));
  }
  if (n_rows > n_ack)
    HIPTRY(hipMemcpyAsync(h_recs.data(), sc.d_recs.get(), (n_rows - n_ack) * sizeof(pc_rec), hipMemcpyDeviceToHost, sh.stream));
  HIPTRY(hipStreamSynchronize(sh.stream));
  double* const acc[2] = {&d->st.rows_ms, &d->st.finish_ms};
  if ((rc = elapsed_phases(acc, sc.ev, 2)) < 0) return rc;

  // the scatter back to input order
  for (size_t r = 0; r < n_ack; ++r) {
    pc_rec& o = out[src[0][r]];
    const pc_ack& a = h_ack[r];
    if (a.state != PC_ACK_FOUND && a.state != PC_ACK_FOUND_EARLIER) continue;
    o.ack = a.state, o.ack_aux = a.aux;
    o.ack_first = a.first < n_ack ? src[0][a.first] : src[0][r];
  }
  {
    size_t r = 0;
    for (uint32_t kind = 1; kind < 3; ++kind)
      for (const uint32_t i : src[kind]) take_verdict(out[i], h_recs[r++]);
  }
  // the FOUND keys leave the watch set (del state.ackdataForWhichImWatching[...], :141)
  if (n_ack)
    for (uint32_t e = 0; e < w_n; ++e)
      if (h_first[e] != PC_NONE) {
        const auto it = d->watch.find(d->flat[e]);
        if (it != d->watch.end()) drop_key(*d, it), d->st.found++;
      }
  d->st.rows_uploaded += n_rows, d->st.ack_rows += n_ack, d->st.bytes_uploaded += total;
  d->st.host_ms += ms_since(t0);
  return 0;
}

}  // extern "C"
