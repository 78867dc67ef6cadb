// bmpow_host_inv.hip -- the device-resident inventory sets (include/bmpow_inv.h): the sets' tables on shard 0's
// device, the load bound and the rebuilds that keep it (grow, tombstone purge, sweep), the round trips of the
// iv_* kernels (bmpow_inv.hip) on shard 0's stream, the walk of `inv` / `dinv` / `getdata` payloads on the host
// (bmpow_inv_fmt.h) with one upload of the payloads as they are, and the step behind the intake's records.
#include "bmpow_host.h"

#include <random>

#include "../../include/bmpow_inv.h"
#include "bmpow_inv_fmt.h"
#include "bmpow_inv_kernels.h"

// One set: its table (owners free on the set's own device, whatever the shard set looks like by then), what it
// holds and its counters.  Every field under g_mu.
struct bmpow_invset {
  uint64_t generation = ~0ULL;  // g_generation of the shard set the table was allocated under
  int dev = -1;
  uint64_t seed = 0;
  uint32_t log2 = 0;
  bmown::DevBuf<uint64_t> d_state, d_keys;
  bmown::DevBuf<iv_val> d_vals;
  uint64_t live = 0, tombs = 0;
  bmpow_inv_stats st{};
};

namespace bmhost {

constexpr uint32_t kMinLog2 = 3, kMaxLog2 = 30;
constexpr uint64_t kMaxRows = 1ull << 30;

// The calls' buffers on shard 0 (grow-only, kept across calls, released with the shard set).
struct InvScratch {
  DevBuf<uint64_t> d_in;  // the uploaded bytes, whole words
  DevBuf<uint32_t> d_offs, d_slot, d_slot2, d_claim, d_cslot, d_first, d_first_out, d_stream, d_aux;
  DevBuf<uint64_t> d_expires, d_out;
  DevBuf<uint8_t> d_flags, d_state;
  DevBuf<iv_val> d_val;
  DevBuf<uint64_t> d_ctr;  // three blocks of IV_CTR_WORDS: the call's first set, its second, a rebuild
  PinBuf<uint64_t> h_ctr;
  Event ev[8];
};
std::unique_ptr<InvScratch> g_inv;

void inv_release_shards() { g_inv.reset(); }

namespace {

using clk = std::chrono::steady_clock;
double ms_since(clk::time_point a) { return std::chrono::duration<double, std::milli>(clk::now() - a).count(); }

template <class B>
hipError_t hold(B& b, int dev, size_t n, unsigned flags = 0) {
  if (b && n <= b.cap()) return hipSuccess;
  return b.alloc(dev, std::max(n + n / 4, (size_t)4096), flags);
}

ivf::Table table_of(const bmpow_invset& s) { return ivf::Table{s.d_state.get(), s.d_keys.get(), s.d_vals.get(), s.seed, s.log2}; }

uint32_t log2_for(uint64_t entries) {  // the smallest table that keeps `entries` at or below half its slots
  uint32_t l = kMinLog2;
  while (l <= kMaxLog2 && (1ull << l) < 2 * entries) ++l;
  return l;
}

// Under g_mu, devices initialised: the set is of this shard set.
int check_set(const bmpow_invset* s) {
  if (!s) return set_err(BMPOW_E_ARG, "null inventory set");
  if (s->generation != g_generation || g_shards.empty() || s->dev != g_shards[0].dev)
    return set_err(BMPOW_E_STATE, "device set changed under a live inventory set");
  return 0;
}

int scratch(InvScratch** out) {
  Shard& sh = g_shards[0];
  if (!g_inv) g_inv.reset(new InvScratch());
  InvScratch& sc = *g_inv;
  if (!sc.d_ctr) HIPTRY(sc.d_ctr.alloc(sh.dev, 3 * IV_CTR_WORDS));
  if (!sc.h_ctr) HIPTRY(sc.h_ctr.alloc(sh.dev, 3 * IV_CTR_WORDS, hipHostMallocDefault));
  for (Event& e : sc.ev)
    if (!e) HIPTRY(e.alloc(sh.dev));
  *out = &sc;
  return 0;
}

// The counters of block b after the stream drained, into the set's.
int take_counters(bmpow_invset& s, const InvScratch& sc, int b) {
  const uint64_t* c = sc.h_ctr.get() + b * IV_CTR_WORDS;
  s.st.probes += c[IV_CTR_PROBES];
  s.st.longest_probe = std::max(s.st.longest_probe, c[IV_CTR_LONGEST]);
  if (c[IV_CTR_BAD]) return set_err(BMPOW_E_STATE, "an inventory set's probe ran over every slot");
  return 0;
}

int alloc_table(int dev, uint32_t log2, DevBuf<uint64_t>& st, DevBuf<uint64_t>& keys, DevBuf<iv_val>& vals, hipStream_t stream) {
  const size_t slots = (size_t)1 << log2;
  HIPTRY(st.alloc(dev, slots));
  HIPTRY(keys.alloc(dev, 4 * slots));
  HIPTRY(vals.alloc(dev, slots));
  HIPTRY(hipMemsetAsync(st.get(), 0, slots * sizeof(uint64_t), stream));
  return 0;
}

// Every full entry with expires >= min_expires into a fresh table of 2^log2 slots; the old one is released.
int rebuild(bmpow_invset& s, uint32_t log2, uint64_t min_expires) {
  if (log2 > kMaxLog2) return set_err(BMPOW_E_ARG, "an inventory set above 2^30 slots");
  Shard& sh = g_shards[0];
  InvScratch* sc = nullptr;
  if (const int rc = scratch(&sc); rc < 0) return rc;
  HIPTRY(hipSetDevice(sh.dev));
  DevBuf<uint64_t> st, keys;
  DevBuf<iv_val> vals;
  if (const int rc = alloc_table(sh.dev, log2, st, keys, vals, sh.stream); rc < 0) return rc;
  uint64_t* ctr = sc->d_ctr.get() + 2 * IV_CTR_WORDS;
  HIPTRY(hipMemsetAsync(ctr, 0, IV_CTR_WORDS * sizeof(uint64_t), sh.stream));
  const ivf::Table to{st.get(), keys.get(), vals.get(), s.seed, log2};
  HIPTRY(hipEventRecord(sc->ev[6].get(), sh.stream));
  HIPTRY(iv_launch_rebuild(sh.stream, table_of(s), to, min_expires, ctr));
  HIPTRY(hipEventRecord(sc->ev[7].get(), sh.stream));
  HIPTRY(hipMemcpyAsync(sc->h_ctr.get() + 2 * IV_CTR_WORDS, ctr, IV_CTR_WORDS * sizeof(uint64_t), hipMemcpyDeviceToHost, sh.stream));
  HIPTRY(hipStreamSynchronize(sh.stream));
  if (const int rc = elapsed(s.st.rebuild_ms, sc->ev[6], sc->ev[7]); rc < 0) return rc;
  s.st.launches++, s.st.rebuilds++;
  if (const int rc = take_counters(s, *sc, 2); rc < 0) return rc;
  s.live = sc->h_ctr[2 * IV_CTR_WORDS + IV_CTR_KEPT];
  s.tombs = 0;
  s.log2 = log2;
  s.d_state = std::move(st), s.d_keys = std::move(keys), s.d_vals = std::move(vals);
  return 0;
}

// live + tombstones + incoming at or below half the slots, by a rebuild first where needed
int ensure_room(bmpow_invset& s, uint64_t incoming) {
  if (2 * (s.live + s.tombs + incoming) <= (1ull << s.log2)) return 0;
  return rebuild(s, std::max(s.log2, log2_for(s.live + incoming)), 0);
}

// n x 32 contiguous key bytes up as the call's rows
int upload_keys(InvScratch& sc, const uint8_t* keys, size_t n, ivf::Rows* rows) {
  Shard& sh = g_shards[0];
  HIPTRY(hold(sc.d_in, sh.dev, 4 * n));
  HIPTRY(hipMemcpyAsync(sc.d_in.get(), keys, 32 * n, hipMemcpyHostToDevice, sh.stream));
  *rows = ivf::Rows{sc.d_in.get(), 32ull * n, nullptr, (uint32_t)n};
  return 0;
}

int zero_counters(InvScratch& sc) {
  return hipMemsetAsync(sc.d_ctr.get(), 0, 2 * IV_CTR_WORDS * sizeof(uint64_t), g_shards[0].stream) == hipSuccess
             ? 0
             : set_err(BMPOW_E_HIP, "hipMemsetAsync of the inventory counters");
}

int fetch_counters(InvScratch& sc) {
  HIPTRY(hipMemcpyAsync(sc.h_ctr.get(), sc.d_ctr.get(), 2 * IV_CTR_WORDS * sizeof(uint64_t), hipMemcpyDeviceToHost,
                        g_shards[0].stream));
  return 0;
}

// claim + finalize of rows into s (ev[e0 .. e0 + 2] around them); the answers stay in d_state / d_first_out
int insert_rows(bmpow_invset& s, InvScratch& sc, const ivf::Rows& rows, const uint8_t* d_flags, const uint32_t* d_skip,
                const uint64_t* d_expires, uint64_t expires_all, const uint32_t* d_stream, const uint32_t* d_aux, int block,
                int e0) {
  Shard& sh = g_shards[0];
  const size_t n = rows.n;
  HIPTRY(hold(sc.d_claim, sh.dev, n));
  HIPTRY(hold(sc.d_cslot, sh.dev, n));
  HIPTRY(hold(sc.d_first, sh.dev, n));
  HIPTRY(hold(sc.d_first_out, sh.dev, n));
  HIPTRY(hold(sc.d_state, sh.dev, n));
  uint64_t* ctr = sc.d_ctr.get() + block * IV_CTR_WORDS;
  HIPTRY(hipMemsetAsync(sc.d_first.get(), 0xff, n * sizeof(uint32_t), sh.stream));
  HIPTRY(hipEventRecord(sc.ev[e0].get(), sh.stream));
  HIPTRY(iv_launch_claim(sh.stream, table_of(s), rows, d_flags, d_skip, sc.d_first.get(), sc.d_claim.get(), sc.d_cslot.get(), ctr));
  HIPTRY(hipEventRecord(sc.ev[e0 + 1].get(), sh.stream));
  HIPTRY(iv_launch_finalize(sh.stream, table_of(s), rows, sc.d_first.get(), sc.d_claim.get(), sc.d_cslot.get(), d_expires,
                            expires_all, d_stream, d_aux, sc.d_state.get(), sc.d_first_out.get(), ctr));
  HIPTRY(hipEventRecord(sc.ev[e0 + 2].get(), sh.stream));
  s.st.launches += 2;
  return 0;
}

struct Call {  // what every device call starts with, under g_mu
  InvScratch* sc = nullptr;
  clk::time_point t0;
};
int begin(Call& c, bmpow_invset* a, bmpow_invset* b) {
  int rc = init_locked();
  if (rc < 0) return rc;
  if ((rc = check_set(a)) < 0) return rc;
  if (b && (rc = check_set(b)) < 0) return rc;
  if (g_abort.load()) return set_err(BMPOW_E_ABORTED, "aborted");
  HIPTRY(hipSetDevice(g_shards[0].dev));
  c.t0 = clk::now();
  return scratch(&c.sc);
}

}  // namespace

}  // namespace bmhost

using namespace bmhost;

extern "C" {

bmpow_invset* bmpow_invset_create(uint64_t slots_hint, uint64_t seed) {
  std::lock_guard<FairMutex> lk(g_mu);
  if (init_locked() < 0) return nullptr;
  if (slots_hint > (1ull << kMaxLog2)) {
    set_err(BMPOW_E_ARG, "an inventory set above 2^30 slots");
    return nullptr;
  }
  std::unique_ptr<bmpow_invset> s(new bmpow_invset());
  while (seed == 0) {
    std::random_device rd;
    seed = ((uint64_t)rd() << 32) | rd();
  }
  Shard& sh = g_shards[0];
  s->generation = g_generation;
  s->dev = sh.dev;
  s->seed = seed;
  s->log2 = log2_for((slots_hint + 1) / 2);
  if (alloc_table(sh.dev, s->log2, s->d_state, s->d_keys, s->d_vals, sh.stream) < 0) return nullptr;
  if (hipStreamSynchronize(sh.stream) != hipSuccess) {
    set_err(BMPOW_E_HIP, "hipStreamSynchronize");
    return nullptr;
  }
  return s.release();
}

void bmpow_invset_destroy(bmpow_invset* set) {
  if (!set) return;
  std::lock_guard<FairMutex> lk(g_mu);
  // of the live shard set: whatever the stream still runs on the table ends first
  if (set->generation == g_generation && !g_shards.empty() && hipSetDevice(g_shards[0].dev) == hipSuccess)
    (void)hipStreamSynchronize(g_shards[0].stream);
  delete set;
}

int bmpow_invset_clear(bmpow_invset* set) {
  std::lock_guard<FairMutex> lk(g_mu);
  Call c;
  if (const int rc = begin(c, set, nullptr); rc < 0) return rc;
  Shard& sh = g_shards[0];
  HIPTRY(hipMemsetAsync(set->d_state.get(), 0, sizeof(uint64_t) << set->log2, sh.stream));
  HIPTRY(hipStreamSynchronize(sh.stream));
  const uint64_t seed = set->seed;
  set->live = set->tombs = 0;
  set->st = bmpow_inv_stats{};
  set->st.seed = seed;
  return 0;
}

int64_t bmpow_invset_len(bmpow_invset* set) {
  std::lock_guard<FairMutex> lk(g_mu);
  int rc = init_locked();
  if (rc < 0 || (rc = check_set(set)) < 0) return rc;
  return (int64_t)set->live;
}

int bmpow_invset_stats(bmpow_invset* set, bmpow_inv_stats* out) {
  if (!out) return set_err(BMPOW_E_ARG, "null pointer");
  std::lock_guard<FairMutex> lk(g_mu);
  int rc = init_locked();
  if (rc < 0 || (rc = check_set(set)) < 0) return rc;
  *out = set->st;
  out->slots = 1ull << set->log2;
  out->seed = set->seed;
  out->live = set->live;
  out->tombstones = set->tombs;
  return 0;
}

int bmpow_invset_add(bmpow_invset* set, size_t n, const uint8_t* keys, const uint64_t* expires, const uint32_t* stream,
                     const uint32_t* aux, uint8_t* state_out, uint32_t* first_out) {
  std::lock_guard<FairMutex> lk(g_mu);
  Call c;
  int rc = begin(c, set, nullptr);
  if (rc < 0) return rc;
  if (n == 0) return 0;
  if (!keys || !state_out || !first_out) return set_err(BMPOW_E_ARG, "null pointer");
  if (n > kMaxRows) return set_err(BMPOW_E_ARG, "more than 2^30 rows");
  if ((rc = ensure_room(*set, n)) < 0) return rc;
  Shard& sh = g_shards[0];
  InvScratch& sc = *c.sc;
  ivf::Rows rows;
  if ((rc = upload_keys(sc, keys, n, &rows)) < 0) return rc;
  if (expires) {
    HIPTRY(hold(sc.d_expires, sh.dev, n));
    HIPTRY(hipMemcpyAsync(sc.d_expires.get(), expires, n * sizeof(uint64_t), hipMemcpyHostToDevice, sh.stream));
  }
  if (stream) {
    HIPTRY(hold(sc.d_stream, sh.dev, n));
    HIPTRY(hipMemcpyAsync(sc.d_stream.get(), stream, n * sizeof(uint32_t), hipMemcpyHostToDevice, sh.stream));
  }
  if (aux) {
    HIPTRY(hold(sc.d_aux, sh.dev, n));
    HIPTRY(hipMemcpyAsync(sc.d_aux.get(), aux, n * sizeof(uint32_t), hipMemcpyHostToDevice, sh.stream));
  }
  if ((rc = zero_counters(sc)) < 0) return rc;
  if ((rc = insert_rows(*set, sc, rows, nullptr, nullptr, expires ? sc.d_expires.get() : nullptr, 0,
                        stream ? sc.d_stream.get() : nullptr, aux ? sc.d_aux.get() : nullptr, 0, 0)) < 0)
    return rc;
  HIPTRY(hipMemcpyAsync(state_out, sc.d_state.get(), n, hipMemcpyDeviceToHost, sh.stream));
  HIPTRY(hipMemcpyAsync(first_out, sc.d_first_out.get(), n * sizeof(uint32_t), hipMemcpyDeviceToHost, sh.stream));
  if ((rc = fetch_counters(sc)) < 0) return rc;
  HIPTRY(hipStreamSynchronize(sh.stream));
  double* const acc[2] = {&set->st.claim_ms, &set->st.finalize_ms};
  if ((rc = elapsed_phases(acc, sc.ev, 2)) < 0) return rc;
  set->live += sc.h_ctr[IV_CTR_ADDED];
  set->st.calls++, set->st.rows += n;
  set->st.host_ms += ms_since(c.t0);
  return take_counters(*set, sc, 0);
}

int bmpow_invset_contains(bmpow_invset* set, size_t n, const uint8_t* keys, uint8_t* present_out, bmpow_inv_value* value_out) {
  static_assert(sizeof(bmpow_inv_value) == sizeof(iv_val), "the value's layout");
  std::lock_guard<FairMutex> lk(g_mu);
  Call c;
  int rc = begin(c, set, nullptr);
  if (rc < 0) return rc;
  if (n == 0) return 0;
  if (!keys || !present_out) return set_err(BMPOW_E_ARG, "null pointer");
  if (n > kMaxRows) return set_err(BMPOW_E_ARG, "more than 2^30 rows");
  Shard& sh = g_shards[0];
  InvScratch& sc = *c.sc;
  ivf::Rows rows;
  if ((rc = upload_keys(sc, keys, n, &rows)) < 0) return rc;
  HIPTRY(hold(sc.d_slot, sh.dev, n));
  if (value_out) HIPTRY(hold(sc.d_val, sh.dev, n));
  if ((rc = zero_counters(sc)) < 0) return rc;
  HIPTRY(hipEventRecord(sc.ev[0].get(), sh.stream));
  HIPTRY(iv_launch_lookup(sh.stream, table_of(*set), rows, nullptr, 0, sc.d_slot.get(), value_out ? sc.d_val.get() : nullptr,
                          sc.d_ctr.get()));
  HIPTRY(hipEventRecord(sc.ev[1].get(), sh.stream));
  static std::vector<uint32_t> slot;  // scratch kept across calls under g_mu
  slot.resize(n);
  HIPTRY(hipMemcpyAsync(slot.data(), sc.d_slot.get(), n * sizeof(uint32_t), hipMemcpyDeviceToHost, sh.stream));
  if (value_out) HIPTRY(hipMemcpyAsync(value_out, sc.d_val.get(), n * sizeof(iv_val), hipMemcpyDeviceToHost, sh.stream));
  if ((rc = fetch_counters(sc)) < 0) return rc;
  HIPTRY(hipStreamSynchronize(sh.stream));
  if ((rc = elapsed(set->st.lookup_ms, sc.ev[0], sc.ev[1])) < 0) return rc;
  for (size_t i = 0; i < n; ++i) present_out[i] = slot[i] != IV_NONE;
  set->st.calls++, set->st.rows += n, set->st.launches++;
  set->st.host_ms += ms_since(c.t0);
  return take_counters(*set, sc, 0);
}

int bmpow_invset_remove(bmpow_invset* set, size_t n, const uint8_t* keys, uint8_t* present_out) {
  std::lock_guard<FairMutex> lk(g_mu);
  Call c;
  int rc = begin(c, set, nullptr);
  if (rc < 0) return rc;
  if (n == 0) return 0;
  if (!keys) return set_err(BMPOW_E_ARG, "null pointer");
  if (n > kMaxRows) return set_err(BMPOW_E_ARG, "more than 2^30 rows");
  Shard& sh = g_shards[0];
  InvScratch& sc = *c.sc;
  ivf::Rows rows;
  if ((rc = upload_keys(sc, keys, n, &rows)) < 0) return rc;
  HIPTRY(hold(sc.d_slot, sh.dev, n));
  if ((rc = zero_counters(sc)) < 0) return rc;
  HIPTRY(hipEventRecord(sc.ev[0].get(), sh.stream));
  HIPTRY(iv_launch_lookup(sh.stream, table_of(*set), rows, nullptr, 0, sc.d_slot.get(), nullptr, sc.d_ctr.get()));
  HIPTRY(hipEventRecord(sc.ev[1].get(), sh.stream));
  HIPTRY(iv_launch_bury(sh.stream, table_of(*set), sc.d_slot.get(), (uint32_t)n, sc.d_ctr.get()));
  HIPTRY(hipEventRecord(sc.ev[2].get(), sh.stream));
  static std::vector<uint32_t> slot;  // scratch kept across calls under g_mu
  slot.resize(n);
  HIPTRY(hipMemcpyAsync(slot.data(), sc.d_slot.get(), n * sizeof(uint32_t), hipMemcpyDeviceToHost, sh.stream));
  if ((rc = fetch_counters(sc)) < 0) return rc;
  HIPTRY(hipStreamSynchronize(sh.stream));
  double* const acc[2] = {&set->st.lookup_ms, &set->st.bury_ms};
  if ((rc = elapsed_phases(acc, sc.ev, 2)) < 0) return rc;
  if (present_out)
    for (size_t i = 0; i < n; ++i) present_out[i] = slot[i] != IV_NONE;
  const uint64_t removed = std::min(sc.h_ctr[IV_CTR_REMOVED], set->live);
  set->live -= removed, set->tombs += removed;
  set->st.calls++, set->st.rows += n, set->st.launches += 2;
  set->st.host_ms += ms_since(c.t0);
  return take_counters(*set, sc, 0);
}

int64_t bmpow_invset_sweep(bmpow_invset* set, uint64_t min_expires) {
  std::lock_guard<FairMutex> lk(g_mu);
  Call c;
  int rc = begin(c, set, nullptr);
  if (rc < 0) return rc;
  if ((rc = rebuild(*set, set->log2, min_expires)) < 0) return rc;
  set->st.calls++;
  set->st.host_ms += ms_since(c.t0);
  return (int64_t)set->live;
}

int64_t bmpow_invset_list(bmpow_invset* set, uint32_t stream, uint64_t now, uint8_t* out, size_t cap) {
  std::lock_guard<FairMutex> lk(g_mu);
  Call c;
  int rc = begin(c, set, nullptr);
  if (rc < 0) return rc;
  if (cap && !out) return set_err(BMPOW_E_ARG, "null pointer");
  if (cap > kMaxRows) return set_err(BMPOW_E_ARG, "more than 2^30 rows");
  Shard& sh = g_shards[0];
  InvScratch& sc = *c.sc;
  HIPTRY(hold(sc.d_out, sh.dev, 4 * std::max(cap, (size_t)1)));
  if ((rc = zero_counters(sc)) < 0) return rc;
  HIPTRY(hipEventRecord(sc.ev[0].get(), sh.stream));
  HIPTRY(iv_launch_list(sh.stream, table_of(*set), stream, now, reinterpret_cast<uint8_t*>(sc.d_out.get()), cap, sc.d_ctr.get()));
  HIPTRY(hipEventRecord(sc.ev[1].get(), sh.stream));
  if ((rc = fetch_counters(sc)) < 0) return rc;
  HIPTRY(hipStreamSynchronize(sh.stream));
  if ((rc = elapsed(set->st.list_ms, sc.ev[0], sc.ev[1])) < 0) return rc;
  const uint64_t found = sc.h_ctr[IV_CTR_LISTED], got = std::min<uint64_t>(found, cap);
  if (got) HIPTRY(hipMemcpy(out, sc.d_out.get(), 32 * got, hipMemcpyDeviceToHost));
  set->st.calls++, set->st.launches++;
  set->st.host_ms += ms_since(c.t0);
  return (int64_t)found;
}

uint64_t bmpow_invset_slot(uint64_t seed, uint32_t log2_slots, const uint8_t key[32]) {
  if (!key || log2_slots < 1 || log2_slots > kMaxLog2) return 0;
  uint64_t k[4];
  std::memcpy(k, key, 32);
  return ivf::start_slot(seed, log2_slots, k);
}

static void walk_into(const uint8_t* payload, uint64_t len, int kind, int dandelion_on, bmpow_inv_pkt* out) {
  const ivf::Walk w = ivf::walk(payload, len);
  *out = bmpow_inv_pkt{w.count, 0, 0, (uint32_t)w.at, BMPOW_INV_OK};
  if (w.status != IV_WALK_OK) {
    *out = bmpow_inv_pkt{0, 0, 0, 0, BMPOW_INV_MALFORMED};
    return;
  }
  if (kind != BMPOW_INV_KIND_GETDATA) {
    if (w.count > BMPOW_INV_MAX_OBJECT_COUNT) {  // bmproto.py:351-354, before the dandelion switch
      out->status = BMPOW_INV_TOO_MANY;
      return;
    }
    if (kind == BMPOW_INV_KIND_DINV && !dandelion_on) {  // :356-358
      out->status = BMPOW_INV_IGNORED;
      return;
    }
  }
  // the full items, the short one, and the first of the empty ones behind the payload's end
  const uint64_t shown = w.full + (w.tail ? 1 : 0);
  out->n_items = (uint32_t)std::min<uint64_t>(w.count, shown + 1);
}

int bmpow_inv_walk(const uint8_t* payload, uint64_t len, int kind, int dandelion_on, bmpow_inv_pkt* out) {
  if (!out || (len && !payload)) return set_err(BMPOW_E_ARG, "null pointer");
  if (kind < BMPOW_INV_KIND_INV || kind > BMPOW_INV_KIND_GETDATA) return set_err(BMPOW_E_ARG, "unknown packet kind");
  if (len >= (1ULL << 32)) return set_err(BMPOW_E_ARG, "a payload of 4 GiB or more");
  walk_into(payload, len, kind, dandelion_on, out);
  return 0;
}

int64_t bmpow_inv_batch(bmpow_invset* have, bmpow_invset* missing, size_t n_pkt, const uint8_t* const* payloads,
                        const uint64_t* lens, const uint8_t* kinds, uint64_t now, int dandelion_on, bmpow_inv_pkt* pkt_recs,
                        uint8_t* item_state, uint32_t* item_first, size_t cap) {
  std::lock_guard<FairMutex> lk(g_mu);
  Call c;
  int rc = begin(c, have, missing);
  if (rc < 0) return rc;
  if (n_pkt == 0) return 0;
  if (!payloads || !lens || !kinds || !pkt_recs || (cap && (!item_state || !item_first))) return set_err(BMPOW_E_ARG, "null pointer");
  if (have == missing) return set_err(BMPOW_E_ARG, "one set given as both have and missing");
  // the walk: items, and the rows (the items of 32 bytes) with where their bytes will lie in the upload
  static std::vector<uint64_t> base;  // scratch kept across calls under g_mu
  static std::vector<uint32_t> offs, row_item, h_slot, h_first;
  static std::vector<uint8_t> flags, h_state;
  base.assign(n_pkt, 0), offs.clear(), row_item.clear(), flags.clear();
  uint64_t items = 0, total = 0, n_add = 0;
  for (size_t p = 0; p < n_pkt; ++p) {
    if (kinds[p] > BMPOW_INV_KIND_GETDATA) return set_err(BMPOW_E_ARG, "unknown packet kind");
    if ((lens[p] && !payloads[p]) || lens[p] >= (1ULL << 32)) return set_err(BMPOW_E_ARG, "a null payload or one of 4 GiB or more");
    walk_into(payloads[p], lens[p], kinds[p], dandelion_on, &pkt_recs[p]);
    pkt_recs[p].first_item = (uint32_t)items;
    items += pkt_recs[p].n_items;
    if (items > cap) return set_err(BMPOW_E_ARG, "the item arrays hold fewer items than the packets carry");
    if (pkt_recs[p].n_items == 0) continue;
    const uint64_t full = std::min<uint64_t>((lens[p] - pkt_recs[p].item_offset) / 32, pkt_recs[p].n_items);
    const bool adds = kinds[p] != BMPOW_INV_KIND_GETDATA;
    for (uint32_t k = 0; k < pkt_recs[p].n_items; ++k) {
      const uint32_t j = pkt_recs[p].first_item + k;
      item_state[j] = BMPOW_INV_ITEM_SHORT;
      item_first[j] = j;
      if (k >= full) continue;
      offs.push_back((uint32_t)(total + pkt_recs[p].item_offset + 32ull * k));
      row_item.push_back(j);
      flags.push_back((uint8_t)(IV_ROW_LOOKUP | (adds ? IV_ROW_ADD : 0u)));
      n_add += adds;
    }
    if (full == 0) continue;  // nothing of this payload is read on the device
    base[p] = total;
    if ((total += lens[p]) >= (1ULL << 32)) return set_err(BMPOW_E_ARG, "the payloads hold 4 GiB or more in all");
    base[p] |= 1ull << 63;  // uploaded
  }
  const size_t n = offs.size();
  if (n == 0) return (int64_t)items;
  if (n > kMaxRows) return set_err(BMPOW_E_ARG, "more than 2^30 rows");
  if (n_add && !missing) return set_err(BMPOW_E_ARG, "inv items and no missing set");
  if (n_add && (rc = ensure_room(*missing, n_add)) < 0) return rc;
  Shard& sh = g_shards[0];
  InvScratch& sc = *c.sc;
  HIPTRY(hold(sc.d_in, sh.dev, (size_t)((total + 7) / 8)));
  HIPTRY(hold(sc.d_offs, sh.dev, n));
  HIPTRY(hold(sc.d_flags, sh.dev, n));
  HIPTRY(hold(sc.d_slot, sh.dev, n));
  for (size_t p = 0; p < n_pkt; ++p)
    if (base[p] >> 63)
      HIPTRY(hipMemcpyAsync(reinterpret_cast<uint8_t*>(sc.d_in.get()) + (base[p] & ~(1ull << 63)), payloads[p], lens[p],
                            hipMemcpyHostToDevice, sh.stream));
  HIPTRY(hipMemcpyAsync(sc.d_offs.get(), offs.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, sh.stream));
  HIPTRY(hipMemcpyAsync(sc.d_flags.get(), flags.data(), n, hipMemcpyHostToDevice, sh.stream));
  const ivf::Rows rows{sc.d_in.get(), total, sc.d_offs.get(), (uint32_t)n};
  if ((rc = zero_counters(sc)) < 0) return rc;
  HIPTRY(hipEventRecord(sc.ev[0].get(), sh.stream));
  HIPTRY(iv_launch_lookup(sh.stream, table_of(*have), rows, sc.d_flags.get(), IV_ROW_LOOKUP, sc.d_slot.get(), nullptr, sc.d_ctr.get()));
  HIPTRY(hipEventRecord(sc.ev[1].get(), sh.stream));
  have->st.launches++;
  h_slot.resize(n), h_state.assign(n, BMPOW_INV_ABSENT), h_first.resize(n);
  if (n_add) {
    if ((rc = insert_rows(*missing, sc, rows, sc.d_flags.get(), sc.d_slot.get(), nullptr, now, nullptr, nullptr, 1, 2)) < 0) return rc;
    HIPTRY(hipMemcpyAsync(h_state.data(), sc.d_state.get(), n, hipMemcpyDeviceToHost, sh.stream));
    HIPTRY(hipMemcpyAsync(h_first.data(), sc.d_first_out.get(), n * sizeof(uint32_t), hipMemcpyDeviceToHost, sh.stream));
  }
  HIPTRY(hipMemcpyAsync(h_slot.data(), sc.d_slot.get(), n * sizeof(uint32_t), hipMemcpyDeviceToHost, sh.stream));
  if ((rc = fetch_counters(sc)) < 0) return rc;
  HIPTRY(hipStreamSynchronize(sh.stream));
  if ((rc = elapsed(have->st.lookup_ms, sc.ev[0], sc.ev[1])) < 0) return rc;
  have->st.calls++, have->st.rows += n;
  if ((rc = take_counters(*have, sc, 0)) < 0) return rc;
  if (n_add) {
    double* const acc[2] = {&missing->st.claim_ms, &missing->st.finalize_ms};
    if ((rc = elapsed_phases(acc, sc.ev + 2, 2)) < 0) return rc;
    missing->live += sc.h_ctr[IV_CTR_WORDS + IV_CTR_ADDED];
    missing->st.calls++, missing->st.rows += n_add;
    if ((rc = take_counters(*missing, sc, 1)) < 0) return rc;
  }
  for (size_t r = 0; r < n; ++r) {
    const uint32_t j = row_item[r];
    if (h_slot[r] != IV_NONE) {
      item_state[j] = BMPOW_INV_ITEM_HAVE;
    } else if (!(flags[r] & IV_ROW_ADD)) {
      item_state[j] = BMPOW_INV_ITEM_NOT_HAVE;
    } else if (h_state[r] == BMPOW_INV_PRESENT) {
      item_state[j] = BMPOW_INV_ITEM_KNOWN;
    } else if (h_state[r] == BMPOW_INV_ADDED || h_first[r] >= n) {
      item_state[j] = BMPOW_INV_ITEM_NEW;
    } else {
      item_state[j] = BMPOW_INV_ITEM_NEW_AGAIN;
      item_first[j] = row_item[h_first[r]];
    }
  }
  have->st.host_ms += ms_since(c.t0);
  return (int64_t)items;
}

int bmpow_inv_admit(bmpow_invset* have, bmpow_invset* missing, size_t n, const void* intake_recs, size_t stride,
                    const uint8_t* store_mask, uint8_t* already_out, uint8_t* state_out) {
  std::lock_guard<FairMutex> lk(g_mu);
  Call c;
  int rc = begin(c, have, missing);
  if (rc < 0) return rc;
  if (n == 0) return 0;
  if (!intake_recs || !store_mask || !already_out || !state_out) return set_err(BMPOW_E_ARG, "null pointer");
  if (have == missing) return set_err(BMPOW_E_ARG, "one set given as both have and missing");
  if (n > kMaxRows) return set_err(BMPOW_E_ARG, "more than 2^30 rows");
  if (stride == 0) stride = sizeof(bmpow_intake_rec);
  if (stride < sizeof(bmpow_intake_rec)) return set_err(BMPOW_E_ARG, "a stride below the record's size");
  static std::vector<uint8_t> keys, flags;  // scratch kept across calls under g_mu
  static std::vector<uint64_t> expires;
  static std::vector<uint32_t> stream, aux, h_slot;
  keys.resize(32 * n), flags.resize(n), expires.resize(n), stream.resize(n), aux.resize(n), h_slot.resize(n);
  uint64_t n_add = 0;
  for (size_t i = 0; i < n; ++i) {
    bmpow_intake_rec r;
    std::memcpy(&r, static_cast<const uint8_t*>(intake_recs) + i * stride, sizeof(r));
    // the statuses behind checkAlreadyHave in bm_command_object's order (bmproto.py:393-419)
    const bool reach = store_mask[i] != BMPOW_INV_ADMIT_SKIP &&
                       (r.status == BMPOW_INTAKE_OK || r.status == BMPOW_INTAKE_INVALID_STREAM ||
                        r.status == BMPOW_INTAKE_UNWANTED_STREAM || r.status == BMPOW_INTAKE_INVALID_FOR_TYPE);
    const bool store = reach && store_mask[i] == BMPOW_INV_ADMIT_STORE;
    flags[i] = reach ? (uint8_t)(IV_ROW_LOOKUP | (store ? IV_ROW_ADD : 0u)) : 0;
    n_add += store;
    std::memcpy(keys.data() + 32 * i, r.inv, 32);
    expires[i] = r.expires;
    stream[i] = r.stream > 0xffffffffULL ? 0xffffffffu : (uint32_t)r.stream;
    aux[i] = (uint32_t)i;
  }
  if (n_add && (rc = ensure_room(*have, n_add)) < 0) return rc;
  Shard& sh = g_shards[0];
  InvScratch& sc = *c.sc;
  ivf::Rows rows;
  if ((rc = upload_keys(sc, keys.data(), n, &rows)) < 0) return rc;
  HIPTRY(hold(sc.d_flags, sh.dev, n));
  HIPTRY(hold(sc.d_slot, sh.dev, n));
  HIPTRY(hold(sc.d_slot2, sh.dev, n));
  HIPTRY(hold(sc.d_expires, sh.dev, n));
  HIPTRY(hold(sc.d_stream, sh.dev, n));
  HIPTRY(hold(sc.d_aux, sh.dev, n));
  HIPTRY(hipMemcpyAsync(sc.d_flags.get(), flags.data(), n, hipMemcpyHostToDevice, sh.stream));
  HIPTRY(hipMemcpyAsync(sc.d_expires.get(), expires.data(), n * sizeof(uint64_t), hipMemcpyHostToDevice, sh.stream));
  HIPTRY(hipMemcpyAsync(sc.d_stream.get(), stream.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, sh.stream));
  HIPTRY(hipMemcpyAsync(sc.d_aux.get(), aux.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, sh.stream));
  if ((rc = zero_counters(sc)) < 0) return rc;
  HIPTRY(hipEventRecord(sc.ev[0].get(), sh.stream));
  HIPTRY(iv_launch_lookup(sh.stream, table_of(*have), rows, sc.d_flags.get(), IV_ROW_LOOKUP, sc.d_slot.get(), nullptr, sc.d_ctr.get()));
  if ((rc = insert_rows(*have, sc, rows, sc.d_flags.get(), nullptr, sc.d_expires.get(), 0, sc.d_stream.get(), sc.d_aux.get(), 0, 1)) < 0)
    return rc;
  if (missing) {
    uint64_t* ctr = sc.d_ctr.get() + IV_CTR_WORDS;
    HIPTRY(iv_launch_lookup(sh.stream, table_of(*missing), rows, sc.d_flags.get(), IV_ROW_LOOKUP, sc.d_slot2.get(), nullptr, ctr));
    HIPTRY(hipEventRecord(sc.ev[4].get(), sh.stream));
    HIPTRY(iv_launch_bury(sh.stream, table_of(*missing), sc.d_slot2.get(), (uint32_t)n, ctr));
    HIPTRY(hipEventRecord(sc.ev[5].get(), sh.stream));
  }
  HIPTRY(hipMemcpyAsync(h_slot.data(), sc.d_slot.get(), n * sizeof(uint32_t), hipMemcpyDeviceToHost, sh.stream));
  HIPTRY(hipMemcpyAsync(state_out, sc.d_state.get(), n, hipMemcpyDeviceToHost, sh.stream));
  if ((rc = fetch_counters(sc)) < 0) return rc;
  HIPTRY(hipStreamSynchronize(sh.stream));
  double* const acc[3] = {&have->st.lookup_ms, &have->st.claim_ms, &have->st.finalize_ms};
  if ((rc = elapsed_phases(acc, sc.ev, 3)) < 0) return rc;
  for (size_t i = 0; i < n; ++i) already_out[i] = h_slot[i] != IV_NONE;
  have->live += sc.h_ctr[IV_CTR_ADDED];
  have->st.calls++, have->st.rows += n, have->st.launches++;
  if ((rc = take_counters(*have, sc, 0)) < 0) return rc;
  if (missing) {
    double* const acc2[2] = {&missing->st.lookup_ms, &missing->st.bury_ms};
    if ((rc = elapsed_phases(acc2, sc.ev + 3, 2)) < 0) return rc;
    const uint64_t removed = std::min(sc.h_ctr[IV_CTR_WORDS + IV_CTR_REMOVED], missing->live);
    missing->live -= removed, missing->tombs += removed;
    missing->st.calls++, missing->st.rows += n, missing->st.launches += 2;
    if ((rc = take_counters(*missing, sc, 1)) < 0) return rc;
  }
  have->st.host_ms += ms_since(c.t0);
  return 0;
}

}  // extern "C"
