// bmpow_host_batch.hip -- the batch tables, the engine's device side (engine_launch / engine_wait), the
// min-trial probe, the scratch batch, the service, and their entry points (bmpow_trials*, bmpow_search*,
// bmpow_min_trial*, bmpow_batch_*, bmpow_service_*).  The scheduler itself is bmpow_sched.cpp.
#include "bmpow_host.h"

namespace bmhost {

// The buffers of one of a shard's two engine launch buffers (the running launch and the one staged behind it).
struct LaunchMem {
  PinBuf<bm_item> h_items;  // pinned: items, then 2 + n counters (zeroed on the host)
  DevBuf<bm_item> d_items;
  PinBuf<bm_result> h_res;  // pinned: results, then the trials counter
  DevBuf<bm_result> d_res;
  size_t cap = 0;
};
struct LaunchBuf {
  LaunchMem m;
  Event ev0, ev1, evd;  // search start / end, launch done
};

// Pinned staging of slot records for the slot-init kernel (an add while launches are in flight):
// reused once the kernel that read it has run.
struct UpBuf {
  PinBuf<uint8_t> h;  // mapped: h.dptr() is the device's address of it
  Event ev;
  bool pending = false;
};

// The engine's per-shard state (indexed like g_shards).
struct EngShard {
  // the engine's launches (searches)
  LaunchBuf lb[2];
  // launch buffers outgrown while the stepper held the engine's mutex: freed by the same stepper after
  // its next wait, without the mutex (hipFree / hipHostFree wait for the device)
  std::vector<LaunchMem> retired;
  std::vector<UpBuf> up;
  double t_prev_done = 0;  // steady-clock ms when the stepper last saw a launch complete
};
std::vector<EngShard> g_eng;

// The min-trial probe's per-shard state (indexed like g_shards).
struct ProbeShard {
  // per-step staging of the min-trial probe (capacity grows): its items, then its counters
  DevBuf<bm_item> d_items;
  DevBuf<bm_result> d_res;
  unsigned long long* d_trials = nullptr;
  unsigned long long* d_queue = nullptr;
  PinBuf<bm_item> h_items;      // pinned, the same layout
  PinBuf<bm_result> h_res;      // pinned
  size_t item_cap = 0;
  // step bookkeeping: items [0, nmain) / chunks [0, chmain) are 64-byte objects (bm_search_kernel),
  // the rest var-form objects (bm_search_var_kernel)
  uint32_t nitems = 0, nchunks = 0, nmain = 0, chmain = 0;
  // min-trial probe: one bm_minpart per workgroup of a launch (grow-only)
  DevBuf<bm_minpart> d_parts;
  PinBuf<bm_minpart> h_parts;  // pinned
};
std::vector<ProbeShard> g_probe;

// The per-device steppers over the shard set (created with it; bmsched::Engine).  Defined after the state
// its steppers use, so that it is destroyed (the steppers joined) before that state is.
std::unique_ptr<bmsched::Engine> g_engine;

void engine_release_shards() { g_eng.clear(); }
void probe_release_shards() { g_probe.clear(); }

// Bytes of a step's upload for n items: the items, then 2 + n counters.
size_t stage_bytes(size_t n) { return n * sizeof(bm_item) + (2 + n) * sizeof(unsigned long long); }

// The same in bm_item elements, rounded up (what the owners of a staging buffer are asked for).
size_t stage_elems(size_t n) { return (stage_bytes(n) + sizeof(bm_item) - 1) / sizeof(bm_item); }

// Grow the shard's item staging to hold n items.  Called while a step's item list is being
// filled, so the host items already written (s.nitems of them) move to the new buffer; the device
// copies and the results are (re)written after the fill.  A failed allocation leaves item_cap 0 and the
// owners it reached empty, so the next call starts over.
int ensure_items(ProbeShard& s, int dev, size_t n) {
  if (n <= s.item_cap) return 0;
  const size_t cap = std::max<size_t>(n, 2 * s.item_cap);
  PinBuf<bm_item> h_items;
  HIPTRY(h_items.alloc(dev, stage_elems(cap), hipHostMallocDefault));
  if (s.h_items) std::memcpy(h_items.get(), s.h_items.get(), std::min<size_t>(s.nitems, s.item_cap) * sizeof(bm_item));
  s.h_items = std::move(h_items);
  s.item_cap = 0;
  HIPTRY(s.d_items.grow(dev, stage_elems(cap)));
  HIPTRY(s.d_res.grow(dev, cap + 1));
  HIPTRY(s.h_res.grow(dev, cap + 1, hipHostMallocDefault));
  s.item_cap = cap;
  return 0;
}

// Grow an engine launch buffer to n items (only ever called for a buffer not in flight).  Called from
// engine_launch, under the engine's mutex: the old buffers are not freed here -- hipFree and hipHostFree
// wait for the whole device, every shard's launches in flight included -- but retired,
// and free_retired releases them from the stepper's wait, outside the mutex.  Retiring is a move of the
// owners into the shard's retired list: nothing is released, and never reset() in place here.
int ensure_launch_buf(EngShard& s, int dev, LaunchMem& m, size_t n) {
  if (n <= m.cap) return 0;
  const size_t cap = std::max<size_t>({n, 2 * m.cap, 1024});
  if (m.cap) s.retired.push_back(std::move(m));
  m.cap = 0;
  HIPTRY(m.h_items.alloc(dev, stage_elems(cap), hipHostMallocDefault));
  HIPTRY(m.d_items.alloc(dev, stage_elems(cap)));
  HIPTRY(m.h_res.alloc(dev, cap + 1, hipHostMallocDefault));
  HIPTRY(m.d_res.alloc(dev, cap + 1));
  m.cap = cap;
  return 0;
}

// Free the launch buffers the shard's stepper outgrew (ensure_launch_buf); none is in flight.
void free_retired(EngShard& s) { s.retired.clear(); }

// Per-shard state made with the shard set: the launch buffers' events, the probe's first staging.
int batch_init_shards() {
  g_eng.clear();
  g_eng.resize(g_shards.size());
  g_probe.clear();
  g_probe.resize(g_shards.size());
  for (size_t s = 0; s < g_shards.size(); ++s) {
    const int dev = g_shards[s].dev;
    for (LaunchBuf& lb : g_eng[s].lb) {
      HIPTRY(lb.ev0.alloc(dev));
      HIPTRY(lb.ev1.alloc(dev));
      HIPTRY(lb.evd.alloc(dev, hipEventDisableTiming | (g_wait == kWaitBlock ? hipEventBlockingSync : 0)));
    }
    if (const int rc = ensure_items(g_probe[s], dev, 1024); rc < 0) return rc;
  }
  return 0;
}

// ---- the engine's device side (bmsched::EngineOps) ----
int engine_launch(bmsched::Launch& L, std::string& err);
int engine_wait(bmsched::Launch& L, std::string& err);

void engine_xstore(uint32_t x, uint64_t v) {
  // every shard's row: the relays poll their own row (bm_relay); plain stores to coherent pinned memory
  for (size_t r = 0; r < g_shards.size(); ++r) __atomic_store_n(&g_xb[r * BM_XSLOTS + x], (unsigned long long)v, __ATOMIC_RELAXED);
  __atomic_thread_fence(__ATOMIC_SEQ_CST);
}

void make_engine() {
  bmsched::EngineOps ops;
  ops.launch = engine_launch;
  ops.wait = engine_wait;
  ops.xstore = engine_xstore;
  ops.aborted = [] { return g_abort.load() != 0; };
  ops.thread_init = [](size_t s) {
    (void)hipSetDevice(g_shards[s].dev);
    if (g_wait == kWaitBlock) (void)hipSetDeviceFlags(hipDeviceScheduleBlockingSync);
    bmsched::set_thread_background();
  };
  g_engine.reset(new bmsched::Engine(ops, g_shards.size(), g_resident, g_step_trials.load()));
  if (const char* e = std::getenv("BMPOW_THROTTLE")) {  // A/B knob "shard:ms" (the throttled-shard GPU test)
    const char* c = std::strchr(e, ':');
    if (c) g_engine->set_throttle((size_t)std::atoi(e), std::atof(c + 1));
  }
}

}  // namespace bmhost

// ---------------------------------------------------------------------------------------
// Batch state: the object table and per-object running minimum stay in HBM for the
// lifetime of the batch (one copy per shard).  best[]/found[] persist across launches: a launch
// queued behind another on the same stream stops at once above the hit the earlier one left there;
// a slot is reset on the device when it gets a new object (slot init, stream-ordered).
// ---------------------------------------------------------------------------------------
struct bmpow_batch : bmsched::BatchState {
  struct Dev {
    bmown::DevBuf<bm_obj> d_obj;
    bmown::DevBuf<unsigned long long> d_best;  // running minimum hit nonce (valid where d_found)
    bmown::DevBuf<uint32_t> d_found;           // 1 once the object has a hit on this shard
    bmown::DevBuf<uint64_t> d_vpool;           // copy of vpool (var-form objects' words), vcap words
  };
  std::vector<Dev> dev;  // one per shard (indexed like g_shards)
  uint64_t generation = ~0ULL;  // g_generation of the shard set dev[] was uploaded to (batch_upload)
  size_t vcap = 0;         // words allocated per shard for the var pool
  size_t vsynced = 0;      // vpool words already on the devices (of epoch vepoch)
  uint64_t vepoch = ~0ULL;
};

namespace bmhost {

// The batch's launches must be finished before its device buffers change: drains the engine when
// it is working on b.
void quiesce(std::unique_lock<std::mutex>& lk, bmpow_batch* b) {
  if (g_engine && g_engine->attached() == b) g_engine->drain(lk);
}

void batch_free_dev(bmpow_batch* b) {
  for (size_t s = 0; s < b->dev.size() && s < g_shards.size(); ++s) {
    (void)hipSetDevice(g_shards[s].dev);
    (void)hipStreamSynchronize(g_shards[s].stream);
  }
  b->dev.clear();
  b->vcap = 0;
  b->vsynced = 0;
  b->vepoch = ~0ULL;
}

// Bring the devices' copy of the var pool up to date: the words appended since the last sync (one
// copy per shard, into words no launch reads yet), or all of them after a reallocation or a new
// epoch (bmsched::add emptied it), which first drains the batch's launches.
int sync_vpool(std::unique_lock<std::mutex>& lk, bmpow_batch* b) {
  const size_t n = b->vpool.size();
  if (b->vepoch != b->vpool_epoch) {
    b->vsynced = 0;
    b->vepoch = b->vpool_epoch;
  }
  if (n == b->vsynced) return 0;
  const bool grow = n > b->vcap;
  const size_t cap = grow ? std::max<size_t>(n, 2 * b->vcap) : b->vcap;
  const size_t from = grow ? 0 : b->vsynced;
  if (grow || from == 0) quiesce(lk, b);
  for (size_t s = 0; s < g_shards.size(); ++s) {
    Shard& sh = g_shards[s];
    HIPTRY(hipSetDevice(sh.dev));
    if (grow) {
      if (b->dev[s].d_vpool) HIPTRY(hipStreamSynchronize(sh.stream));  // no launch may still read the old copy
      HIPTRY(b->dev[s].d_vpool.alloc(sh.dev, cap));
    }
    // the host vector may be appended to before an async copy ran: a synchronous copy
    HIPTRY(hipMemcpy(b->dev[s].d_vpool.get() + from, b->vpool.data() + from, (n - from) * sizeof(uint64_t),
                     hipMemcpyHostToDevice));
  }
  b->vcap = cap;
  b->vsynced = n;
  return 0;
}

int batch_upload(std::unique_lock<std::mutex>& lk, bmpow_batch* b) {
  b->dev.clear();
  b->dev.resize(g_shards.size());
  b->generation = g_generation;
  const size_t n = std::max<size_t>(b->cap, std::max<size_t>(b->n, 1));
  b->cap = n;
  for (size_t s = 0; s < g_shards.size(); ++s) {
    Shard& sh = g_shards[s];
    bmpow_batch::Dev& d = b->dev[s];
    HIPTRY(d.d_obj.alloc(sh.dev, n));
    HIPTRY(d.d_best.alloc(sh.dev, n));
    HIPTRY(d.d_found.alloc(sh.dev, n));
    if (b->n) {
      HIPTRY(hipMemcpyAsync(d.d_obj.get(), b->objs.data(), b->n * sizeof(bm_obj), hipMemcpyHostToDevice, sh.stream));
      HIPTRY(hipMemsetAsync(d.d_best.get(), 0xFF, b->n * sizeof(unsigned long long), sh.stream));
      HIPTRY(hipMemsetAsync(d.d_found.get(), 0, b->n * sizeof(uint32_t), sh.stream));
    }
  }
  if (const int rc = sync_shards(); rc < 0) return rc;
  return sync_vpool(lk, b);
}

int batch_init(std::unique_lock<std::mutex>& lk, bmpow_batch* b, size_t n, const uint8_t* ihs,
               const uint64_t* targets, const uint64_t* start, const uint64_t* ih_off = nullptr) {
  bmsched::init(*b, n, ihs, targets, start, ih_off);
  return batch_upload(lk, b);
}

// Write objects into slots of the devices' tables -- the record, best = UINT64_MAX, found = 0 --
// on each shard's stream, behind whatever is in flight there (bm_slots_init_kernel reading the
// records from pinned staging).  Called under the engine's mutex, under which the steppers also plan
// AND enqueue their launches, so every launch planned for the slot's previous occupant is queued
// before this init: it hashes the old record, its results are stale by the slot's generation, and the
// init resets best[] / found[] behind it (bmsched::Engine::stepper).
int init_slots(bmpow_batch* b, const uint32_t* slots, size_t m) {
  if (m == 0) return 0;
  const size_t rec = m * sizeof(bm_obj), bytes = rec + m * sizeof(uint32_t);
  for (size_t s = 0; s < g_shards.size(); ++s) {
    Shard& sh = g_shards[s];
    HIPTRY(hipSetDevice(sh.dev));
    std::vector<UpBuf>& up = g_eng[s].up;
    UpBuf* u = nullptr;
    for (UpBuf& x : up) {
      if (x.pending && hipEventQuery(x.ev.get()) == hipSuccess) x.pending = false;
      if (!x.pending && (!u || (x.h.cap() >= bytes && u->h.cap() < bytes))) u = &x;
    }
    if (!u) {
      up.emplace_back();
      u = &up.back();
      HIPTRY(u->ev.alloc(sh.dev, hipEventDisableTiming));
    }
    // (an idle staging buffer, pinned host memory no kernel reads any more: grown in place, as before)
    if (u->h.cap() < bytes) HIPTRY(u->h.grow(sh.dev, std::max<size_t>(bytes, 64 << 10), hipHostMallocMapped));
    uint8_t *h = u->h.get(), *d = u->h.dptr();
    bm_obj* recs = reinterpret_cast<bm_obj*>(h);
    for (size_t i = 0; i < m; ++i) recs[i] = b->objs[slots[i]];
    std::memcpy(h + rec, slots, m * sizeof(uint32_t));
    HIPTRY(bm_launch_slots_init(sh.stream, b->dev[s].d_obj.get(), b->dev[s].d_best.get(), b->dev[s].d_found.get(),
                                reinterpret_cast<const bm_obj*>(d), reinterpret_cast<const uint32_t*>(d + rec),
                                (uint32_t)m));
    HIPTRY(hipEventRecord(u->ev.get(), sh.stream));
    u->pending = true;
  }
  return 0;
}

// Append m objects to a live session (bmsched::add: released slots first, then the table grows --
// device buffers reallocated at twice the size and re-uploaded from the host mirror, after the
// batch's launches drained).  Otherwise only the slots written go up (init_slots), behind the
// launches in flight: the steppers go on.  lk holds the engine's mutex.
int batch_add_locked(std::unique_lock<std::mutex>& lk, bmpow_batch* b, size_t m, const uint8_t* ihs,
                     const uint64_t* targets, const uint64_t* start, uint32_t* slot_out,
                     const uint64_t* ih_off = nullptr) {
  if (b->generation != g_generation) return set_err(BMPOW_E_STATE, "device set changed under a live batch");
  const size_t fresh = m > b->free_slots.size() ? m - b->free_slots.size() : 0;
  if (b->n + fresh > 0xffffffffULL) return set_err(BMPOW_E_ARG, "too many objects");
  if (b->n + fresh > b->cap) quiesce(lk, b);  // the tables will be reallocated
  std::vector<uint32_t> slots;
  const bool grew = bmsched::add(*b, m, ihs, targets, start, slots, ih_off);
  if (slot_out) std::copy(slots.begin(), slots.end(), slot_out);
  if (grew) {
    b->cap = std::max<size_t>({b->n, 2 * b->cap, 1024});
    batch_free_dev(b);
    const int rc = batch_upload(lk, b);
    if (g_engine) g_engine->notify();
    return rc;
  }
  int rc = sync_vpool(lk, b);  // before the slots that use the new words are handed to the steppers' kernels
  if (rc == 0 && !b->vmoved.empty()) {  // a compaction moved live objects' words (sync_vpool drained)
    rc = init_slots(b, b->vmoved.data(), b->vmoved.size());
    b->vmoved.clear();
  }
  if (rc == 0) rc = init_slots(b, slots.data(), slots.size());
  if (g_engine) g_engine->notify();
  return rc;
}

// Stage the plan's per-shard item lists in the shards' pinned buffers (sized once per step, so
// nothing written is ever reallocated under the copy): the min-trial probe's staging.
int stage_items(const bmsched::StepPlan& p) {
  for (size_t s = 0; s < g_shards.size(); ++s) {
    ProbeShard& sh = g_probe[s];
    const std::vector<bm_item>& items = p.items[s];
    sh.nitems = 0;
    const int rc = ensure_items(sh, g_shards[s].dev, std::max<size_t>(items.size(), 1));
    if (rc < 0) return rc;
    if (!items.empty()) std::memcpy(sh.h_items.get(), items.data(), items.size() * sizeof(bm_item));
    sh.nitems = (uint32_t)items.size();
    // the counters after the items, zeroed here so the step's one upload resets them
    std::memset(sh.h_items.get() + sh.nitems, 0, (2 + (size_t)sh.nitems) * sizeof(unsigned long long));
    sh.d_trials = reinterpret_cast<unsigned long long*>(sh.d_items.get() + sh.nitems);
    sh.d_queue = sh.d_trials + 2;
    sh.nchunks = p.nchunks[s];
    sh.nmain = p.nmain.empty() ? sh.nitems : p.nmain[s];
    sh.chmain = p.chmain.empty() ? sh.nchunks : p.chmain[s];
  }
  return 0;
}

// ---- the engine's device side ----

// Stage and enqueue one launch on its shard's stream: items and zeroed counters up (one copy), the
// search kernel(s), the resolve kernel (each item's minimum and its trial value), results home.
int engine_launch(bmsched::Launch& L, std::string& err) {
  Shard& sh = g_shards[L.shard];
  LaunchBuf& lb = g_eng[L.shard].lb[L.buf];
  bmpow_batch* b = static_cast<bmpow_batch*>(L.batch);
  const std::vector<bm_item>& items = L.plan.items[0];
  const size_t n = items.size();
  int rc = ensure_launch_buf(g_eng[L.shard], sh.dev, lb.m, std::max<size_t>(n, 1));
  if (rc < 0) {
    err = g_err;
    return rc;
  }
  bm_item *const h_items = lb.m.h_items.get(), *const d_items = lb.m.d_items.get();
  std::memcpy(h_items, items.data(), n * sizeof(bm_item));
  std::memset(h_items + n, 0, (2 + n) * sizeof(unsigned long long));
  unsigned long long* d_trials = reinterpret_cast<unsigned long long*>(d_items + n);
  unsigned long long* d_queue = d_trials + 2;
  const uint32_t nmain = L.plan.nmain.empty() ? (uint32_t)n : L.plan.nmain[0];
  const uint32_t nch = L.plan.nchunks[0];
  const uint32_t chmain = L.plan.chmain.empty() ? nch : L.plan.chmain[0];
  // the batch's tables on this shard
  bm_obj* const d_obj = b->dev[L.shard].d_obj.get();
  unsigned long long* const d_best = b->dev[L.shard].d_best.get();
  uint32_t* const d_found = b->dev[L.shard].d_found.get();
  uint64_t* const d_vpool = b->dev[L.shard].d_vpool.get();
  bm_xbound xb;
  if (L.plan.nx) {
    xb.table = sh.d_xb;
    xb.row = (uint32_t)L.shard;
    xb.rows = (uint32_t)g_shards.size();
  }
  hipError_t e = hipSetDevice(sh.dev);
  if (e == hipSuccess)
    e = hipMemcpyAsync(d_items, h_items, stage_bytes(n), hipMemcpyHostToDevice, sh.stream);
  if (e == hipSuccess) e = hipEventRecord(lb.ev0.get(), sh.stream);
  if (e == hipSuccess && nmain)
    e = bm_launch_search(sh.stream, chmain, d_obj, d_items, nmain, d_best, d_found, d_trials, d_queue, xb);
  if (e == hipSuccess && n > nmain && nmain && xb.table)  // the var launch's relay counts its own columns
    e = hipMemsetAsync(d_trials + 1, 0, sizeof(unsigned long long), sh.stream);
  if (e == hipSuccess && n > nmain)
    e = bm_launch_search_var(sh.stream, nch - chmain, d_obj, d_items + nmain, (uint32_t)n - nmain, d_best, d_found,
                             d_trials, d_queue + nmain, xb, d_vpool);
  if (e == hipSuccess) e = hipEventRecord(lb.ev1.get(), sh.stream);
  if (e == hipSuccess)
    e = bm_launch_resolve(sh.stream, d_obj, d_items, (uint32_t)n, d_best, d_found, lb.m.d_res.get(), d_vpool, d_trials);
  if (e == hipSuccess)
    e = hipMemcpyAsync(lb.m.h_res.get(), lb.m.d_res.get(), (n + 1) * sizeof(bm_result), hipMemcpyDeviceToHost, sh.stream);
  if (e == hipSuccess) e = hipEventRecord(lb.evd.get(), sh.stream);
  if (e != hipSuccess) {
    err = std::string("search launch: ") + hipGetErrorString(e);
    return BMPOW_E_HIP;
  }
  return 0;
}

int engine_wait(bmsched::Launch& L, std::string& err) {
  Shard& sh = g_shards[L.shard];
  EngShard& es = g_eng[L.shard];
  LaunchBuf& lb = es.lb[L.buf];
  const hipEvent_t evd = lb.evd.get();
  hipError_t e = hipSetDevice(sh.dev);
  if (e == hipSuccess) {
    if (g_wait == kWaitSleep) {
      const auto t0 = std::chrono::steady_clock::now();
      while ((e = hipEventQuery(evd)) == hipErrorNotReady) {
        const int64_t waited = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
        std::this_thread::sleep_for(std::chrono::microseconds(std::min<int64_t>(1000, std::max<int64_t>(20, waited / 32))));
      }
    } else if (g_wait == kWaitPoll) {
      while ((e = hipEventQuery(evd)) == hipErrorNotReady) std::this_thread::sleep_for(std::chrono::microseconds(50));
    } else {
      e = hipEventSynchronize(evd);
    }
  }
  float ms = 0;
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, lb.ev0.get(), lb.ev1.get());
  if (e != hipSuccess) {
    err = std::string("search wait: ") + hipGetErrorString(e);
    return BMPOW_E_HIP;
  }
  es.t_prev_done = now_ms();
  const size_t n = L.plan.items[0].size();
  const bm_result* h_res = lb.m.h_res.get();
  L.res.assign(h_res, h_res + n);
  if (!es.retired.empty()) free_retired(es);  // here, outside the engine's mutex
  L.trials = h_res[n].nonce;  // the trials counter rides home after the results
  L.ms = ms;
  return 0;
}

int ensure_parts(ProbeShard& s, int dev, size_t n) {
  if (n <= s.d_parts.cap() && n <= s.h_parts.cap()) return 0;
  const size_t cap = std::max<size_t>(n, 2 * std::min(s.d_parts.cap(), s.h_parts.cap()));
  HIPTRY(s.d_parts.grow(dev, cap));
  HIPTRY(s.h_parts.grow(dev, cap, hipHostMallocDefault));
  return 0;
}

// Min-trial probe over n (object, range) pairs: min_out[i] = min{trial(m) : m in [start[i],
// start[i] + count[i])} (clipped at 2^64-1) and argmin_out[i] = the first such m reaching it.
// Steps of ~g_step_trials per shard; ranges are covered in ascending order, cut over the shards
// like a search step, and each workgroup's (trial, nonce) minimum is reduced here,
// lexicographically, so ties keep the smaller nonce.
int min_trial_locked(size_t n, const uint8_t* ihs, const uint64_t* start, const uint64_t* count, uint64_t* min_out,
                     uint64_t* argmin_out, const uint64_t* ih_off = nullptr) {
  if (n > 0xffffffffULL) return set_err(BMPOW_E_ARG, "too many objects");
  const size_t S = g_shards.size();
  std::vector<bm_obj> objs(n);
  std::vector<uint64_t> vpool;
  bool any_var = false;
  for (size_t i = 0; i < n; ++i) {
    bmsched::pack_var(bmsched::ih_ptr(ihs, ih_off, i), bmsched::ih_len(ih_off, i), 0, &objs[i], vpool);
    any_var = any_var || objs[i].ihlen != BM_IH_MAIN;
  }
  bmsched::MinTrial mt;
  mt.init(n, start, count, min_out, argmin_out);
  std::vector<DevBuf<bm_obj>> d_obj(S);  // released when the call returns
  std::vector<DevBuf<uint64_t>> d_vpool(S);
  int rc = 0;
  for (size_t s = 0; s < S && rc == 0; ++s) {
    Shard& sh = g_shards[s];
    hipError_t e = d_obj[s].alloc(sh.dev, std::max<size_t>(n, 1));
    if (e == hipSuccess && n)
      e = hipMemcpyAsync(d_obj[s].get(), objs.data(), n * sizeof(bm_obj), hipMemcpyHostToDevice, sh.stream);
    if (e == hipSuccess && !vpool.empty()) e = d_vpool[s].alloc(sh.dev, vpool.size());
    if (e == hipSuccess && !vpool.empty())
      e = hipMemcpyAsync(d_vpool[s].get(), vpool.data(), vpool.size() * sizeof(uint64_t), hipMemcpyHostToDevice, sh.stream);
    if (e != hipSuccess) rc = set_err(BMPOW_E_HIP, std::string("min-trial upload: ") + hipGetErrorString(e));
  }
  const uint64_t total_chunks = std::max<uint64_t>(g_step_trials * S / BM_CHUNK, S);
  bmsched::StepPlan plan;
  while (rc == 0) {
    if (g_abort.load()) {
      rc = set_err(BMPOW_E_ABORTED, "aborted");
      break;
    }
    uint64_t C = 0;
    if (!mt.plan(total_chunks, plan.wins, C)) break;
    bmsched::slice(plan.wins, C, BM_CHUNK, S, plan);
    bmsched::split_kinds(objs, any_var, plan);
    rc = stage_items(plan);
    if (rc < 0) break;
    for (size_t s = 0; s < S && rc == 0; ++s) {
      Shard& sh = g_shards[s];
      ProbeShard& pr = g_probe[s];
      if (pr.nitems == 0) continue;
      rc = ensure_parts(pr, sh.dev, pr.nchunks);
      if (rc < 0) break;
      bm_item* const d_items = pr.d_items.get();
      bm_minpart* const d_parts = pr.d_parts.get();
      hipError_t e = hipSetDevice(sh.dev);
      if (e == hipSuccess)
        e = hipMemcpyAsync(d_items, pr.h_items.get(), pr.nitems * sizeof(bm_item), hipMemcpyHostToDevice, sh.stream);
      if (e == hipSuccess) e = hipEventRecord(sh.ev0.get(), sh.stream);
      if (e == hipSuccess && pr.nmain)
        e = bm_launch_mintrial(sh.stream, pr.chmain, d_obj[s].get(), d_items, pr.nmain, d_parts);
      if (e == hipSuccess && pr.nitems > pr.nmain)
        e = bm_launch_mintrial_var(sh.stream, pr.nchunks - pr.chmain, d_obj[s].get(), d_items + pr.nmain,
                                   pr.nitems - pr.nmain, d_parts + pr.chmain, d_vpool[s].get());
      if (e == hipSuccess) e = hipEventRecord(sh.ev1.get(), sh.stream);
      if (e == hipSuccess)
        e = hipMemcpyAsync(pr.h_parts.get(), d_parts, pr.nchunks * sizeof(bm_minpart), hipMemcpyDeviceToHost, sh.stream);
      if (e != hipSuccess) rc = set_err(BMPOW_E_HIP, std::string("min-trial launch: ") + hipGetErrorString(e));
    }
    for (size_t s = 0; s < S && rc == 0; ++s) {
      Shard& sh = g_shards[s];
      const ProbeShard& pr = g_probe[s];
      if (pr.nitems == 0) continue;
      hipError_t e = hipSetDevice(sh.dev);
      if (e == hipSuccess) e = hipStreamSynchronize(sh.stream);
      float ms = 0;
      if (e == hipSuccess) e = hipEventElapsedTime(&ms, sh.ev0.get(), sh.ev1.get());
      if (e != hipSuccess) {
        rc = set_err(BMPOW_E_HIP, std::string("min-trial: ") + hipGetErrorString(e));
        break;
      }
      g_stats.probe_kernel_ms += ms;
      const std::vector<bm_item>& its = plan.items[s];
      const std::vector<bm_item> main_items(its.begin(), its.begin() + pr.nmain),
          var_items(its.begin() + pr.nmain, its.end());
      mt.reduce_parts(main_items, pr.h_parts.get(), min_out, argmin_out);
      if (!var_items.empty()) mt.reduce_parts(var_items, pr.h_parts.get() + pr.chmain, min_out, argmin_out);
    }
    if (rc < 0) break;
    for (const bmsched::Win& w : plan.wins) g_stats.probe_trials += w.count;
    mt.advance(plan.wins);
  }
  return rc;
}

// Library-owned scratch batch reused by the stateless entry points (bmpow_search*, bmpow_search_batch).
bmpow_batch* g_scratch = nullptr;

// Re-initialise the scratch batch with n objects and attach it.  Reused while it is large enough and
// the device set is unchanged: a run() call then writes its 128-B record into slot 0 behind whatever
// is still in flight there (the previous call's lookahead launch, which stops at once on that call's
// hit; its results are stale by the slot's generation), with no allocation and no host wait.
int scratch_batch(std::unique_lock<std::mutex>& lk, size_t n, const uint8_t* ihs, const uint64_t* targets,
                  const uint64_t* start, const uint64_t* ih_off = nullptr) {
  if (g_scratch && g_scratch->dev.size() == g_shards.size() && g_scratch->cap >= n) {
    g_engine->attach(lk, g_scratch);
    const size_t cap = g_scratch->cap;
    bmsched::init(*g_scratch, n, ihs, targets, start, ih_off);
    g_scratch->cap = cap;
    int rc = sync_vpool(lk, g_scratch);
    if (rc < 0) return rc;
    std::vector<uint32_t> slots(n);
    for (size_t i = 0; i < n; ++i) slots[i] = (uint32_t)i;
    return init_slots(g_scratch, slots.data(), n);
  }
  if (g_scratch) {
    if (g_engine->attached() == g_scratch) g_engine->detach(lk);
    batch_free_dev(g_scratch);
    delete g_scratch;
    g_scratch = nullptr;
  }
  g_scratch = new bmpow_batch();
  g_engine->detach(lk);  // nothing may run while the new tables are uploaded synchronously
  const int rc = batch_init(lk, g_scratch, n, ihs, targets, start, ih_off);
  if (rc == 0) g_engine->attach(lk, g_scratch);
  return rc;
}

// Drop the scratch batch (device set change, shutdown).  lk: the engine's mutex.
void drop_scratch(std::unique_lock<std::mutex>& lk) {
  if (!g_scratch) return;
  if (g_engine && g_engine->attached() == g_scratch) g_engine->detach(lk);
  batch_free_dev(g_scratch);
  delete g_scratch;
  g_scratch = nullptr;
}

}  // namespace bmhost

// ---------------------------------------------------------------------------------------
// Continuous-batching service (bmpow_service_*): bmsched::Service's stepper thread over a resident
// session, so no caller thread -- and no Python GIL -- sits between two steps.  Its ops take g_mu
// one at a time; the service's own mutex is never held with it.
// ---------------------------------------------------------------------------------------
struct bmpow_service {
  bmpow_batch* b = nullptr;  // resident session (ops run on the stepper thread, under g_mu)
  uint64_t budget = 0;       // trials per step (0 = library default)
  std::unique_ptr<bmsched::Service> svc;
};

namespace bmhost {

// Services not yet destroyed: bmpow_atexit stops their threads before it releases the devices.
std::mutex g_svc_mu;
std::vector<bmpow_service*> g_live_services;

void service_stop_all() {
  std::vector<bmpow_service*> live;
  {
    std::lock_guard<std::mutex> g(g_svc_mu);
    live = g_live_services;
  }
  for (bmpow_service* s : live) s->svc->stop();
}

// A service op finds the library shut down (bmpow_shutdown / resetPoW under a live service): an error
// the service reports through its poll, never a step on released devices.
int engine_gone(std::string& err) {
  err = "the library was shut down under this service";
  return BMPOW_E_STATE;
}

bmsched::ServiceOps service_ops(bmpow_service* s) {
  bmsched::ServiceOps ops;
  ops.add = [s](size_t n, const uint8_t* ihs, const uint64_t* ih_off, const uint64_t* tg, uint32_t* slots,
                std::string& err) {
    std::lock_guard<FairMutex> g(g_mu);
    if (!g_engine || s->b->generation != g_generation) return engine_gone(err);
    std::unique_lock<std::mutex> lk(g_engine->mu);
    const int rc = batch_add_locked(lk, s->b, n, ihs, tg, nullptr, slots, ih_off);
    if (rc < 0) err = g_err;
    return rc;
  };
  // let the steppers claim one round of launches (and keep one queued behind it) and return as soon
  // as an object finished, so the service hands it out while the devices go on
  ops.step = [s](std::string& err) {
    std::lock_guard<FairMutex> g(g_mu);
    if (!g_engine || s->b->generation != g_generation) return engine_gone(err);
    std::unique_lock<std::mutex> lk(g_engine->mu);
    g_engine->attach(lk, s->b);
    bmpow_batch* b = s->b;
    const uint64_t budget = (s->budget ? s->budget : g_step_trials.load()) * g_shards.size();
    // ... or as soon as a launch completes while another caller waits for the library (a serial run())
    return g_engine->run(lk, budget, true,
                         [b] { return b->finished_head < b->finished.size() || b->pending == 0 || g_mu.waiting() > 0; },
                         err);
  };
  ops.take = [s](size_t cap, uint32_t* slot, uint64_t* nonce, uint64_t* trial, uint8_t* done) -> size_t {
    std::lock_guard<FairMutex> g(g_mu);
    if (!g_engine) return 0;
    std::lock_guard<std::mutex> lk(g_engine->mu);
    return bmsched::take_done(*s->b, cap, slot, nonce, trial, done);
  };
  ops.reset = [s](std::string& err) {
    std::lock_guard<FairMutex> g(g_mu);
    if (!g_engine) return engine_gone(err);
    std::unique_lock<std::mutex> lk(g_engine->mu);
    if (g_engine->attached() == s->b) g_engine->detach(lk);
    batch_free_dev(s->b);
    delete s->b;
    s->b = new bmpow_batch();
    const int rc = batch_init(lk, s->b, 0, nullptr, nullptr, nullptr);
    if (rc < 0) err = g_err;
    return rc;
  };
  return ops;
}

}  // namespace bmhost

using namespace bmhost;

extern "C" {

int bmpow_trials_len(const uint8_t* ih, size_t ih_len, const uint64_t* nonces, size_t n, uint64_t* trials_out) {
  std::lock_guard<FairMutex> lk(g_mu);
  int rc = init_locked();
  if (rc < 0) return rc;
  if ((!ih && ih_len) || (n && (!nonces || !trials_out))) return set_err(BMPOW_E_ARG, "null pointer");
  if (ih_len > BMPOW_MAX_IH_LEN) return set_err(BMPOW_E_ARG, "initialHash longer than BMPOW_MAX_IH_LEN");
  if (n == 0) return 0;
  Shard& sh = g_shards[0];
  HIPTRY(hipSetDevice(sh.dev));
  bm_obj o;
  std::vector<uint64_t> vpool;
  const uint8_t zero = 0;
  bmsched::pack_var(ih ? ih : &zero, ih_len, 0, &o, vpool);
  DevBuf<bm_obj> d_o;  // the call's buffers: released when it returns
  DevBuf<uint64_t> d_n, d_t, d_v;
  HIPTRY(d_o.alloc(sh.dev, 1));
  HIPTRY(d_n.alloc(sh.dev, n));
  HIPTRY(d_t.alloc(sh.dev, n));
  if (!vpool.empty()) HIPTRY(d_v.alloc(sh.dev, vpool.size()));
  hipError_t e = hipMemcpyAsync(d_o.get(), &o, sizeof o, hipMemcpyHostToDevice, sh.stream);
  if (e == hipSuccess && d_v)
    e = hipMemcpyAsync(d_v.get(), vpool.data(), vpool.size() * sizeof(uint64_t), hipMemcpyHostToDevice, sh.stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_n.get(), nonces, n * sizeof(uint64_t), hipMemcpyHostToDevice, sh.stream);
  if (e == hipSuccess) e = bm_launch_trials(sh.stream, d_o.get(), d_n.get(), n, d_t.get(), d_v.get());
  if (e == hipSuccess) e = hipMemcpyAsync(trials_out, d_t.get(), n * sizeof(uint64_t), hipMemcpyDeviceToHost, sh.stream);
  if (e == hipSuccess) e = hipStreamSynchronize(sh.stream);
  if (e != hipSuccess) return set_err(BMPOW_E_HIP, std::string("bmpow_trials: ") + hipGetErrorString(e));
  return 0;
}

int bmpow_trials(const uint8_t ih[64], const uint64_t* nonces, size_t n, uint64_t* trials_out) {
  if (!ih) return set_err(BMPOW_E_ARG, "null pointer");
  return bmpow_trials_len(ih, 64, nonces, n, trials_out);
}

int bmpow_search(const uint8_t ih[64], uint64_t target, uint64_t start, uint64_t max_trials,
                 uint64_t* nonce_out, uint64_t* trial_out) {
  if (!ih) return set_err(BMPOW_E_ARG, "null pointer");
  return bmpow_search_len(ih, 64, target, start, max_trials, nonce_out, trial_out);
}

int bmpow_search_len(const uint8_t* ih, size_t ih_len, uint64_t target, uint64_t start, uint64_t max_trials,
                     uint64_t* nonce_out, uint64_t* trial_out) {
  std::lock_guard<std::timed_mutex> one(g_one_mu);
  std::unique_lock<FairMutex> g(g_mu);
  int rc = init_locked();
  if (rc < 0) return rc;
  if ((!ih && ih_len) || !nonce_out || !trial_out) return set_err(BMPOW_E_ARG, "null pointer");
  if (ih_len > BMPOW_MAX_IH_LEN) return set_err(BMPOW_E_ARG, "initialHash longer than BMPOW_MAX_IH_LEN");
  if (max_trials == 0) return BMPOW_NOT_FOUND;
  if (g_abort.load()) return set_err(BMPOW_E_ABORTED, "aborted");
  // every 64-byte object takes the single-object path, on any number of devices (round 5; before, only
  // one shard did and several took the engine's split windows)
  if (ih_len == 64 && g_one_enabled) return search_one(ih, target, start, max_trials, nonce_out, trial_out, g);
  const uint8_t zero = 0;
  const uint64_t off[2] = {0, ih_len};
  std::unique_lock<std::mutex> lk(g_engine->mu);
  rc = scratch_batch(lk, 1, ih ? ih : &zero, &target, &start, ih_len == 64 ? nullptr : off);
  if (rc < 0) return rc;
  bmpow_batch* b = g_scratch;
  // the search's last nonce: windows are cut there, so a hit past the caller's budget is never
  // reported (it resumes at start + max_trials and finds it again)
  b->lim[0] = (max_trials - 1 > kU64Max - start) ? kU64Max : start + max_trials - 1;
  std::string err;
  rc = g_engine->run(lk, kU64Max, false, [b] { return b->done[0] != BMPOW_PENDING; }, err);
  if (rc < 0) return set_err(rc, err);
  if (b->done[0] == BMPOW_DONE_FOUND) {
    *nonce_out = b->nonce[0];
    *trial_out = b->trial[0];
    return BMPOW_FOUND;
  }
  return BMPOW_NOT_FOUND;
}

int bmpow_min_trial(const uint8_t ih[64], uint64_t start, uint64_t count, uint64_t* min_out, uint64_t* argmin_out) {
  std::lock_guard<FairMutex> lk(g_mu);
  int rc = init_locked();
  if (rc < 0) return rc;
  if (!ih || !min_out || !argmin_out) return set_err(BMPOW_E_ARG, "null pointer");
  return min_trial_locked(1, ih, &start, &count, min_out, argmin_out);
}

int bmpow_min_trial_batch(size_t n, const uint8_t* ihs, const uint64_t* start, const uint64_t* count,
                          uint64_t* min_out, uint64_t* argmin_out) {
  std::lock_guard<FairMutex> lk(g_mu);
  int rc = init_locked();
  if (rc < 0) return rc;
  if (n == 0) return 0;
  if (!ihs || !start || !count || !min_out || !argmin_out) return set_err(BMPOW_E_ARG, "null pointer");
  return min_trial_locked(n, ihs, start, count, min_out, argmin_out);
}

// shared argument check of the *_var entry points: n + 1 ascending offsets, lengths in range
static int check_ih_offsets(size_t n, const uint8_t* ihs, const uint64_t* ih_off) {
  if (!ih_off || (!ihs && ih_off[n] > ih_off[0])) return set_err(BMPOW_E_ARG, "null pointer");
  for (size_t i = 0; i < n; ++i) {
    if (ih_off[i + 1] < ih_off[i]) return set_err(BMPOW_E_ARG, "initialHash offsets are not ascending");
    if (ih_off[i + 1] - ih_off[i] > BMPOW_MAX_IH_LEN)
      return set_err(BMPOW_E_ARG, "initialHash longer than BMPOW_MAX_IH_LEN");
  }
  return 0;
}

int bmpow_min_trial_var(size_t n, const uint8_t* ihs, const uint64_t* ih_off, const uint64_t* start,
                        const uint64_t* count, uint64_t* min_out, uint64_t* argmin_out) {
  std::lock_guard<FairMutex> lk(g_mu);
  int rc = init_locked();
  if (rc < 0) return rc;
  if (n == 0) return 0;
  if (!start || !count || !min_out || !argmin_out) return set_err(BMPOW_E_ARG, "null pointer");
  rc = check_ih_offsets(n, ihs, ih_off);
  if (rc < 0) return rc;
  const uint8_t zero = 0;
  return min_trial_locked(n, ihs ? ihs : &zero, start, count, min_out, argmin_out, ih_off);
}

int bmpow_search_batch(size_t n, const uint8_t* ihs, const uint64_t* targets, uint64_t* next_start,
                       uint64_t budget, uint64_t* nonce_out, uint64_t* trial_out, uint8_t* done) {
  std::lock_guard<FairMutex> g(g_mu);
  int rc = init_locked();
  if (rc < 0) return rc;
  if (n == 0) return 0;
  if (!ihs || !targets || !next_start || !nonce_out || !trial_out || !done)
    return set_err(BMPOW_E_ARG, "null pointer");
  if (g_abort.load()) return set_err(BMPOW_E_ABORTED, "aborted");
  std::unique_lock<std::mutex> lk(g_engine->mu);
  rc = scratch_batch(lk, n, ihs, targets, next_start);
  if (rc < 0) return rc;
  bmpow_batch* b = g_scratch;
  for (size_t i = 0; i < n; ++i) {
    if (done[i] != BMPOW_PENDING) {
      b->done[i] = done[i];
      b->pending--;
    }
  }
  if (budget == 0) budget = g_step_trials * g_shards.size();
  // no lookahead: every claim is applied when the call returns, so next_start is where the batch stands
  std::string err;
  rc = g_engine->run(lk, budget, false, [b] { return b->pending == 0; }, err);
  if (rc < 0) return set_err(rc, err);
  for (size_t i = 0; i < n; ++i) {
    if (done[i] != BMPOW_PENDING) continue;
    done[i] = b->done[i];
    next_start[i] = bmsched::resume_point(*b, i);
    if (b->done[i] == BMPOW_DONE_FOUND) {
      nonce_out[i] = b->nonce[i];
      trial_out[i] = b->trial[i];
    }
  }
  return (int)std::min<size_t>(b->pending, 0x7fffffff);
}

bmpow_batch* bmpow_batch_create(size_t n, const uint8_t* ihs, const uint64_t* targets, const uint64_t* start) {
  std::lock_guard<FairMutex> g(g_mu);
  if (init_locked() < 0) return nullptr;
  if (n && (!ihs || !targets)) {
    set_err(BMPOW_E_ARG, "null pointer");
    return nullptr;
  }
  if (n > 0xffffffffULL) {
    set_err(BMPOW_E_ARG, "too many objects");
    return nullptr;
  }
  std::unique_lock<std::mutex> lk(g_engine->mu);
  bmpow_batch* b = new bmpow_batch();
  if (batch_init(lk, b, n, ihs, targets, start) < 0) {
    batch_free_dev(b);
    delete b;
    return nullptr;
  }
  return b;
}

// Let the steppers claim ~budget trials of the batch (and one more launch per shard, which stays
// queued behind the running one when this returns, so consecutive calls keep every device busy).
int bmpow_batch_step(bmpow_batch* b, uint64_t budget) {
  std::lock_guard<FairMutex> g(g_mu);
  if (!b) return set_err(BMPOW_E_STATE, "null batch");
  if (!g_engine) return set_err(BMPOW_E_STATE, "library not initialised");
  if (b->generation != g_generation) return set_err(BMPOW_E_STATE, "device set changed under a live batch");
  if (g_abort.load()) return set_err(BMPOW_E_ABORTED, "aborted");
  std::unique_lock<std::mutex> lk(g_engine->mu);
  g_engine->attach(lk, b);
  if (budget == 0) budget = g_step_trials.load() * g_shards.size();
  std::string err;
  const int rc = g_engine->run(lk, budget, true, [b] { return b->pending == 0; }, err);
  if (rc < 0) return set_err(rc, err);
  return (int)std::min<size_t>(b->pending, 0x7fffffff);
}

int bmpow_batch_results(const bmpow_batch* b, uint64_t* nonce_out, uint64_t* trial_out, uint8_t* done,
                        uint64_t* next_start) {
  std::lock_guard<FairMutex> g(g_mu);
  if (!b) return set_err(BMPOW_E_STATE, "null batch");
  std::unique_lock<std::mutex> lk;
  if (g_engine) lk = std::unique_lock<std::mutex>(g_engine->mu);
  for (size_t i = 0; i < b->n; ++i) {
    if (nonce_out) nonce_out[i] = b->nonce[i];
    if (trial_out) trial_out[i] = b->trial[i];
    if (done) done[i] = b->done[i];
    if (next_start) next_start[i] = bmsched::resume_point(*b, i);
  }
  return (int)std::min<size_t>(b->pending, 0x7fffffff);
}

int bmpow_batch_reset(bmpow_batch* b, const uint64_t* start) {
  std::lock_guard<FairMutex> g(g_mu);
  if (!b) return set_err(BMPOW_E_STATE, "null batch");
  if (b->generation != g_generation || !g_engine) return set_err(BMPOW_E_STATE, "device set changed under a live batch");
  std::unique_lock<std::mutex> lk(g_engine->mu);
  quiesce(lk, b);
  bmsched::reset(*b, start);
  for (size_t s = 0; s < g_shards.size(); ++s) {
    Shard& sh = g_shards[s];
    HIPTRY(hipSetDevice(sh.dev));
    if (b->n) HIPTRY(hipMemsetAsync(b->dev[s].d_best.get(), 0xFF, b->n * sizeof(unsigned long long), sh.stream));
    if (b->n) HIPTRY(hipMemsetAsync(b->dev[s].d_found.get(), 0, b->n * sizeof(uint32_t), sh.stream));
  }
  if (const int rc = sync_shards(); rc < 0) return rc;
  g_engine->notify();
  return (int)std::min<size_t>(b->pending, 0x7fffffff);
}

int bmpow_batch_set_pending(bmpow_batch* b, size_t first, size_t count, int pending) {
  std::lock_guard<FairMutex> g(g_mu);
  if (!b) return set_err(BMPOW_E_STATE, "null batch");
  if (first > b->n || count > b->n - first) return set_err(BMPOW_E_ARG, "range outside the batch");
  std::unique_lock<std::mutex> lk;
  if (g_engine) lk = std::unique_lock<std::mutex>(g_engine->mu);
  bmsched::set_pending(*b, first, count, pending != 0);
  if (g_engine) g_engine->notify();
  return (int)std::min<size_t>(b->pending, 0x7fffffff);
}

int bmpow_batch_add(bmpow_batch* b, size_t n, const uint8_t* ihs, const uint64_t* targets, const uint64_t* start,
                    uint32_t* slot_out) {
  std::lock_guard<FairMutex> g(g_mu);
  if (!b) return set_err(BMPOW_E_STATE, "null batch");
  if (n == 0) return (int)std::min<size_t>(b->pending, 0x7fffffff);
  if (!ihs || !targets) return set_err(BMPOW_E_ARG, "null pointer");
  if (!g_engine) return set_err(BMPOW_E_STATE, "library not initialised");
  std::unique_lock<std::mutex> lk(g_engine->mu);
  const int rc = batch_add_locked(lk, b, n, ihs, targets, start, slot_out);
  if (rc < 0) return rc;
  return (int)std::min<size_t>(b->pending, 0x7fffffff);
}

int bmpow_batch_add_var(bmpow_batch* b, size_t n, const uint8_t* ihs, const uint64_t* ih_off, const uint64_t* targets,
                        const uint64_t* start, uint32_t* slot_out) {
  std::lock_guard<FairMutex> g(g_mu);
  if (!b) return set_err(BMPOW_E_STATE, "null batch");
  if (n == 0) return (int)std::min<size_t>(b->pending, 0x7fffffff);
  if (!targets) return set_err(BMPOW_E_ARG, "null pointer");
  if (!g_engine) return set_err(BMPOW_E_STATE, "library not initialised");
  int rc = check_ih_offsets(n, ihs, ih_off);
  if (rc < 0) return rc;
  const uint8_t zero = 0;
  std::unique_lock<std::mutex> lk(g_engine->mu);
  rc = batch_add_locked(lk, b, n, ihs ? ihs : &zero, targets, start, slot_out, ih_off);
  if (rc < 0) return rc;
  return (int)std::min<size_t>(b->pending, 0x7fffffff);
}

int bmpow_batch_take_done(bmpow_batch* b, size_t cap, uint32_t* slot_out, uint64_t* nonce_out, uint64_t* trial_out,
                          uint8_t* done_out) {
  std::lock_guard<FairMutex> g(g_mu);
  if (!b) return set_err(BMPOW_E_STATE, "null batch");
  if (cap && !slot_out) return set_err(BMPOW_E_ARG, "null pointer");
  std::unique_lock<std::mutex> lk;
  if (g_engine) lk = std::unique_lock<std::mutex>(g_engine->mu);
  const size_t k = bmsched::take_done(*b, std::min<size_t>(cap, 0x7fffffff), slot_out, nonce_out, trial_out, done_out);
  return (int)k;
}

void bmpow_batch_destroy(bmpow_batch* b) {
  std::lock_guard<FairMutex> g(g_mu);
  if (!b) return;
  if (g_engine) {
    std::unique_lock<std::mutex> lk(g_engine->mu);
    if (g_engine->attached() == b) g_engine->detach(lk);
  }
  batch_free_dev(b);
  delete b;
}

bmpow_service* bmpow_service_create(uint64_t step_budget, uint32_t flags) {
  bmpow_service* s = new bmpow_service();
  {
    std::lock_guard<FairMutex> g(g_mu);
    s->b = new bmpow_batch();
    if (init_locked() < 0) {
      delete s->b;
      delete s;
      return nullptr;
    }
    std::unique_lock<std::mutex> lk(g_engine->mu);
    if (batch_init(lk, s->b, 0, nullptr, nullptr, nullptr) < 0) {
      batch_free_dev(s->b);
      delete s->b;
      delete s;
      return nullptr;
    }
    s->budget = step_budget;
  }
  s->svc.reset(new bmsched::Service(service_ops(s), (flags & BMPOW_SERVICE_VERIFY) != 0));
  std::lock_guard<std::mutex> g(g_svc_mu);
  g_live_services.push_back(s);
  return s;
}

int bmpow_service_submit(bmpow_service* s, size_t n, const uint8_t* ihs, const uint64_t* targets,
                         uint64_t* tickets_out) {
  if (!s) return set_err(BMPOW_E_STATE, "null service");
  if (n && (!ihs || !targets)) return set_err(BMPOW_E_ARG, "null pointer");
  const int rc = s->svc->submit(n, ihs, targets, tickets_out);
  return rc < 0 ? set_err(rc, "service stopping") : rc;
}

int bmpow_service_submit_var(bmpow_service* s, size_t n, const uint8_t* ihs, const uint64_t* ih_off,
                             const uint64_t* targets, uint64_t* tickets_out) {
  if (!s) return set_err(BMPOW_E_STATE, "null service");
  if (n == 0) return 0;
  if (!targets) return set_err(BMPOW_E_ARG, "null pointer");
  int rc = check_ih_offsets(n, ihs, ih_off);
  if (rc < 0) return rc;
  const uint8_t zero = 0;
  rc = s->svc->submit(n, ihs ? ihs : &zero, targets, tickets_out, ih_off);
  return rc < 0 ? set_err(rc, "service stopping") : rc;
}

int bmpow_service_poll(bmpow_service* s, size_t cap, int timeout_ms, uint64_t* tickets, uint64_t* nonce_out,
                       uint64_t* trial_out, uint8_t* done_out) {
  if (!s) return set_err(BMPOW_E_STATE, "null service");
  if (cap && !tickets) return set_err(BMPOW_E_ARG, "null pointer");
  std::string err;
  const int rc = s->svc->poll(cap, timeout_ms, tickets, nonce_out, trial_out, done_out, err);
  if (rc < 0) g_err = err;
  return rc;
}

int bmpow_service_cancel(bmpow_service* s) {
  if (!s) return set_err(BMPOW_E_STATE, "null service");
  s->svc->cancel();
  return 0;
}

int bmpow_service_outstanding(bmpow_service* s) {
  if (!s) return set_err(BMPOW_E_STATE, "null service");
  return (int)std::min<size_t>(s->svc->outstanding(), 0x7fffffff);
}

void bmpow_service_stop(bmpow_service* s) {
  if (s) s->svc->stop();
}

void bmpow_service_destroy(bmpow_service* s) {
  if (!s) return;
  {
    std::lock_guard<std::mutex> g(g_svc_mu);
    g_live_services.erase(std::remove(g_live_services.begin(), g_live_services.end(), s), g_live_services.end());
  }
  s->svc.reset();  // joins the service thread after its current op
  std::lock_guard<FairMutex> g(g_mu);
  if (g_engine) {
    std::unique_lock<std::mutex> lk(g_engine->mu);
    if (g_engine->attached() == s->b) g_engine->detach(lk);
  }
  batch_free_dev(s->b);
  delete s->b;
  delete s;
}

unsigned long long BitmessagePOW(unsigned char* starthash, unsigned long long target) {
  uint64_t start = 1, nonce = 0, tv = 0;
  for (;;) {
    const uint64_t budget = 1ULL << 34;
    int rc = bmpow_search(starthash, target, start, budget, &nonce, &tv);
    if (rc == BMPOW_FOUND) return nonce;
    if (rc < 0) return 0;
    if (start > kU64Max - budget) return 0;
    start += budget;
  }
}

}  // extern "C"
