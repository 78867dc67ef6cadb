// bmpow_host.hip -- C ABI (include/bmpow.h) and host scheduler of libbmpow_hip.so.
//
// Replaces the reference's native PoW entry points:
//   BitmessagePOW          src/bitmsghash/bitmsghash.cpp:127-165  (pthreads + OpenSSL)
//   do_opencl_pow/initCL   src/openclpow.py:31-111                (pyopencl window loop)
//
// Scheduler (round 4: per-device stepping, bmsched::Engine in bmpow_sched.cpp).  One stepper thread
// and stream per shard (device, or a stream of one).  Whenever a shard has fewer than two launches
// in flight, its stepper claims windows from the objects' frontiers under the engine's mutex --
// its fair share of the objects, each a window of its step's budget, or one piece each of windows
// split over every shard when fewer objects than shards are pending -- and enqueues the launch
// behind the running one: items up, bm_search_kernel (+ the var-form kernel), bm_resolve_kernel,
// results home.  When a launch completes, its per-item minima are folded into the objects (the host
// min-reduction over shards; no RCCL: no data moves between GPUs); an object is final once every
// window below its least hit has completed on whichever shard ran it.  No shard waits for another.
// The entry points (bounded searches, batch steps, the service) let the steppers claim a trial
// budget and wait for what they need, so the caller polls its shutdown flag between bounded calls
// (dev/powinterrupttest.py:22-37).
//
// The host units (bmpow_host.h is what they share; each holds its subsystem's C-ABI entry points):
//   bmpow_host.hip         knobs, the shard set, init / shutdown / the exit hook, device + stats entry points
//   bmpow_host_batch.hip   batch tables, the engine's device side, min-trial probe, searches, the service
//   bmpow_host_one.hip     run()'s single-object path and the streams kept for it
//   bmpow_host_verify.hip  receive-side verification;   bmpow_host_addr.hip  the address search
//   bmpow_host_ecies.hip   ECIES trial decryption of received msgs (include/bmpow_ecies.h)
//   bmpow_host_intake.hip  object intake: inventory hashes, header walk and checks (include/bmpow_intake.h)
//   bmpow_host_packets.hip packet framing in front of the intake: checksums, verdicts (include/bmpow_packets.h)
//   bmpow_host_inv.hip     the inventory sets behind them: have and missing on the device (include/bmpow_inv.h)
//   bmpow_host_proc.hip    the object processor's queue: acks, getpubkeys, onionpeers, routes (include/bmpow_proc.h)
//   bmpow_host_sig.hip     ECDSA signature verification of received objects (include/bmpow_sig.h)
//   bmpow_host_send.hip    public keys, signatures and ECIES encryption of outgoing objects (include/bmpow_send.h)
//   bmpow_host_seal.hip    the seal and CBC kernels' round trip;   bmpow_host_tx.hip  outgoing objects in one call
// and what groups of them share: bmpow_host_scalar.h (host only: scalars, range checks, padding, DER, draws,
// cleansed host owners), bmpow_host_sendkit.h (the send side: KeySet, the sign-again loop, the wall-clock
// guard), bmpow_seal_plan.h (host only: slots, sets), bmpow_host_sig.h / bmpow_host_rows.h (the receive side).
#include "bmpow_host.h"

namespace bmhost {

bool g_inited = false;

// Release the shard set.  The order stays: per shard its stream drains first, then every subsystem's
// buffers on it (each owner frees on the device it was allocated for), the shard's events, the stream last.
void free_shards() {
  for (Shard& s : g_shards) {
    if (s.dev < 0 || !s.stream) continue;
    (void)hipSetDevice(s.dev);
    (void)hipStreamSynchronize(s.stream);
  }
  engine_release_shards();
  probe_release_shards();
  verify_release_shards();
  addr_release_shards();
  intake_release_shards();
  packets_release_shards();
  inv_release_shards();
  proc_release_shards();
  for (Shard& s : g_shards) {
    s.ev0.reset();
    s.ev1.reset();
    if (s.stream) (void)hipSetDevice(s.dev), (void)hipStreamDestroy(s.stream);
  }
  g_shards.clear();
}

int make_shard(int dev, Shard& s) {
  s.dev = dev;
  HIPTRY(hipSetDevice(dev));
  HIPTRY(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
  HIPTRY(s.ev0.alloc(dev));
  HIPTRY(s.ev1.alloc(dev));
  HIPTRY(hipDeviceGetAttribute(&s.cus, hipDeviceAttributeMultiprocessorCount, dev));
  s.resident = (uint32_t)std::max(1, bm_search_resident_per_cu()) * (uint32_t)s.cus;
  if (const char* e = std::getenv("BMPOW_COLUMNS"))  // A/B knob: columns per shard and window
    if (std::atoi(e) > 0) s.resident = (uint32_t)std::atoi(e);
  return 0;
}

int sync_shards() {
  for (auto& sh : g_shards) {
    HIPTRY(hipSetDevice(sh.dev));
    HIPTRY(hipStreamSynchronize(sh.stream));
  }
  return 0;
}

// The streams whose kernels overlap on one device: its hardware queues (GPU_MAX_HW_QUEUES, HIP's default 4).
uint32_t hw_queues() {
  if (const char* e = std::getenv("GPU_MAX_HW_QUEUES"))
    if (std::atoi(e) > 0) return (uint32_t)std::atoi(e);
  return 4;
}

std::vector<int> visible_gfx950() {
  std::vector<int> out;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return out;
  for (int i = 0; i < n; ++i) {
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, i) != hipSuccess) continue;
    if (std::strncmp(p.gcnArchName, "gfx950", 6) == 0) out.push_back(i);
  }
  return out;
}

double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// Hand the engine its device groups (one per physical device, or every shard its own under
// bmpow_set_engine_split) and the matching column cap; drains what is in flight.
void apply_engine_groups() {
  if (!g_engine) return;
  std::vector<uint16_t> group;
  uint32_t resident = g_resident;
  if (!g_engine_split) {
    std::vector<int> devs;
    for (const Shard& sh : g_shards) {
      size_t g = (size_t)(std::find(devs.begin(), devs.end(), sh.dev) - devs.begin());
      if (g == devs.size()) devs.push_back(sh.dev);
      group.push_back((uint16_t)g);
    }
    resident = g_dev_resident;
  }
  std::unique_lock<std::mutex> lk(g_engine->mu);
  g_engine->set_groups(lk, group, resident);
}

int select_devices(const std::vector<int>& ids) {
  ++g_generation;  // whatever was built for the old set is stale, whether or not the new one is as large
  g_engine.reset();  // joins the steppers once their launches are applied
  free_one();
  free_shards();
  if (ids.size() > BM_MAX_SHARDS) return set_err(BMPOW_E_ARG, "more than BM_MAX_SHARDS shards");
  const auto vis = visible_gfx950();
  for (int id : ids) {
    if (std::find(vis.begin(), vis.end(), id) == vis.end())
      return set_err(BMPOW_E_ARG, "device " + std::to_string(id) + " is not a visible gfx950 device");
  }
  g_shards.resize(ids.size());
  for (size_t i = 0; i < ids.size(); ++i) {
    int rc = make_shard(ids[i], g_shards[i]);
    if (rc < 0) return rc;
  }
  if (const int rc = batch_init_shards(); rc < 0) return rc;
  if (!g_xb) {
    HIPTRY(g_xb.alloc(g_shards[0].dev, (size_t)BM_MAX_SHARDS * BM_XSLOTS,
                      hipHostMallocPortable | hipHostMallocMapped | hipHostMallocCoherent));
    for (size_t i = 0; i < g_xb.cap(); ++i) g_xb[i] = ~0ULL;
  }
  g_resident = ~0u;
  g_dev_resident = ~0u;
  for (auto& sh : g_shards) {
    HIPTRY(hipSetDevice(sh.dev));
    void* dp = nullptr;
    HIPTRY(hipHostGetDevicePointer(&dp, g_xb.get(), 0));
    sh.d_xb = (unsigned long long*)dp;
    // Shards sharing a device split its resident workgroups -- over the kernels that can run at once:
    // the device's hardware queues (GPU_MAX_HW_QUEUES, HIP's default 4) bound the streams whose
    // kernels overlap, so 8 shards on one GPU get a quarter of it each, not an eighth (an eighth left 2
    // waves per SIMD while 4 shards ran: 5.5 against 6.7 GH/s, profiles/r04/final/).
    const uint32_t same = (uint32_t)std::count_if(g_shards.begin(), g_shards.end(),
                                                  [&](const Shard& o) { return o.dev == sh.dev; });
    const uint32_t hwq = hw_queues();
    g_resident = std::min<uint32_t>(g_resident, std::max<uint32_t>(1, sh.resident / std::min(same, hwq)));
    g_dev_resident = std::min<uint32_t>(g_dev_resident, std::max<uint32_t>(1, sh.resident));
  }
  make_engine();
  apply_engine_groups();
  return (int)g_shards.size();
}

bool g_exited = false;  // bmpow_atexit ran: no stream may be created again (see g_masked)

int init_locked() {
  if (g_exited) return set_err(BMPOW_E_STATE, "the process is exiting (bmpow_atexit ran)");
  if (g_inited) return (int)g_shards.size();
  if (const char* w = std::getenv("BMPOW_WAIT"))
    g_wait = std::strcmp(w, "spin") == 0    ? kWaitSpin
             : std::strcmp(w, "poll") == 0  ? kWaitPoll
             : std::strcmp(w, "block") == 0 ? kWaitBlock
                                            : kWaitSleep;
  if (const char* w = std::getenv("BMPOW_WAIT1"))
    g_one_wait = std::strcmp(w, "spin") == 0 ? kOneSpin : std::strcmp(w, "sleep") == 0 ? kOneSleep : kOneAuto;
  if (const char* w = std::getenv("BMPOW_ONE_QUERY")) g_one_query = std::max(0, std::atoi(w));
  if (const char* w = std::getenv("BMPOW_ONE_EVENT")) g_one_event = std::atoi(w) != 0;
  if (const char* w = std::getenv("BMPOW_SPLIT_CUMASK")) g_split_cumask = std::atoi(w) != 0;
  if (const char* w = std::getenv("BMPOW_SPIN_YIELD")) g_spin_yield = std::atoi(w) != 0;
  if (const char* w = std::getenv("BMPOW_ONE")) g_one_enabled = std::atoi(w) != 0;
  if (const char* w = std::getenv("BMPOW_TRACE")) g_trace = std::atoi(w) != 0;
  if (const char* w = std::getenv("BMPOW_RUN_STREAM")) g_run_stream = std::atoi(w) != 0;
  const auto vis = visible_gfx950();
  // Release everything at exit, before the HIP runtime's own exit handlers: they were registered when
  // the runtime initialised (by the call above), and atexit runs handlers last-registered first.  Without
  // it the stepper threads were joined by g_engine's static destructor, and the streams kept for the
  // process destroyed by the runtime, after its teardown (a traced process with CU-masked streams alive
  // ended in a segfault inside the runtime's exit handlers, round 5).
  static bool hooked = false;
  if (!hooked) {
    hooked = true;
    std::atexit(bmpow_atexit);
  }
  if (vis.empty()) return set_err(BMPOW_E_NODEV, "no gfx950 (MI355X) device visible to the HIP runtime");
  std::vector<int> ids = vis;
  if (const char* e = std::getenv("BMPOW_BLOCKS_PER_WORKER"))  // A/B knob
    if (std::atoi(e) > 0) bmsched::g_blocks_per_worker = (uint32_t)std::atoi(e);
  if (const char* env = std::getenv("BMPOW_DEVICES")) {
    ids.clear();
    std::string e(env);
    size_t pos = 0;
    while (pos <= e.size()) {
      size_t c = e.find(',', pos);
      std::string tok = e.substr(pos, c == std::string::npos ? std::string::npos : c - pos);
      if (!tok.empty()) ids.push_back(std::atoi(tok.c_str()));
      if (c == std::string::npos) break;
      pos = c + 1;
    }
    if (ids.empty()) return set_err(BMPOW_E_ARG, "BMPOW_DEVICES names no device");
  }
  int rc = select_devices(ids);
  if (rc < 0) return rc;
  g_inited = true;
  return rc;
}

}  // namespace bmhost

using namespace bmhost;

// =======================================================================================
// C ABI
// =======================================================================================
extern "C" {

int bmpow_init(void) {
  std::lock_guard<FairMutex> lk(g_mu);
  return init_locked();
}

int bmpow_device_count(void) { return (int)visible_gfx950().size(); }

int bmpow_set_devices(const int* ids, int n) {
  std::lock_guard<std::timed_mutex> one(g_one_mu);
  std::lock_guard<FairMutex> lk(g_mu);
  if (n < 0) return set_err(BMPOW_E_ARG, "bad device list");
  std::vector<int> v;
  if (n == 0) {
    v = visible_gfx950();
  } else if (!ids) {  // the first n visible devices (int bmpow_set_devices(int ndev))
    v = visible_gfx950();
    if ((size_t)n > v.size())
      return set_err(BMPOW_E_ARG, std::to_string(n) + " devices asked for, " + std::to_string(v.size()) + " visible");
    v.resize((size_t)n);
  } else {
    v.assign(ids, ids + n);
  }
  if (g_engine) {
    std::unique_lock<std::mutex> el(g_engine->mu);
    drop_scratch(el);
    g_engine->detach(el);
  }
  if (v.empty()) return set_err(BMPOW_E_NODEV, "no gfx950 (MI355X) device visible to the HIP runtime");
  int rc = select_devices(v);
  g_inited = rc > 0;
  return rc;
}

int bmpow_set_device_count(int ndev) {
  if (ndev < 1) return set_err(BMPOW_E_ARG, "device count must be >= 1");
  return bmpow_set_devices(nullptr, ndev);
}

int bmpow_get_devices(int* ids, int cap) {
  std::lock_guard<FairMutex> lk(g_mu);
  for (int i = 0; i < (int)g_shards.size() && i < cap; ++i) ids[i] = g_shards[i].dev;
  return (int)g_shards.size();
}

int bmpow_device_pci_bus_id(int device, char* out, int len) {
  if (!out || len < 13) return set_err(BMPOW_E_ARG, "buffer too small");
  const hipError_t e = hipDeviceGetPCIBusId(out, len, device);
  if (e != hipSuccess) return set_err(BMPOW_E_ARG, std::string("hipDeviceGetPCIBusId: ") + hipGetErrorString(e));
  return 0;
}

int bmpow_get_shard_rates(double* rates, int cap) {
  std::lock_guard<FairMutex> lk(g_mu);
  if (!rates && cap > 0) return set_err(BMPOW_E_ARG, "null pointer");
  if (!g_engine) return 0;
  std::lock_guard<std::mutex> el(g_engine->mu);
  const std::vector<double>& ema = g_engine->rates.ema;
  for (int i = 0; i < (int)g_shards.size() && i < cap; ++i) rates[i] = i < (int)ema.size() ? ema[i] : 0.0;
  return (int)g_shards.size();
}

static void shutdown_locked() {
  if (g_engine) {
    std::unique_lock<std::mutex> el(g_engine->mu);
    drop_scratch(el);
    g_engine->detach(el);
  }
  ++g_generation;
  g_engine.reset();
  free_one();
  free_shards();
  g_xb.reset();
  g_inited = false;
}

void bmpow_shutdown(void) {
  std::lock_guard<std::timed_mutex> one(g_one_mu);
  std::lock_guard<FairMutex> lk(g_mu);
  shutdown_locked();
}

void bmpow_atexit(void) {
  // No HIP call during static destruction: whichever way this hook returns -- after its own shutdown, or
  // giving up because another thread is still inside a call -- the owners (bmpow_own.h) that the library's
  // statics still hold are forgotten, not freed, by their destructors: those run after the runtime's own
  // exit handlers.  (This hook is registered after the statics are constructed, so it runs before them.)
  struct Exiting {
    ~Exiting() { bmown::g_exiting.store(true); }
  } exiting;
  // the services' threads step the engine: stopped (joined after their current op) first
  service_stop_all();
  // a call still running in another thread (a daemon thread at interpreter exit) keeps the library
  std::unique_lock<std::timed_mutex> one(g_one_mu, std::chrono::milliseconds(5000));
  if (!one.owns_lock() || !g_mu.try_lock_for(std::chrono::milliseconds(5000))) return;
  if (!g_exited) {
    g_exited = true;
    shutdown_locked();
    // the streams kept for the life of the process (no stream is created after this: init refuses)
    for (const MaskedStream& m : g_masked) {
      (void)hipSetDevice(m.dev);
      (void)hipStreamSynchronize(m.stream);
      (void)hipStreamDestroy(m.stream);
    }
    g_masked.clear();
    for (const auto& r : g_run_streams) {
      (void)hipSetDevice(r.first);
      (void)hipStreamSynchronize(r.second);
      (void)hipStreamDestroy(r.second);
    }
    g_run_streams.clear();
  }
  g_mu.unlock();
}

const char* bmpow_last_error(void) { return g_err.c_str(); }

const char* bmpow_version(void) {
  static char buf[160];
  // BM_SRC_ID (the Makefile: an md5 of every source and header the library is built from) identifies
  // the library a bench line or profile came from; no build time, so a rebuild of the same sources in
  // the same tree gives the same file (bench.py compares the PMC passes' library md5 with the benched one)
#ifndef BM_SRC_ID
#define BM_SRC_ID "unknown"
#endif
  std::snprintf(buf, sizeof buf, "bmpow %d gfx950 block=%d iters=%d src %s", BMPOW_ABI_VERSION, BM_BLOCK, BM_ITERS,
                BM_SRC_ID);
  return buf;
}

void bmpow_abort(void) { g_abort.store(1); }
void bmpow_clear_abort(void) { g_abort.store(0); }

int bmpow_get_stats(bmpow_stats* out) {
  std::lock_guard<FairMutex> lk(g_mu);
  if (!out) return BMPOW_E_ARG;
  *out = g_stats;
  out->masked_streams = g_masked.size();
  out->run_streams = g_run_streams.size();
  if (g_engine) {  // the searches: the engine's launches
    std::lock_guard<std::mutex> el(g_engine->mu);
    const bmsched::EngineStats& es = g_engine->stats;
    out->launches += es.launches;
    out->trials += es.trials;
    out->kernel_ms += es.kernel_ms;
    out->steps += es.launches;
    double mx = 0;
    for (double ms : es.shard_ms) mx = std::max(mx, ms);
    out->max_shard_kernel_ms += mx;
    out->past_window += es.waste.window;
    out->past_later += es.waste.later;
    out->past_split += es.waste.split;
    out->engine_hashed_est += es.waste.hashed;
  }
  return 0;
}

void bmpow_reset_stats(void) {
  std::lock_guard<FairMutex> lk(g_mu);
  g_stats = bmpow_stats{};
  one_reset_stats();
  if (g_engine) {
    std::lock_guard<std::mutex> el(g_engine->mu);
    bmsched::EngineStats& es = g_engine->stats;
    const size_t S = es.shard_ms.size();
    es = bmsched::EngineStats();
    es.shard_ms.assign(S, 0.0);
    es.shard_trials.assign(S, 0);
  }
}

int bmpow_get_shard_stats(uint64_t* trials, double* kernel_ms, int cap) {
  std::lock_guard<FairMutex> lk(g_mu);
  if (!g_engine) return 0;
  std::lock_guard<std::mutex> el(g_engine->mu);
  const bmsched::EngineStats& es = g_engine->stats;
  for (int i = 0; i < (int)es.shard_ms.size() && i < cap; ++i) {
    // the engine's launches and run()'s single-object pieces on the shard
    if (trials) trials[i] = es.shard_trials[i];
    if (kernel_ms) kernel_ms[i] = es.shard_ms[i];
    one_add_stats((size_t)i, trials ? trials + i : nullptr, kernel_ms ? kernel_ms + i : nullptr);
  }
  return (int)g_shards.size();
}

int bmpow_set_engine_split(int per_shard) {
  std::lock_guard<FairMutex> lk(g_mu);
  const int prev = g_engine_split ? 1 : 0;
  if (per_shard < 0) return prev;
  if ((per_shard != 0) != g_engine_split) {
    g_engine_split = per_shard != 0;
    apply_engine_groups();
  }
  return prev;
}

int bmpow_get_thread_info(double* cpu_s, int* policy, int cap) {
  std::lock_guard<FairMutex> lk(g_mu);
  if (!g_engine) return 0;
  std::vector<double> c;
  std::vector<int> p;
  {
    std::lock_guard<std::mutex> el(g_engine->mu);
    g_engine->thread_info(c, p);
  }
  for (int i = 0; i < (int)c.size() && i < cap; ++i) {
    if (cpu_s) cpu_s[i] = c[i];
    if (policy) policy[i] = p[i];
  }
  return (int)c.size();
}

int bmpow_set_shard_throttle(int shard, double ms) {
  std::lock_guard<FairMutex> lk(g_mu);
  if (!g_engine) return set_err(BMPOW_E_STATE, "library not initialised");
  if (shard < 0 || shard >= (int)g_shards.size() || !(ms >= 0)) return set_err(BMPOW_E_ARG, "bad shard or delay");
  g_engine->set_throttle((size_t)shard, ms);
  return 0;
}

uint64_t bmpow_get_step_trials(void) { return g_step_trials.load(); }

void bmpow_set_step_trials(uint64_t t) {
  std::lock_guard<FairMutex> lk(g_mu);
  g_step_trials.store(t ? std::max<uint64_t>(t, BM_CHUNK) : kDefaultStepTrials);
  if (g_engine) {
    std::lock_guard<std::mutex> el(g_engine->mu);
    g_engine->set_step_trials(g_step_trials.load());
  }
}

}  // extern "C"
