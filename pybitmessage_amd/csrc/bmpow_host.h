// bmpow_host.h -- what the host units of libbmpow_hip.so share (internal; the map of the units is in
// bmpow_host.hip): the library's locks, error string, knobs, the shard set and the engine.
//
// Lock order, everywhere: g_one_mu, then g_mu, then the engine's mutex (g_engine->mu).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include <sched.h>

#include "../../include/bmpow.h"
#include "bmpow_kernels.h"
#include "bmpow_sched.h"
#include "bmpow_own.h"

namespace bmhost {

constexpr uint64_t kU64Max = ~0ULL;
// Per shard per launch: ~80 ms on one MI355X, the interrupt granularity of a batch.  Against 2^28, the
// launch's tail and the host's planning between launches cost half as much: C2 6.683 / 6.679 against
// 6.668 / 6.658 GH/s, the C5 sample 6.667 / 6.674 against 6.662 / 6.664 (same box, twice each;
// 2^30 no better; profiles/r03/step_trials_ab.txt).
constexpr uint64_t kDefaultStepTrials = 1ULL << 29;

inline thread_local std::string g_err;
// A first-come first-served mutex.  The library's entry points take it one at a time, and the batch
// service's thread takes it for every step (up to a launch, ~80 ms) and again right after: with a plain
// std::mutex a serial run() beside a busy service waited 0.3-36 s for it -- until the batch was nearly
// done (tools/diag/run_beside_service.py, profiles/r05/run_beside_service/).  Tickets hand it out in
// arrival order, and waiting() lets a service step end at its next completed launch when a caller waits.
class FairMutex {
 public:
  void lock() {
    std::unique_lock<std::mutex> lk(m_);
    const uint64_t t = next_.fetch_add(1, std::memory_order_relaxed);
    cv_.wait(lk, [&] { return serving_.load(std::memory_order_relaxed) == t; });
  }
  void unlock() {
    {
      std::lock_guard<std::mutex> lk(m_);
      serving_.fetch_add(1, std::memory_order_relaxed);
    }
    cv_.notify_all();
  }
  // take the lock only if it comes free (no holder, no one queued) within d; false otherwise (the
  // process's exit hook: a call still running in another thread is left alone)
  bool try_lock_for(std::chrono::milliseconds d) {
    std::unique_lock<std::mutex> lk(m_);
    if (!cv_.wait_for(lk, d, [&] {
          return serving_.load(std::memory_order_relaxed) == next_.load(std::memory_order_relaxed);
        }))
      return false;
    next_.fetch_add(1, std::memory_order_relaxed);  // our ticket is the one being served
    return true;
  }
  // threads waiting for the lock (while one holds it)
  uint64_t waiting() const {
    const uint64_t n = next_.load(std::memory_order_relaxed), s = serving_.load(std::memory_order_relaxed);
    return n > s + 1 ? n - s - 1 : 0;
  }

 private:
  std::mutex m_;
  std::condition_variable cv_;
  std::atomic<uint64_t> next_{0}, serving_{0};
};
inline FairMutex g_mu;  // one entry point at a time (the steppers never take it)
// run()'s single-object state (g_ones, g_xone, the call ring, the streams run() launches on): held by a
// 64-byte run() for its whole call -- which releases g_mu while it waits for its windows, so the batch
// service steps between them -- and by every entry point that frees or re-plans that state (device
// selection, shutdown, the split knob).  Taken before g_mu (the lock order above).
inline std::timed_mutex g_one_mu;
inline std::atomic<int> g_abort{0};
inline std::atomic<uint64_t> g_step_trials{kDefaultStepTrials};  // read without the lock (bmpow_get_step_trials)

inline int set_err(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

#define HIPTRY(expr)                                                                            \
  do {                                                                                          \
    hipError_t e_ = (expr);                                                                     \
    if (e_ != hipSuccess)                                                                       \
      return set_err(BMPOW_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));           \
  } while (0)

// How a stepper waits for its launch (BMPOW_WAIT, read once):
//   "sleep" (default): query the launch's event and sleep between queries for 1/32 of the time waited
//     so far (20 us .. 1 ms) -- a few hundred queries per second of launch, and while two launches
//     are in flight a late wake-up costs the GPU nothing (the next launch is already queued);
//   "block": hipEventSynchronize on an event created with hipEventBlockingSync, with the device's
//     hipDeviceScheduleBlockingSync flag set (measured on MI355X: without the flag the wait spins at
//     one CPU per stepper, profiles/r04/);
//   "spin": HIP's default wait (busy); "poll": query the event every 50 us.
enum WaitMode { kWaitSleep, kWaitBlock, kWaitSpin, kWaitPoll };
inline WaitMode g_wait = kWaitSleep;
// run()'s single-object path (search_one): BMPOW_WAIT1 "auto" (default) spins on the result word when
// the call's answer is due within a few ms and sleeps between polls otherwise, "spin" / "sleep" force
// one (A/B); BMPOW_ONE=0 sends run() through the engine instead (A/B).
enum OneWait { kOneAuto, kOneSpin, kOneSleep };
inline OneWait g_one_wait = kOneAuto;
// The wait's fault check: an event recorded behind each launch, queried every g_one_query sleeping
// polls (BMPOW_ONE_QUERY=N, 0: never).  BMPOW_ONE_EVENT=0 queries the stream instead (A/B):
// hipStreamQuery cost the process 0.13 - 1.0 CPU-s per s during a 2^33 sweep, an event query 0.012
// (tools/diag/one_cpu.py, profiles/r05/one_cpu.jsonl).
inline int g_one_query = 8;
inline bool g_one_event = true;
inline bool g_spin_yield = true;  // BMPOW_SPIN_YIELD=0: a spinning wait never yields (A/B)
// Forced pieces that share a device each run on their own slice of its CUs (a CU-masked stream, CUs
// [j N / m, (j + 1) N / m) of the mask for piece j of m -- the mask's bits are dealt to the XCDs in turn,
// so a slice holds N / 8m CUs of every XCD): the pieces then never compete for a SIMD, as pieces on
// separate GPUs do not (tools/diag/cumask_probe.hip: 8 streams of 32 CUs each run side by side).
// BMPOW_SPLIT_CUMASK=0 shares the whole device instead (A/B).
inline bool g_split_cumask = true;
inline bool g_one_enabled = true;
// BMPOW_TRACE=1: the single-object path's set-up and tear-down steps on stderr, with the state of every
// stream they wait on (a diagnostic; tools/diag/rss_layout.py).
inline bool g_trace = false;
inline bool g_run_stream = true;  // run() on its own stream per device (run_stream); BMPOW_RUN_STREAM=0: the shard's
double now_ms();  // steady clock
#define BM_TRACE(...)                                                     \
  do {                                                                     \
    if (g_trace) {                                                         \
      std::fprintf(stderr, "[bmpow %.3f] ", now_ms());                     \
      std::fprintf(stderr, __VA_ARGS__);                                   \
      std::fputc('\n', stderr);                                            \
    }                                                                      \
  } while (0)

using bmown::DevBuf;
using bmown::Event;
using bmown::PinBuf;
using bmown::WipeDevBuf;

// The device time between two completed events, added to acc: the one way a unit's per-phase counters are fed.
inline int elapsed(double& acc, const Event& a, const Event& b) {
  float ms = 0;
  HIPTRY(hipEventElapsedTime(&ms, a.get(), b.get()));
  acc += ms;
  return 0;
}

// k consecutive phases: ev[i] .. ev[i + 1] into *acc[i]
inline int elapsed_phases(double* const* acc, const Event* ev, int k) {
  for (int i = 0; i < k; ++i)
    if (const int rc = elapsed(*acc[i], ev[i], ev[i + 1]); rc < 0) return rc;
  return 0;
}

// A shard: a device, or a stream of one.  What every subsystem shares; each subsystem keeps its own
// per-shard state in a vector indexed like g_shards and releases it in its *_release_shards().
struct Shard {
  int dev = -1;
  hipStream_t stream = nullptr;
  Event ev0, ev1;
  int cus = 0;                  // compute units of the device (the binned kernel: 4 bins per CU)
  uint32_t resident = 0;        // bm_search_kernel workgroups resident on the device (occupancy x CUs)
  unsigned long long* d_xb = nullptr;  // the cross-shard bound table as this device addresses it
};

inline std::vector<Shard> g_shards;
// Counts the shard sets: bumped whenever g_shards is released (select_devices, shutdown).  A batch, a
// verification batch or a service's session remembers the set its device buffers were made for and is
// refused (BMPOW_E_STATE) under any other -- a re-selection to a set of the same size included.  Under g_mu.
inline uint64_t g_generation = 0;
// The cross-shard bound (bmpow_layout.h): BM_MAX_SHARDS rows of BM_XSLOTS words, host-pinned, coherent
// and mapped into every device; allocated with the shard set.
inline PinBuf<unsigned long long> g_xb;
// Columns a work item may get per shard.  Shards of one device form one device group of the engine
// (bmsched::PlanCtx::group): they never hold one object at once and never split a window among
// themselves, so an item may have all of its device's resident workgroups (g_dev_resident).  Under the
// rehearsal knob (bmpow_set_engine_split: every shard its own group, as separate GPUs) the pieces of a
// split window share a device, and each gets the device's resident workgroups over the shards sharing
// it (g_resident), so every piece's sweep is on the chip at once.
inline uint32_t g_resident = 0, g_dev_resident = 0;
inline bool g_engine_split = false;
// The per-device steppers over the shard set (created with it; bmsched::Engine).
extern std::unique_ptr<bmsched::Engine> g_engine;  // bmpow_host_batch.hip, after the state its steppers use
inline bmpow_stats g_stats{};

// bmpow_host.hip
int init_locked();
int sync_shards();  // every shard's stream, drained
uint32_t hw_queues();
// bmpow_host_batch.hip
void make_engine();
int batch_init_shards();
void drop_scratch(std::unique_lock<std::mutex>& lk);
void service_stop_all();
// bmpow_host_one.hip
struct MaskedStream {
  int dev;
  uint32_t lo, hi;
  hipStream_t stream;
};
extern std::vector<MaskedStream> g_masked;
extern std::vector<std::pair<int, hipStream_t>> g_run_streams;
void free_one();
int search_one(const uint8_t ih[64], uint64_t target, uint64_t start, uint64_t max_trials, uint64_t* nonce_out,
               uint64_t* trial_out, std::unique_lock<FairMutex>& g);
void one_reset_stats();
void one_add_stats(size_t shard, uint64_t* trials, double* kernel_ms);
// bmpow_host_addr.hip: the 16-bit fixed-base comb of the shard's device (table[i << 16 | v] =
// v 2^(16 i) G, affine), built on first use and kept with the shard set -- the address search's
// table, shared with the signature verification
int addr_comb16_table(Shard& sh, const ec::ge** table);
// Each subsystem's per-shard state, released (bmpow_host.hip free_shards: after the shard's stream drained)
void engine_release_shards();
void probe_release_shards();
void verify_release_shards();
void addr_release_shards();
void intake_release_shards();
void packets_release_shards();
void inv_release_shards();
void proc_release_shards();

}  // namespace bmhost
