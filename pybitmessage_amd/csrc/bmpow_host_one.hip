// bmpow_host_one.hip -- run()'s single-object path (search_one), the streams kept for it, and the
// bmpow_set_run_split / bmpow_get_run_pieces entry points.
#include "bmpow_host.h"

namespace bmhost {

// ---------------------------------------------------------------------------------------
// run()'s single-object path (bm_search1_kernel, bm_one_* in bmpow_layout.h).  A serial run() call --
// every call site in the reference (class_singleWorker.py:236,1276, api.py:1304,1350) -- needs the
// lowest latency per object: the object rides in the kernel arguments (no upload), each window is one
// launch per piece with the next window queued behind it when it may be needed (it stops at once on
// the call's hit), and each launch's last workgroup writes its result into host-mapped memory that this
// thread polls (no resolve kernel, no copy, no event, no stepper thread in between).
//
// Pieces (round 5).  On several physical devices each window is cut into one interleaved piece per
// device (columns [g0, g0 + nwg) of the window's gn, as the engine's split windows) and the pieces share
// the call's running minimum through the cross-device bound (a host-pinned table, one slot per call in
// the ring, one row per piece; bm_publish / the kernel's relay).  Shards that share a device never split
// a window: their kernels would compete for the same SIMDs (the engine's split windows over 8 streams
// of one MI355X ran C1 at 3.11 GH/s with 46 % of the hashed nonces past the answer, round 4), so such a
// device gets one piece with all its resident workgroups.  bmpow_set_run_split(1) forces one piece per
// shard (the tests' rehearsal of the multi-device path on one GPU).
// ---------------------------------------------------------------------------------------
struct OnePath {
  int dev = -1;
  DevBuf<bm_one_call> d_calls;
  DevBuf<bm_one_ctr> d_ctr;
  PinBuf<bm_one_out> h_out;  // host-mapped ring of results (h_out.dptr(): the device's address of it)
  unsigned long long* d_xone = nullptr;  // the cross-device table as this device maps it
  hipStream_t stream = nullptr;  // run_stream (or the shard's), or (a forced piece sharing its device) a masked one
  bool masked = false;           // stream is the CU-masked stream of this piece's slice (masked_stream)
  uint32_t cus = 0;              // CUs of that slice (0: the whole device)
  uint32_t slice = 0, slices = 1;  // this piece's slice of its device, of `slices`
  Event ev[8];  // BMPOW_ONE_EVENT: recorded behind launch seq in ev[seq % 8]
  uint64_t seq = 0;
  double rate = 0;  // trials per ms, an exponential average over launches of >= 2^24 trials (0: none yet)
  uint64_t trials = 0;  // since bmpow_reset_stats (bmpow_get_shard_stats)
  double ms = 0;
};
std::vector<OnePath> g_ones;  // per shard; set up for the shards that carry pieces
PinBuf<unsigned long long> g_xone;  // the cross-device bound of split run() calls (BM_MAX_SHARDS x BM_XSLOTS)
uint64_t g_one_call = 0;
bool g_run_split = false;  // bmpow_set_run_split: one piece per shard even where shards share a device
// The wait (g_one_wait): "auto" spins when the call's answer is expected within kOneSpinMs (E over
// the pieces' measured rate), and otherwise sleeps between polls of the result word.  The reference's PoW threads run at SCHED_IDLE
// (bitmsghash.cpp:149) and its pool workers at nice 20 (proofofwork.py:72-87): run() happens on the
// caller's own thread here, so it keeps its priority and instead leaves the CPU alone while the GPU
// works, except for the last few ms of a short call.
constexpr double kOneSpinMs = 20.0;
// A run() beside a busy batch expected to take longer than this (one engine launch is ~80 ms) shares the
// device with the batch instead of going first (search_one_calls)
constexpr double kOneShareMs = 100.0;
// a piece's rate before it has a sample: one MI355X's bm_search1_kernel, measured
constexpr double kOneRateGuess = 6.5e6;

// CU-masked streams, one per (device, CU range), created on first use and kept for the life of the
// process.  On this ROCm (7.2) creating a masked stream after masked streams were destroyed hangs inside
// hipExtStreamCreateWithCUMask -- the second creation after three were destroyed, every time
// (tools/diag/cumask_free.hip, profiles/r05/cumask_free/) -- while creating many and destroying none
// does not.  So the library never destroys one; a forced split reuses its slices' streams, and past
// kMaxMasked distinct ranges a piece runs on its shard's stream unmasked.  (Each holds a hardware queue
// and ~190 MiB of host memory in the runtime: tools/diag/rss_layout.py.)
std::vector<MaskedStream> g_masked;  // (raw: bmpow_atexit destroys them, nothing else ever does)
constexpr size_t kMaxMasked = 24;

// The stream of CUs [lo, hi) of device dev (n CUs), or null once kMaxMasked ranges exist.
int masked_stream(int dev, uint32_t n, uint32_t lo, uint32_t hi, hipStream_t* out) {
  *out = nullptr;
  for (const MaskedStream& m : g_masked)
    if (m.dev == dev && m.lo == lo && m.hi == hi) {
      *out = m.stream;
      return 0;
    }
  if (g_masked.size() >= kMaxMasked) return 0;
  std::vector<uint32_t> mask((n + 31) / 32, 0);
  for (uint32_t cu = lo; cu < hi; ++cu) mask[cu / 32] |= 1u << (cu % 32);
  hipStream_t st = nullptr;
  HIPTRY(hipExtStreamCreateWithCUMask(&st, (uint32_t)mask.size(), mask.data()));
  g_masked.push_back({dev, lo, hi, st});
  BM_TRACE("masked stream %zu: dev %d CUs [%u, %u) stream %p", g_masked.size() - 1, dev, lo, hi, (void*)st);
  *out = st;
  return 0;
}

// run()'s stream on a device: one per device, of the highest priority, kept for the process like the
// masked streams.  On the shard's stream a run() beside a busy batch queued behind the engine's running
// launch and its lookahead (160-240 ms, tools/diag/run_beside_service.py); on its own stream the call's
// workgroups are dispatched as the running launch's retire.  Used only by calls made while the engine
// has work, and created at the first such call: a stream costs the runtime a hardware queue and ~190 MiB
// of host memory (tools/diag/rss_layout.py).  BMPOW_RUN_STREAM=0: always the shard's stream (A/B,
// g_run_stream).
std::vector<std::pair<int, hipStream_t>> g_run_streams;

int run_stream(int dev, hipStream_t* out) {
  for (const auto& r : g_run_streams)
    if (r.first == dev) {
      *out = r.second;
      return 0;
    }
  int least = 0, greatest = 0;
  HIPTRY(hipDeviceGetStreamPriorityRange(&least, &greatest));
  hipStream_t st = nullptr;
  HIPTRY(hipStreamCreateWithPriority(&st, hipStreamNonBlocking, greatest));
  g_run_streams.emplace_back(dev, st);
  BM_TRACE("run stream: dev %d priority %d (range %d..%d) stream %p", dev, greatest, least, greatest, (void*)st);
  *out = st;
  return 0;
}

void free_one() {
  // every stream a piece launched on drains before any buffer is freed (hipFree waits for the device)
  for (size_t s = 0; s < g_ones.size(); ++s) {
    OnePath& op = g_ones[s];
    if (op.dev < 0) continue;
    (void)hipSetDevice(op.dev);
    BM_TRACE("free_one: piece %zu dev %d masked %d: stream %s, shard stream %s", s, op.dev, (int)op.masked,
             op.stream ? hipGetErrorName(hipStreamQuery(op.stream)) : "-",
             s < g_shards.size() && g_shards[s].stream ? hipGetErrorName(hipStreamQuery(g_shards[s].stream)) : "-");
    if (s < g_shards.size() && g_shards[s].stream) (void)hipStreamSynchronize(g_shards[s].stream);
    if (op.stream && (s >= g_shards.size() || op.stream != g_shards[s].stream)) (void)hipStreamSynchronize(op.stream);
  }
  BM_TRACE("free_one: streams drained");
  g_ones.clear();
  g_xone.reset();
  BM_TRACE("free_one: done");
}

int ensure_one(size_t s, uint32_t slice, uint32_t slices) {
  if (g_ones.size() != g_shards.size()) g_ones.resize(g_shards.size());
  OnePath& op = g_ones[s];
  const Shard& sh = g_shards[s];
  if (op.dev == sh.dev && op.d_calls && op.slice == slice && op.slices == slices) return 0;
  HIPTRY(hipSetDevice(sh.dev));
  if (op.stream && op.stream != sh.stream) (void)hipStreamSynchronize(op.stream);  // another slice than before
  op = OnePath();  // releases the piece's previous ring and events
  if (!g_xone) {
    HIPTRY(g_xone.alloc(sh.dev, (size_t)BM_MAX_SHARDS * BM_XSLOTS,
                        hipHostMallocPortable | hipHostMallocMapped | hipHostMallocCoherent));
    for (size_t i = 0; i < g_xone.cap(); ++i) g_xone[i] = ~0ULL;
  }
  op.dev = sh.dev;
  op.slice = slice;
  op.slices = slices;
  op.stream = sh.stream;  // search_one_calls moves it to run_stream while a batch is running
  if (slices > 1 && g_split_cumask && sh.cus > 0) {
    const uint32_t n = (uint32_t)sh.cus, lo = slice * n / slices, hi = (slice + 1) * n / slices;
    hipStream_t st = nullptr;
    const int rc = masked_stream(sh.dev, n, lo, hi, &st);
    if (rc < 0) return rc;
    if (st) {
      op.stream = st;
      op.masked = true;
      op.cus = hi - lo;
    }
    BM_TRACE("ensure_one: piece %zu dev %d slice %u/%u: CUs [%u, %u) stream %p", s, sh.dev, slice, slices, lo, hi,
             (void*)op.stream);
  }
  bm_one_call init[BM_ONE_CALLS];
  std::memset(init, 0, sizeof init);
  for (bm_one_call& c : init) c.best = ~0ULL;
  HIPTRY(op.d_calls.alloc(sh.dev, BM_ONE_CALLS));
  HIPTRY(hipMemcpy(op.d_calls.get(), init, sizeof init, hipMemcpyHostToDevice));
  HIPTRY(op.d_ctr.alloc(sh.dev, BM_ONE_RING));
  HIPTRY(hipMemset(op.d_ctr.get(), 0, BM_ONE_RING * sizeof(bm_one_ctr)));
  HIPTRY(op.h_out.alloc(sh.dev, BM_ONE_RING, hipHostMallocMapped | hipHostMallocCoherent));
  std::memset(op.h_out.get(), 0, BM_ONE_RING * sizeof(bm_one_out));
  void* dp = nullptr;
  HIPTRY(hipHostGetDevicePointer(&dp, g_xone.get(), 0));  // portable: as this piece's device maps it
  op.d_xone = (unsigned long long*)dp;
  if (g_one_event)
    for (Event& e : op.ev) HIPTRY(e.alloc(sh.dev, hipEventDisableTiming));
  return 0;
}

// The shards that carry a run()'s pieces: the first shard of every device (or every shard, forced).
std::vector<size_t> one_pieces() {
  std::vector<size_t> p;
  for (size_t s = 0; s < g_shards.size(); ++s) {
    bool dup = false;
    for (size_t q : p) dup = dup || g_shards[q].dev == g_shards[s].dev;
    if (!dup || g_run_split) p.push_back(s);
  }
  return p;
}

// Wait for launch `seq`'s result word.  spin: poll it with a pause (the answer is due within a few
// ms); else sleep between polls for 1/64 of the time waited so far (20 us .. 250 us) -- a few
// thousand polls per second, each a load of host memory.  The launch's event is queried every few
// polls, so a launch that ended without writing its result (a fault) is caught instead of waited for
// forever.
int wait_one(OnePath& op, uint64_t seq, bool spin, double& spin_ms, double& sleep_ms) {
  bm_one_out* o = &op.h_out[seq % BM_ONE_RING];
  const double t0 = now_ms();
  for (uint32_t k = 1;; ++k) {
    if (__atomic_load_n(&o->seq, __ATOMIC_ACQUIRE) == seq) break;
    if (spin ? k % 1024u == 0 : (g_one_query > 0 && k % (uint32_t)g_one_query == 0)) {
      const hipError_t e = g_one_event ? hipEventQuery(op.ev[seq % 8].get()) : hipStreamQuery(op.stream);
      if (e == hipSuccess) {
        if (__atomic_load_n(&o->seq, __ATOMIC_ACQUIRE) == seq) break;
        return set_err(BMPOW_E_HIP, "single-object launch completed without its result");
      }
      if (e != hipErrorNotReady) return set_err(BMPOW_E_HIP, std::string("single-object launch: ") + hipGetErrorString(e));
    }
    if (spin) {
      // a spinning wait still gives its CPU to any other runnable thread now and then (the reference's
      // PoW threads run at SCHED_IDLE, bitmsghash.cpp:149: they never hold a CPU another thread wants)
      if (g_spin_yield && (k & 63) == 0) sched_yield();
      else __builtin_ia32_pause();
    } else {
      const double waited_us = (now_ms() - t0) * 1e3;
      std::this_thread::sleep_for(std::chrono::microseconds((int64_t)std::min(250.0, std::max(20.0, waited_us / 64))));
    }
  }
  const double ms = now_ms() - t0;
  (spin ? spin_ms : sleep_ms) += ms;
  return 0;
}

// g: the library's lock (g_mu), held by the caller, who also holds g_one_mu for the whole call.  It is
// released while the call waits for a window's pieces, so the batch service's steps go on between
// run()'s windows (round 6: before, a long run() held it to the end and the batch stalled behind it).
int search_one_calls(const uint8_t ih[64], uint64_t target, uint64_t start, uint64_t max_trials, uint64_t* nonce_out,
                     uint64_t* trial_out, std::unique_lock<FairMutex>& g) {
  const std::vector<size_t> pieces = one_pieces();
  const size_t P = pieces.size();
  for (size_t p = 0; p < P; ++p) {
    uint32_t slice = 0, slices = 0;  // this piece's place among the pieces on its device
    for (size_t q = 0; q < P; ++q)
      if (g_shards[pieces[q]].dev == g_shards[pieces[p]].dev) {
        if (q < p) ++slice;
        ++slices;
      }
    const int rc = ensure_one(pieces[p], slice, slices);
    if (rc < 0) return rc;
  }
  const uint64_t end = (max_trials - 1 > kU64Max - start) ? kU64Max : start + max_trials - 1;  // last nonce
  const uint64_t call = ++g_one_call;  // every call launches on every piece (it resets call + 2's state)
  const uint32_t xslot = (uint32_t)(call % BM_ONE_CALLS);
  if (P > 1) {
    // the call's slot of every row starts at "no hit": launches still in flight belong to the previous
    // call (each call waits for its first window on every piece), which uses another slot
    for (size_t r = 0; r < P; ++r) __atomic_store_n(&g_xone[r * BM_XSLOTS + xslot], ~0ULL, __ATOMIC_RELAXED);
    __atomic_thread_fence(__ATOMIC_SEQ_CST);
  }
  // Columns per piece: the device's resident workgroups over the pieces sharing it (at most the
  // hardware queues' worth run at once), less the relay's workgroup of a split call.
  const uint32_t hwq = hw_queues();
  std::vector<uint32_t> cap(P);
  double rate = 0;
  bool shared = false;  // pieces share a device (bmpow_set_run_split)
  for (size_t p = 0; p < P; ++p) {
    const Shard& sh = g_shards[pieces[p]];
    const OnePath& op = g_ones[pieces[p]];
    uint32_t same = 0;
    for (size_t q : pieces) same += g_shards[q].dev == sh.dev;
    // a piece on its own CU slice owns that slice's resident workgroups; pieces sharing a whole device
    // split its resident workgroups over the kernels that run at once
    const bool sliced = op.cus > 0;
    shared = shared || (same > 1 && !sliced);
    const double part = sliced ? (double)op.cus / (double)std::max(1, sh.cus) : 1.0 / std::min(same, hwq);
    uint32_t c = sliced ? (uint32_t)((uint64_t)sh.resident * op.cus / (uint32_t)std::max(1, sh.cus))
                        : sh.resident / std::min(same, hwq);
    if (P > 1 && c > 1) --c;
    cap[p] = std::max<uint32_t>(1, std::min<uint32_t>(c, BM_ONE_MAX_WG));
    rate += (op.rate > 0 ? op.rate : kOneRateGuess * part);
  }
  // Beside a batch with work (the engine's launches on the shard streams): a call expected to end within
  // kOneShareMs (E, or its budget, over the pieces' rate) takes run()'s own stream of the highest priority
  // -- its windows are dispatched first, and the batch waits at most that long --, a longer one the shard's
  // stream, where its windows and the engine's launches queue in turn and share the device launch by
  // launch (with g_mu released between its windows the service keeps the engine fed).  Round 5 gave every
  // call the priority stream and held g_mu throughout: a C4-difficulty run() stalled the batch for its
  // whole call.  Else the shard's stream.  A piece changing streams first lets the old one drain (a queued
  // window of the previous call stops at its first block), so its launches stay in call order.
  const double expect_ms = std::min(18446744073709551616.0 / ((double)target + 1.0), (double)max_trials) / rate;
  bool busy = false;
  if (g_run_stream && g_engine && expect_ms <= kOneShareMs) {
    std::lock_guard<std::mutex> el(g_engine->mu);
    const bmsched::BatchState* b = g_engine->attached();
    busy = g_engine->in_flight() > 0 || (b && b->pending > 0);
  }
  for (size_t p = 0; p < P; ++p) {
    OnePath& op = g_ones[pieces[p]];
    if (op.masked) continue;
    hipStream_t want = g_shards[pieces[p]].stream;
    if (busy) {
      HIPTRY(hipSetDevice(op.dev));
      const int rc = run_stream(op.dev, &want);
      if (rc < 0) return rc;
    }
    if (op.stream != want) {
      HIPTRY(hipStreamSynchronize(op.stream));
      op.stream = want;
    }
  }
  // A window: one step per piece (a piece hashes ~1/P of it; bm_one_ctr.acc's trial field).  Pieces
  // that share a device do not all run at once (its hardware queues run 4 kernels; the rest start as
  // those finish), so a piece may sweep its whole share of a window before the piece holding the answer
  // starts: there a window is 2E (bmsched::expect_cap), as the engine's split windows.
  uint64_t step = std::min<uint64_t>(g_step_trials.load(), BM_ONE_MAX_WINDOW) * P;
  if (shared) step = std::min(step, bmsched::expect_cap(target, P, BM_CHUNK));
  const uint64_t bpw = bmsched::kBlocksPerWorker;
  uint64_t next = start;
  bool top = false;
  // windows in flight, oldest first: their nonces and each piece's sequence number
  struct Fly {
    uint64_t n;
    uint64_t seq[BM_MAX_SHARDS];
  };
  Fly fly[2];
  int nfly = 0;
  // The next window is queued behind the running one only while the windows in flight may well hold
  // no hit (fewer than kAheadE x E nonces, E = 2^64 / (target + 1): P(no hit) > e^-8): a C1 object
  // (E ~ 1.3e7 against a 2^29 window) then costs one launch per piece, and no idle lookahead launch sits
  // in the next call's way; a hard object (C4) or a sweep (C3) keeps two windows in flight.
  constexpr double kAheadE = 8.0;
  const double expect = 18446744073709551616.0 / ((double)target + 1.0);
  auto want_next = [&]() {
    double n = 0;
    for (int i = 0; i < nfly; ++i) n += (double)fly[i].n;
    return !top && nfly < 2 && (nfly == 0 || n < kAheadE * expect);
  };
  // spin only for a call whose answer is due within kOneSpinMs (at most that much CPU per call); a
  // longer call sleeps between polls, so a wake-up may come up to 250 us late -- 0.2 % of a 120 ms call
  const bool short_call = expect / rate < kOneSpinMs;
  bm_one_args a;
  std::memset(&a, 0, sizeof a);
  for (int i = 0; i < 8; ++i) a.w[i] = bmsched::load_be64(ih + 8 * i);
  a.target = target;
  a.xslot = xslot;
  a.xrows = (uint32_t)P;
  uint32_t nwg[BM_MAX_SHARDS];
  auto launch = [&]() -> int {
    const uint64_t room = end - next;  // nonces after next, up to end
    const uint64_t count = room >= step ? step : room + 1;
    const uint64_t nblk = count / BM_BLOCK + (count % BM_BLOCK ? 1 : 0);
    const uint64_t per = (nblk + P - 1) / P;  // blocks of a piece
    uint32_t gn = 0;
    for (size_t p = 0; p < P; ++p) {
      nwg[p] = (uint32_t)std::min<uint64_t>(cap[p], std::max<uint64_t>(1, (per + bpw - 1) / bpw));
      gn += nwg[p];
    }
    Fly& f = fly[nfly];
    f.n = count;
    a.start = next;
    a.count = count;
    a.gn = gn;
    uint32_t g0 = 0;
    for (size_t p = 0; p < P; ++p) {
      const Shard& sh = g_shards[pieces[p]];
      OnePath& op = g_ones[pieces[p]];
      a.call = op.d_calls.get() + call % BM_ONE_CALLS;
      a.reset = op.d_calls.get() + (call + 2) % BM_ONE_CALLS;
      a.nwg = nwg[p];
      a.g0 = g0;
      g0 += nwg[p];
      a.xb = P > 1 ? op.d_xone : nullptr;
      a.xrow = (uint32_t)p;
      a.seq = ++op.seq;
      const uint32_t r = (uint32_t)(a.seq % BM_ONE_RING);
      a.ctr = op.d_ctr.get() + r;
      a.out = op.h_out.dptr() + r;
      f.seq[p] = a.seq;
      if (P > 1) HIPTRY(hipSetDevice(sh.dev));
      HIPTRY(bm_launch_search1(op.stream, a));
      if (g_one_event) HIPTRY(hipEventRecord(op.ev[a.seq % 8].get(), op.stream));
    }
    ++nfly;
    if (room < step) top = true;
    else next += count;
    return 0;
  };
  if (P == 1) HIPTRY(hipSetDevice(g_shards[pieces[0]].dev));
  int rc = launch();
  while (rc == 0 && want_next()) rc = launch();  // the next window, queued behind
  while (rc == 0) {
    // the oldest window: every piece's launch, waited for without the library's lock (only this
    // call's pieces are read meanwhile: g_one_mu keeps every other user of them out)
    bool found = false;
    uint64_t best = 0, best_trial = 0;
    double span = 0, spin_ms = 0, sleep_ms = 0;
    const bool spin = g_one_wait == kOneSpin || (g_one_wait == kOneAuto && short_call);
    g.unlock();
    for (size_t p = 0; p < P && rc == 0; ++p) rc = wait_one(g_ones[pieces[p]], fly[0].seq[p], spin, spin_ms, sleep_ms);
    g.lock();
    g_stats.one_wait_spin_ms += spin_ms;
    g_stats.one_wait_sleep_ms += sleep_ms;
    for (size_t p = 0; p < P && rc == 0; ++p) {
      OnePath& op = g_ones[pieces[p]];
      const uint64_t seq = fly[0].seq[p];
      const bm_one_out& o = op.h_out[seq % BM_ONE_RING];
      const double ms = (double)(o.t1 - o.t0) * 1e-5;  // s_memrealtime: 100 MHz
      g_stats.launches++;
      g_stats.trials += o.trials;
      g_stats.cut_trials += o.cut;
      g_stats.kernel_ms += ms;
      span = std::max(span, ms);
      op.trials += o.trials;
      op.ms += ms;
      if (o.trials >= bmsched::kRateMinTrials && ms > 0)
        op.rate = op.rate > 0 ? (1 - bmsched::kRateAlpha) * op.rate + bmsched::kRateAlpha * (double)o.trials / ms
                              : (double)o.trials / ms;
      // a piece's result is its device's running minimum: its own hit, or one the relay folded in (a
      // real hit of the object too); found is its own.  The least found over the pieces is the answer:
      // every piece hashed all of its blocks that start at or below any hit it saw, so the block holding
      // the least hit of the window was hashed by its piece, which then holds that hit
      if (o.found && (!found || o.nonce < best)) {
        found = true;
        best = o.nonce;
        best_trial = o.trial;
      }
    }
    if (rc < 0) break;
    g_stats.steps++;
    g_stats.max_shard_kernel_ms += span;
    if (found) {  // the lowest hit: every earlier window of the call ended without one
      *nonce_out = best;
      *trial_out = best_trial;
      return BMPOW_FOUND;  // a window still queued stops at its first block (the call's best)
    }
    fly[0] = fly[1];
    --nfly;
    if (g_abort.load()) return set_err(BMPOW_E_ABORTED, "aborted");
    while (rc == 0 && want_next()) rc = launch();
    if (nfly == 0) return BMPOW_NOT_FOUND;
  }
  return rc;
}

int search_one(const uint8_t ih[64], uint64_t target, uint64_t start, uint64_t max_trials, uint64_t* nonce_out,
               uint64_t* trial_out, std::unique_lock<FairMutex>& g) {
  const int rc = search_one_calls(ih, target, start, max_trials, nonce_out, trial_out, g);
  // A call that failed may have launched on only some pieces (or none): the pieces it skipped did not
  // put the state of the call two ahead back to "no hit", which that call would then read.  Start the
  // ring afresh (an abort comes only after every piece's first launch, so it keeps the ring).
  if (rc < 0 && rc != BMPOW_E_ABORTED) free_one();
  return rc;
}

// run()'s pieces in the shard statistics (bmpow_reset_stats, bmpow_get_shard_stats)
void one_reset_stats() {
  for (OnePath& op : g_ones) {
    op.trials = 0;
    op.ms = 0;
  }
}

void one_add_stats(size_t shard, uint64_t* trials, double* kernel_ms) {
  if (shard >= g_ones.size()) return;
  if (trials) *trials += g_ones[shard].trials;
  if (kernel_ms) *kernel_ms += g_ones[shard].ms;
}

}  // namespace bmhost

using namespace bmhost;

extern "C" {

int bmpow_set_run_split(int per_shard) {
  std::lock_guard<std::timed_mutex> one(g_one_mu);
  std::lock_guard<FairMutex> lk(g_mu);
  const int prev = g_run_split ? 1 : 0;
  if (per_shard < 0) return prev;
  if ((per_shard != 0) != g_run_split) {
    // a shard that carries no piece misses the ring resets of the calls it sits out: start afresh
    free_one();
    g_run_split = per_shard != 0;
  }
  return prev;
}

int bmpow_get_run_pieces(int* shards, int cap) {
  std::lock_guard<FairMutex> lk(g_mu);
  const int rc = init_locked();
  if (rc < 0) return rc;
  const std::vector<size_t> p = one_pieces();
  for (int i = 0; i < (int)p.size() && i < cap; ++i)
    if (shards) shards[i] = (int)p[i];
  return (int)p.size();
}

}  // extern "C"
