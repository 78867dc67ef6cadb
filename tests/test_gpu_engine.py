"""The per-device stepping engine (bmsched::Engine, bmpow_sched.cpp) and run()'s single-object path
(bm_search1_kernel) on the GPU.

* Shards step independently: 8 shards (streams) on this device, one of them throttled (its stepper
  sleeps before every launch, a slow device), solve a C4-like batch exactly while the other seven
  keep the device busy -- their work is not gated by the slow one, as a lockstep step would be
  (VERDICT round 3 "Missing #1").
* The steppers run at SCHED_IDLE, as the reference's PoW threads (src/bitmsghash/bitmsghash.cpp:149),
  and sleep while the GPU works (bmpow_get_thread_info).
* The single-object path: exact at the edges of a bounded call, with the hit log overflowing, and
  one call's queued next window behind another call.
Answers are proven exact with the min-trial probe and, on samples, the C oracle.
"""
import ctypes
import hashlib
import random
import time

import numpy as np
import pytest

import bench
from pybitmessage_amd import _lib, proofofwork
from tests.test_gpu_configs import ROW, ROWS_PAST, assert_exact_first_nonces, oracle_sample

pytestmark = pytest.mark.gpu
U64 = (1 << 64) - 1
SCHED_IDLE = 5
THROTTLE_MS = 400.0


def shard_stats(lib, n):
    tr, ms = (ctypes.c_uint64 * n)(), (ctypes.c_double * n)()
    assert lib.bmpow_get_shard_stats(tr, ms, n) == n
    return [int(x) for x in tr], [float(x) for x in ms]


def c4_like(n, div):
    """bench's C4 objects (1 KB, 20x nonceTrialsPerByte, 28 d) at 1/div of the difficulty: E ~ 1.5e9 / div."""
    objs, _ = bench.make_objects('c4', 0, n)
    return [(t * div, ih) for t, ih in objs]


def test_throttled_shard_does_not_gate_the_others(gpulib, shards, engine_split, coracle):
    """8 shards on this device, each its own device group (bmpow_set_engine_split: as 8 GPUs), with
    2^26-trial launches; shard 0's stepper sleeps THROTTLE_MS before each launch (a slow device).  The
    batch's answers stay exact, and the bounds come from the throttle, not from measured rates:
      * shard 0 plans at most one launch per sleep, each claiming at most one step:
        trials[0] <= (wall / THROTTLE + 1) x 2^26;
      * a lockstep step would hold every shard to that pace, so the other seven together would hash at
        most 7 x that; they hash more (their steppers never wait for shard 0's)."""
    shards([0] * 8)
    engine_split(True)
    step = 1 << 26
    gpulib.bmpow_set_step_trials(step)
    objs = c4_like(64, 8)  # ~1.9e8 trials each, ~1.2e10 in all
    for throttle in (0.0, THROTTLE_MS):
        assert gpulib.bmpow_set_shard_throttle(0, throttle) == 0
        gpulib.bmpow_reset_stats()
        t0 = time.perf_counter()
        res = proofofwork.run_batch(objs)
        wall = time.perf_counter() - t0
        trials, _ = shard_stats(gpulib, 8)
        assert_exact_first_nonces(gpulib, objs, res)
        if throttle:
            cap = (wall / (throttle / 1e3) + 1) * step
            assert trials[0] <= cap, (trials, wall)
            assert sum(trials[1:]) > 7 * cap, (trials, wall)
    assert gpulib.bmpow_set_shard_throttle(0, 0.0) == 0
    oracle_sample(coracle, objs, res, [min(range(len(res)), key=lambda i: res[i][1])])


def test_steppers_idle_priority_and_cpu(gpulib, shards):
    """Every stepper thread runs at SCHED_IDLE and, while a C2-like batch keeps the GPU busy for a
    few seconds, uses a small share of one CPU (it sleeps between queries of its launch's event,
    bmpow_host_batch.hip engine_wait)."""
    shards([0, 0])
    objs, _ = bench.make_objects('c2', 0, 96)
    cpu0 = (ctypes.c_double * 2)()
    pol = (ctypes.c_int * 2)()
    proofofwork.run_batch(objs[:4])  # the steppers exist and have run
    assert gpulib.bmpow_get_thread_info(cpu0, pol, 2) == 2
    assert list(pol) == [SCHED_IDLE, SCHED_IDLE], list(pol)
    t0 = time.perf_counter()
    proofofwork.run_batch(objs)
    wall = time.perf_counter() - t0
    cpu1 = (ctypes.c_double * 2)()
    gpulib.bmpow_get_thread_info(cpu1, pol, 2)
    per_s = [(b - a) / wall for a, b in zip(cpu0, cpu1)]
    assert wall > 0.3
    # bound from the wait's schedule (bmpow_host_batch.hip engine_wait): a stepper sleeps max(20 us, min(1 ms,
    # waited / 32)) between event queries -- ~290 wake-ups over a 160 ms launch (half the device), about
    # 1,800 per second -- and a wake-up (event query, nanosleep, reschedule) costs well under 28 us:
    # 1,800 x 28 us = 0.05 s per second.  Measured 0.0045 (profiles/r04/final/bench.json host_cpu).
    assert all(x < 0.05 for x in per_s), per_s


def test_split_object_over_shards_exact_and_shared_bound(gpulib, shards, engine_split, coracle):
    """Fewer objects than device groups: each window is cut into interleaved pieces, one claimed by each
    group's stepper, the pieces sharing the cross-shard bound; the answers equal the C oracle's for easy
    and harder objects, over 2, 3 and 8 groups (shards of this device, each its own group under
    bmpow_set_engine_split -- the multi-GPU split rehearsed on one GPU)."""
    rng = random.Random(12)
    engine_split(True)
    for layout in ([0, 0], [0, 0, 0], [0] * 8):
        shards(layout)
        objs = [(U64 // rng.choice([3000, 200000, 5000000]), rng.randbytes(64)) for _ in range(len(layout) - 1)]
        res = proofofwork.run_batch(objs)
        for (t, ih), r in zip(objs, res):
            assert tuple(r) == coracle.search(ih, t), (layout, t)
        for t, ih in objs:
            assert proofofwork.run(t, ih) == list(coracle.search(ih, t))


def test_single_object_path_edges(gpulib, coracle):
    """bmpow_search on one shard (bm_search1_kernel): every nonce a hit (the hit log overflows and
    the result's trial is re-hashed), a hit on the last nonce of the call's range and one just past
    it (NOT_FOUND, then found by the next call), and consecutive calls whose previous lookahead
    launch is still queued."""
    n, t = ctypes.c_uint64(), ctypes.c_uint64()
    ih = hashlib.sha512(b'one-path').digest()
    assert gpulib.bmpow_search(ih, U64, 1, 1 << 20, ctypes.byref(n), ctypes.byref(t)) == _lib.FOUND
    assert (n.value, t.value) == (1, coracle.trial(1, ih))
    assert gpulib.bmpow_search(ih, U64 // 2, 77, 1 << 20, ctypes.byref(n), ctypes.byref(t)) == _lib.FOUND
    assert (t.value, n.value) == coracle.search(ih, U64 // 2, 77)
    want_t, want_n = coracle.search(ih, U64 // 40000)
    # the call's last nonce is the answer
    assert gpulib.bmpow_search(ih, U64 // 40000, 1, want_n, ctypes.byref(n), ctypes.byref(t)) == _lib.FOUND
    assert (t.value, n.value) == (want_t, want_n)
    # the answer is one past the call's range: NOT_FOUND, and the next call finds it first
    assert gpulib.bmpow_search(ih, U64 // 40000, 1, want_n - 1, ctypes.byref(n), ctypes.byref(t)) == _lib.NOT_FOUND
    assert gpulib.bmpow_search(ih, U64 // 40000, want_n, 5, ctypes.byref(n), ctypes.byref(t)) == _lib.FOUND
    assert (t.value, n.value) == (want_t, want_n)
    # many short calls back to back; with 2^20-trial windows and E = 2^18 .. 2^19 the next window is
    # queued behind the first (fewer than 8 E nonces in flight), so most calls return with it still
    # queued and the next call's launches run behind it
    rng = random.Random(9)
    gpulib.bmpow_set_step_trials(1 << 20)
    try:
        for i in range(40):
            x = rng.randbytes(64)
            tg = U64 // rng.choice([10, 700, 30000] if i % 2 else [1 << 18, 1 << 19])
            assert proofofwork.run(tg, x) == list(coracle.search(x, tg))
    finally:
        gpulib.bmpow_set_step_trials(0)


def test_single_object_golden_c1(gpulib, golden):
    """The golden C1 object (nonce 10,909,138) through run() on one shard (the single-object path):
    the answer, and the trials hashed within a few block rows of it (one launch: with E ~ 1.3e7 no
    window is queued behind the first 2^29)."""
    k = [k for k in golden('first_nonce_kats.json')['kats'] if k['nonce'] == 10909138][0]
    ih = bytes.fromhex(k['ih'])
    hashed = []
    for _ in range(5):
        gpulib.bmpow_reset_stats()
        assert proofofwork.run(k['target'], ih) == [k['trial'], k['nonce']]
        st = _lib.BmpowStats()
        gpulib.bmpow_get_stats(ctypes.byref(st))
        assert st.trials >= k['nonce'] - 1 and st.launches == 1 and st.kernel_ms > 0, (st.trials, st.launches)
        hashed.append(st.trials)
    # the median call within a few block rows of the answer (a rare call runs on: test_gpu_configs)
    assert sorted(hashed)[2] <= k['nonce'] + 4 * 1024 * 256, hashed


def test_no_empty_launch_stream_behind_a_slow_shard(gpulib, shards, engine_split, coracle):
    """Two shards on this device as two device groups (bmpow_set_engine_split: two GPUs, so shard 1 may
    take over shard 0's objects), shard 0's stepper sleeping 150 ms before each launch, a batch of easy
    objects (E = 2^12 .. 2^16) with 2^20-trial launches: shard 1 finishes its own objects and takes
    over shard 0's, but opens no object's window more than two past the object's oldest open one
    (bmsched::kMaxOpen) -- before that cap it streamed thousands of launches that ended at once on a
    bound its device already held while shard 0's report of the answer was queued.  Answers exact."""
    shards([0, 0])
    engine_split(True)
    gpulib.bmpow_set_step_trials(1 << 20)
    rng = random.Random(31)
    objs = [(U64 >> rng.choice([12, 14, 16]), rng.randbytes(64)) for _ in range(40)]
    assert gpulib.bmpow_set_shard_throttle(0, 150.0) == 0
    try:
        gpulib.bmpow_reset_stats()
        res = proofofwork.run_batch(objs)
        st = _lib.BmpowStats()
        gpulib.bmpow_get_stats(ctypes.byref(st))
    finally:
        gpulib.bmpow_set_shard_throttle(0, 0.0)
    for (t, ih), r in zip(objs, res):
        assert tuple(r) == coracle.search(ih, t), t
    # bound from the window cap: a launch is planned only when it claims a window, an object has at most
    # kMaxOpen = 2 windows past its oldest open one, and a window is 2^20 / q >= 2^20 / 40 nonces (E <=
    # 2^16 ~ 2.5 windows per object's expected answer): ~40 x (2.5 + 2) launches' worth of claims, under
    # 200; without the cap shard 1 streamed thousands of empty launches
    assert st.launches < 200, st.launches


@pytest.fixture
def run_split(gpulib):
    """bmpow_set_run_split for the test body, restored after."""
    prev = gpulib.bmpow_set_run_split(-1)
    yield lambda on: gpulib.bmpow_set_run_split(1 if on else 0)
    gpulib.bmpow_set_run_split(prev)


def run_pieces(lib):
    ids = (ctypes.c_int * 64)()
    n = lib.bmpow_get_run_pieces(ids, 64)
    return list(ids[:n])


def test_run_split_over_pieces_exact(gpulib, shards, run_split, golden, coracle):
    """run() split into 2, 3 and 8 interleaved pieces (bmpow_set_run_split: one piece per shard, here
    shards of this device, each piece on its own CU slice -- the multi-device path of round 5 rehearsed
    on one GPU: every piece a bm_search1_kernel<true> launch with its relay, the cross-device bound in
    host-pinned memory).  The golden C1 object (10,909,138), the test_openclpow vector (224,121,278), random
    objects against the C oracle, and bounded calls whose answer is the last nonce of the range or
    one past it."""
    kats = golden('first_nonce_kats.json')['kats']
    c1 = [k for k in kats if k['nonce'] == 10909138][0]
    ocl = [k for k in kats if k['nonce'] == 224121278][0]
    rng = random.Random(77)
    n, t = ctypes.c_uint64(), ctypes.c_uint64()
    run_split(True)
    for layout in ([0, 0], [0, 0, 0], [0] * 8):
        shards(layout)
        assert run_pieces(gpulib) == list(range(len(layout)))
        for k in (c1, ocl):
            assert proofofwork.run(k['target'], bytes.fromhex(k['ih'])) == [k['trial'], k['nonce']], (layout, k['note'])
        for k in kats[:12]:
            assert proofofwork.run(k['target'], bytes.fromhex(k['ih'])) == [k['trial'], k['nonce']], layout
        for _ in range(6):
            x = rng.randbytes(64)
            tg = U64 // rng.choice([10, 3000, 200000, 5000000])
            assert proofofwork.run(tg, x) == list(coracle.search(x, tg)), layout
        # bounded calls: the answer is the last nonce of the range, then one past it
        ih = hashlib.sha512(b'split-edge %d' % len(layout)).digest()
        want_t, want_n = coracle.search(ih, U64 // 40000)
        assert gpulib.bmpow_search(ih, U64 // 40000, 1, want_n, ctypes.byref(n), ctypes.byref(t)) == _lib.FOUND
        assert (t.value, n.value) == (want_t, want_n)
        assert gpulib.bmpow_search(ih, U64 // 40000, 1, want_n - 1, ctypes.byref(n), ctypes.byref(t)) == _lib.NOT_FOUND
        assert gpulib.bmpow_search(ih, U64 // 40000, want_n, 5, ctypes.byref(n), ctypes.byref(t)) == _lib.FOUND
        assert (t.value, n.value) == (want_t, want_n)
        # every nonce a hit: the pieces' hit logs overflow and the trial is re-hashed on the device
        assert gpulib.bmpow_search(ih, U64, 1, 1 << 20, ctypes.byref(n), ctypes.byref(t)) == _lib.FOUND
        assert (n.value, t.value) == (1, coracle.trial(1, ih))
        # the reference's own C export (bitmsghash.cpp:127), unchanged signature, and the openclpow
        # surface (do_opencl_pow, openclpow.py:77-111) through the pieces
        assert gpulib.BitmessagePOW(bytes.fromhex(c1['ih']), c1['target']) == c1['nonce']
        from pybitmessage_amd import hippow
        hippow.initCL()
        assert hippow.do_opencl_pow(ocl['ih'], ocl['target']) == ocl['nonce']


def test_run_split_small_windows_and_sweep(gpulib, shards, run_split, coracle):
    """Split run() with 2^20-trial windows per piece (several windows per call, the next queued behind
    the running one on every piece) over 3 pieces: answers against the C oracle; and a no-hit sweep
    (target 0) of 2^28 nonces that hashes exactly 2^28 trials in all (no block lost or hashed twice
    over the pieces' interleaved columns)."""
    shards([0, 0, 0])
    run_split(True)
    gpulib.bmpow_set_step_trials(1 << 20)
    rng = random.Random(5)
    for i in range(12):
        x = rng.randbytes(64)
        tg = U64 // rng.choice([1 << 18, 1 << 20, 1 << 21])
        assert proofofwork.run(tg, x) == list(coracle.search(x, tg)), i
    gpulib.bmpow_reset_stats()
    n, t = ctypes.c_uint64(), ctypes.c_uint64()
    ih = hashlib.sha512(b'split sweep').digest()
    assert gpulib.bmpow_search(ih, 0, 1, 1 << 28, ctypes.byref(n), ctypes.byref(t)) == _lib.NOT_FOUND
    st = _lib.BmpowStats()
    gpulib.bmpow_get_stats(ctypes.byref(st))
    assert st.trials == 1 << 28, st.trials
    tr, _ = shard_stats(gpulib, 3)
    assert sum(tr) == 1 << 28 and min(tr) > 0, tr


def test_shards_sharing_a_device_do_not_split_run(gpulib, shards, golden):
    """Without the forced split, shards that share a device give run() ONE piece (their kernels would
    compete for the same SIMDs): 8 shards of this device run the golden C1 object as one shard does --
    one launch, within a few block rows of the answer."""
    shards([0] * 8)
    assert run_pieces(gpulib) == [0]
    k = [k for k in golden('first_nonce_kats.json')['kats'] if k['nonce'] == 10909138][0]
    past = []
    for _ in range(5):
        gpulib.bmpow_reset_stats()
        assert proofofwork.run(k['target'], bytes.fromhex(k['ih'])) == [k['trial'], k['nonce']]
        st = _lib.BmpowStats()
        gpulib.bmpow_get_stats(ctypes.byref(st))
        assert st.launches == 1
        past.append(st.trials - k['nonce'])
    assert max(past) <= ROWS_PAST * ROW, past


def test_long_run_leaves_the_cpu_alone(gpulib, shards):
    """A run() call of over a second sleeps while the GPU works (the reference's PoW threads run at
    SCHED_IDLE, bitmsghash.cpp:149, its pool workers at nice 20, proofofwork.py:72-87; round 4's
    single-object path busy-polled a core for the whole call): process CPU under 0.1 s per second,
    for a no-hit sweep of 2^33 nonces and for a series of objects of E = 2^30 (~165 ms each)."""
    import resource
    shards([0])
    n, t = ctypes.c_uint64(), ctypes.c_uint64()
    ih = hashlib.sha512(b'cpu sweep').digest()

    def cpu():
        ru = resource.getrusage(resource.RUSAGE_SELF)
        return ru.ru_utime + ru.ru_stime
    assert gpulib.bmpow_search(ih, 0, 1, 1 << 26, ctypes.byref(n), ctypes.byref(t)) == _lib.NOT_FOUND  # warm
    gpulib.bmpow_reset_stats()
    c0, w0 = cpu(), time.perf_counter()
    assert gpulib.bmpow_search(ih, 0, 1, 1 << 33, ctypes.byref(n), ctypes.byref(t)) == _lib.NOT_FOUND
    wall, used = time.perf_counter() - w0, cpu() - c0
    st = _lib.BmpowStats()
    gpulib.bmpow_get_stats(ctypes.byref(st))
    # bound from the sleeping wait (bmpow_host_one.hip wait_one): it sleeps min(250 us, max(20 us, waited /
    # 64)) between polls of the result word -- past the first 16 ms of a window, 4,000 polls per second,
    # each a load of host memory and a nanosleep (with an event query every g_one_query polls), well under
    # 25 us: 4,000 x 25 us = 0.1 s per second.  Measured 0.007 (profiles/r05/final/c3.json host_cpu).
    assert wall > 1.0 and used / wall < 0.1, (wall, used)
    # a call expected to take > 20 ms (kOneSpinMs) never spins, and its host work outside the wait -- two
    # launches per window of 2^29 -- is microseconds per 80 ms window: the sleeping wait is the call
    assert st.one_wait_sleep_ms > 0.9 * wall * 1e3 and st.one_wait_spin_ms == 0, (st.one_wait_sleep_ms, st.one_wait_spin_ms)
    rng = random.Random(8)
    objs = [(U64 >> 30, rng.randbytes(64)) for _ in range(10)]
    c0, w0 = cpu(), time.perf_counter()
    for tg, x in objs:
        proofofwork.run(tg, x)  # re-checked with hashlib inside
    wall, used = time.perf_counter() - w0, cpu() - c0
    assert wall > 1.0 and used / wall < 0.1, (wall, used)  # the same bound: each call sleeps (E / rate > 20 ms)


def test_run_split_top_of_space_and_abort(gpulib, shards, run_split, coracle):
    """Split run() (3 forced pieces) at the top of the nonce space -- windows clipped at 2^64 - 1, the
    last nonce itself a hit, NOT_FOUND at the end -- and an abort from another thread during a long
    split sweep: the call returns E_ABORTED within a window, and the next calls (whose launches queue
    behind the aborted call's) are exact."""
    import threading
    shards([0, 0, 0])
    run_split(True)
    n, t = ctypes.c_uint64(), ctypes.c_uint64()
    ih = hashlib.sha512(b'split top').digest()
    top = U64 - 5000
    # every nonce a hit: the first one is the answer
    assert gpulib.bmpow_search(ih, U64, top, 1 << 20, ctypes.byref(n), ctypes.byref(t)) == _lib.FOUND
    assert n.value == top and t.value == coracle.trial(top, ih)
    # the first hit near the top, against the C oracle's scan of the same range
    tg = U64 // 700
    want = coracle.search(ih, tg, top)
    rc = gpulib.bmpow_search(ih, tg, top, 1 << 20, ctypes.byref(n), ctypes.byref(t))
    if want is None:
        assert rc == _lib.NOT_FOUND
    else:
        assert rc == _lib.FOUND and (t.value, n.value) == tuple(want)
    # no hit up to 2^64 - 1 (target 0): NOT_FOUND, every nonce of the clipped range hashed once
    gpulib.bmpow_reset_stats()
    assert gpulib.bmpow_search(ih, 0, top, 1 << 20, ctypes.byref(n), ctypes.byref(t)) == _lib.NOT_FOUND
    st = _lib.BmpowStats()
    gpulib.bmpow_get_stats(ctypes.byref(st))
    assert st.trials == U64 - top + 1, st.trials
    # abort a long split sweep from another thread
    gpulib.bmpow_set_step_trials(1 << 26)
    timer = threading.Timer(0.3, gpulib.bmpow_abort)
    timer.start()
    t0 = time.perf_counter()
    rc = gpulib.bmpow_search(ih, 0, 1, 1 << 40, ctypes.byref(n), ctypes.byref(t))
    took = time.perf_counter() - t0
    timer.join()
    gpulib.bmpow_clear_abort()
    # bound: the abort is seen after the current window (search_one_calls checks g_abort per window);
    # a window is 3 pieces of 2^26 trials on a third of the device each (~30 ms), with one more queued
    # behind it: the timer's 0.3 s + two windows, under 0.4 s -- 2 s leaves 5x for a slow box
    assert rc == _lib.E_ABORTED and took < 2.0, (rc, took)
    rng = random.Random(3)
    for _ in range(4):
        x = rng.randbytes(64)
        tg = U64 // rng.choice([5000, 300000])
        assert proofofwork.run(tg, x) == list(coracle.search(x, tg))


def test_run_split_every_first_nonce_kat_and_fuzz(gpulib, shards, run_split, golden, coracle):
    """Every first-nonce KAT of the reference (tests/golden/first_nonce_kats.json: _doSafePoW answers,
    the C1 object and the test_openclpow vector among them) through run() split into 5 forced pieces,
    then a seeded fuzz of objects, targets, start nonces and call budgets over 2 to 7 pieces against the C
    oracle's sequential search (bounded calls resumed where the previous one stopped, as _doCPoW's
    caller would)."""
    run_split(True)
    shards([0] * 5)
    for k in golden('first_nonce_kats.json')['kats']:
        assert proofofwork.run(k['target'], bytes.fromhex(k['ih'])) == [k['trial'], k['nonce']], k['note']
    rng = random.Random(2026)
    n, t = ctypes.c_uint64(), ctypes.c_uint64()
    for case in range(24):
        shards([0] * rng.randint(2, 7))
        ih = rng.randbytes(64)
        e = rng.choice([2, 50, 900, 20000, 400000])
        tg = U64 // e
        start = rng.choice([1, 2, 1000, 1 << 32, U64 - 100000])
        want = coracle.search(ih, tg, start)
        # call budgets from one nonce up, at least E / 64 so a search takes at most a few hundred calls
        budget = max(rng.choice([1, 300, 5000, 1 << 16, 1 << 22]), e // 64)
        at, got = start, None
        for _ in range(4096):
            rc = gpulib.bmpow_search(ih, tg, at, budget, ctypes.byref(n), ctypes.byref(t))
            assert rc in (_lib.FOUND, _lib.NOT_FOUND), (case, rc)
            if rc == _lib.FOUND:
                got = (t.value, n.value)
                break
            if at > U64 - budget:
                break
            at += budget
        assert got == want, (case, start, budget, got, want)


def test_serial_runs_beside_a_running_service(gpulib, shards, run_split, coracle):
    """The worker thread's batches and the API thread's serial run() calls at once (class_singleWorker.py
    :236, api.py:1304): a PowService solving 48 objects on the engine while two threads make run() calls
    -- single-object launches queued on the same shard streams as the engine's, with one and with 3
    forced pieces.  Every answer exact."""
    import threading
    from pybitmessage_amd import worker
    rng = random.Random(404)
    for layout, split in (([0, 0], False), ([0, 0, 0], True)):
        shards(layout)
        run_split(split)
        batch = [(U64 // rng.choice([3000, 70000, 900000]), rng.randbytes(64)) for _ in range(48)]
        serial = [[(U64 // rng.choice([50, 5000, 200000]), rng.randbytes(64)) for _ in range(8)] for _ in range(2)]
        got = [None, None]

        def caller(k):
            got[k] = [proofofwork.run(t, ih) for t, ih in serial[k]]
        svc = worker.PowService().start()
        try:
            futs = svc.submit_many(batch)
            th = [threading.Thread(target=caller, args=(k,)) for k in range(2)]
            for x in th:
                x.start()
            res = [f.result(timeout=120) for f in futs]
            for x in th:
                x.join(120)
        finally:
            svc.stop(30)
        assert [list(r) for r in res] == [list(r) for r in coracle.search_many(batch)], layout
        for k in range(2):
            assert got[k] == [list(r) for r in coracle.search_many(serial[k])], (layout, k)


def test_run_is_not_starved_by_a_busy_service(gpulib, shards, coracle):
    """A serial run() while a PowService works through a batch of hard objects (PyBitmessage's API
    thread, api.py:1304, beside its worker's batches): the library's lock is handed out first come first
    served and a service step ends at its next completed launch when a caller waits, and run() has its
    own stream of the highest priority -- so a call waits about one engine launch (~80 ms), not for the
    batch (up to 36 s with a plain mutex: tools/diag/run_beside_service.py).  Answers exact."""
    from pybitmessage_amd import worker
    shards([0])
    rng = random.Random(505)
    batch = [(U64 // 2_000_000_000, rng.randbytes(64)) for _ in range(64)]  # ~0.3 s each: ~20 s of work
    calls = [(U64 // 300_000, rng.randbytes(64)) for _ in range(6)]
    svc = worker.PowService().start()
    try:
        svc.submit_many(batch)
        time.sleep(0.5)
        took, got = [], []
        for t, ih in calls:
            t0 = time.perf_counter()
            got.append(proofofwork.run(t, ih))
            took.append(time.perf_counter() - t0)
    finally:
        svc.stop(60)
    assert got == [list(coracle.search(ih, t)) for t, ih in calls]
    # bound: a waiting caller ends the service's step at its next completed launch (g_mu.waiting()) and
    # takes the fair lock next; run() then launches on its own high-priority stream, whose workgroups are
    # dispatched as the engine's running launch retires: at most two engine launches of 2^29 trials
    # (~2 x 81 ms at 6.6 GH/s) plus the call's own hashing (E = 300,000: 0.05 ms) -- 1 s is 6x that
    assert max(took) < 1.0, took


def test_long_run_and_the_service_share_the_gpu(gpulib, shards):
    """C4-difficulty serial run() calls (api.py:1304,1350) beside a PowService busy with a batch
    (class_singleWorker.py:1276): a run() expected to take longer than one engine launch releases the
    library's lock while it waits for its windows and queues them on the shard's stream between the
    engine's launches (round 6), so both make progress.

    Bound from the round-5 design, where run() held the lock for its whole call: the service could
    finish only what was already claimed when the calls took the lock -- the step in progress and its
    lookahead, at most 3 launches of 2^29 trials -- about 3 x 2^29 / E = 24 of these objects, and
    hand none of them out until the calls ended.  The service finishes more than 3x that while the
    calls run.  Every answer (the calls' and the batch's) is proven minimal by the min-trial probe."""
    from pybitmessage_amd import worker
    shards([0])
    rng = random.Random(707)
    e = 1 << 26
    batch = [(U64 // e, rng.randbytes(64)) for _ in range(800)]  # ~8 s of work alone
    calls, _ = bench.make_objects('c4', 0, 6)  # E ~ 1.5e9: ~0.23 s each alone
    reach = 3 * (1 << 29) // e
    svc = worker.PowService().start()
    try:
        futs = svc.submit_many(batch)
        time.sleep(0.5)
        done0 = sum(f.done() for f in futs)
        t0 = time.perf_counter()
        got = [proofofwork.run(t, ih) for t, ih in calls]
        took = time.perf_counter() - t0
        during = sum(f.done() for f in futs) - done0
        res = [f.result(timeout=300) for f in futs]
    finally:
        svc.stop(60)
    assert during > 3 * reach, (during, reach, took)
    assert_exact_first_nonces(gpulib, calls, got)
    assert_exact_first_nonces(gpulib, batch, [list(r) for r in res])


_KEPT_STREAMS_CHILD = r'''
import ctypes, json, os, random, sys
sys.path.insert(0, os.environ["BMPOW_ROOT"])
from pybitmessage_amd import _lib, proofofwork, worker
lib = _lib.get()
U64 = (1 << 64) - 1
rng = random.Random(11)
def kept():
    st = _lib.BmpowStats()
    lib.bmpow_get_stats(ctypes.byref(st))
    return [int(st.masked_streams), int(st.run_streams)]
def layout(ids):
    assert lib.bmpow_set_devices((ctypes.c_int * len(ids))(*ids), len(ids)) == len(ids)
out = {}
# the default paths: run() on one shard and on 8 shards of the device, a batch over 8 shards, a service
# with a run() beside it
for ids in ([0], [0] * 8):
    layout(ids)
    for _ in range(3):
        t, ih = U64 // 300000, rng.randbytes(64)
        proofofwork.run(t, ih)
    proofofwork.run_batch([(U64 // 200000, rng.randbytes(64)) for _ in range(12)])
svc = worker.PowService().start()
futs = svc.submit_many([(U64 // 2000000000, rng.randbytes(64)) for _ in range(8)])
proofofwork.run(U64 // 300000, rng.randbytes(64))
[f.result(timeout=60) for f in futs]
svc.stop(30)
out["default"] = kept()
# the rehearsal knob: forced pieces on CU slices of the device
lib.bmpow_set_run_split(1)
layout([0, 0, 0])
proofofwork.run(U64 // 300000, rng.randbytes(64))
out["forced"] = kept()
print(json.dumps(out), flush=True)
# exit with masked streams, a run() stream and a live service: the exit hook releases them before the
# HIP runtime's exit handlers (round 5: a traced process in this state segfaulted in them)
svc2 = worker.PowService().start()
svc2.submit_many([(U64 // 2000000000, rng.randbytes(64)) for _ in range(4)])
'''


def test_kept_streams_only_under_the_knob_and_a_clean_exit(gpulib):
    """The streams the library keeps for the process (CU-masked streams cost a hardware queue and ~190
    MiB of host memory each) are created only by the rehearsal knob: a process that runs run() on one
    and on eight shards of the device, a batch over eight shards and a service with a run() beside it
    holds no masked stream (a run() stream at most); after a forced 3-piece split it holds three.  The
    process then exits -- masked streams, a run() stream and a busy service alive -- with status 0:
    bmpow_atexit releases them before the HIP runtime's exit handlers."""
    import json
    import os
    import subprocess
    import sys
    env = dict(os.environ, BMPOW_ROOT=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    r = subprocess.run([sys.executable, '-c', _KEPT_STREAMS_CHILD], capture_output=True, text=True, timeout=180,
                       env=env)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out['default'][0] == 0 and out['default'][1] <= 1, out
    assert out['forced'][0] == 3, out
