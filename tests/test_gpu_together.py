"""The entry points together, on the GPU: the way a node uses the library is several subsystems at once, from
several threads, while the PoW engine is busy -- and every crypto entry point, and the network side's (packet
framing, the inventory sets, the object processor's dispatch), queues its copies and kernels on
shard 0's stream, the stream the engine's stepper for shard 0 launches the search kernel on, under the one fair
lock (g_mu) that a service's step holds and hands over when somebody waits.

* beside a live service: a PowService kept busy by two objects that can never finish, a feeder submitting
  objects of 200 / 20,000 / 200,000 expected trials and checking every answer against the C oracle, serial
  run() calls on the reference's first-nonce KATs, and four threads cycling through tests/workloads.py from
  different offsets, every result byte-equal to the idle baseline -- under one shard, four shards, and three
  forced run() pieces;
* bmpow_abort() with four threads inside different subsystems: a call that returns is its baseline or
  E_ABORTED, nothing else; once every thread has seen the flag every call raises; after bmpow_clear_abort() a
  full round is the baseline again; and from one thread, with the flag set first, every workload's run() leaves by
  E_ABORTED, while an inventory set and a dispatcher can still be made;
* every workload under a layout other than the default, and after returning to it (the 16-bit comb table,
  rebuilt with the shard set, is read by the signature, send and outgoing units as well as the address search).

The expectations are the fixtures' own: workloads.baseline() holds each workload's idle result against its
fixture with the per-subsystem tests' checkers, and everything here is equality with those bytes.  The
latencies and rates printed are measurements, not conditions ("The entry points together").
One process, at most 8 Python threads, every join and result with a timeout; on a timeout the test aborts the
library so that blocked calls return, joins again, clears the flag and fails.  Run on an MI355X."""
import random
import statistics
import threading
import time

import pytest

from pybitmessage_amd import _lib, proofofwork, worker
from tests import workloads
from tests.test_gpu_engine import run_split  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
U64 = (1 << 64) - 1
LAYOUTS = (([0], False), ([0, 0, 0, 0], False), ([0, 0, 0], True))
EXPECT = (200, 20000, 200000)  # the feeder's objects: expected trials (target = 2^64 / E)
CRYPTO_THREADS = 4
HANG_S = 60                    # a hang guard, in the order of the f.result(60) used elsewhere; a phase takes seconds
FEED_ALONE = 12                # answers the feeder checks before the crypto threads start: its rate without them


@pytest.fixture(scope='module')
def base(gpulib):
    """The idle baseline: every workload run once, checked against its fixture, its canonical bytes kept."""
    return workloads.baseline()


def trials_hashed(lib):
    st = _lib.BmpowStats()
    assert lib.bmpow_get_stats(st) == 0
    return int(st.trials)


def guard(fn, crashed, stop):
    """A thread's exception is collected and ends the phase (the soak's pattern)."""
    def body(*a):
        try:
            fn(*a)
        except Exception as e:  # noqa: BLE001 -- surfaced by the phase's assertion
            crashed.append('%s: %r' % (fn.__name__, e))
            stop.set()
    return body


def join_all(threads, lib, stop):
    """Join with a timeout; on a timeout abort the library so that blocked calls return, join again, clear the
    flag and fail."""
    stop.set()
    for x in threads:
        x.join(HANG_S)
    stuck = [x.name for x in threads if x.is_alive()]
    if stuck:
        lib.bmpow_abort()
        try:
            for x in threads:
                x.join(HANG_S)
        finally:
            lib.bmpow_clear_abort()
        pytest.fail('threads did not end within %d s: %s' % (HANG_S, stuck))


def median_ms(samples):
    return round(1000 * statistics.median(samples), 2) if samples else None


def alone_latencies(base):
    """Three idle calls of every workload: each equal to the baseline; the median seconds per call."""
    out = {}
    for w in workloads.workloads():
        took = []
        for _ in range(3):
            t0 = time.perf_counter()
            got = w()
            took.append(time.perf_counter() - t0)
            assert got == base[w.name], w.name
        out[w.name] = statistics.median(took)
    return out


# ------------------------------------------------------------------ a. beside a live service
@pytest.mark.parametrize('layout,split', LAYOUTS, ids=['one_shard', 'four_shards', 'three_run_pieces'])
def test_every_entry_point_beside_a_live_service(gpulib, shards, engine_split, run_split, golden, coracle, base,  # noqa: F811
                                                 layout, split):
    engine_split(False)
    shards(layout)
    run_split(split)
    wl = workloads.workloads()
    alone = alone_latencies(base)
    kats = golden('first_nonce_kats.json')['kats']

    stop, feeder_alone = threading.Event(), threading.Event()
    lock = threading.Lock()
    crashed, bad = [], []
    checks = {w.name: [] for w in wl}   # per workload: the thread of each check that passed
    beside = {w.name: [] for w in wl}   # per workload: seconds per call beside the service
    fed = []                            # perf_counter of each feeder answer checked
    serial = [0]

    def covered():
        return all(len(v) >= 3 and len(set(v)) >= 2 for v in checks.values())

    def feeder(svc, rng):
        while not stop.is_set():
            objs = [(U64 // rng.choice(EXPECT), rng.randbytes(64)) for _ in range(4)]
            for (t, ih), f in zip(objs, svc.submit_many(objs)):
                got = f.result(timeout=HANG_S)
                if list(got) != list(coracle.search(ih, t)):
                    bad.append(('feeder', t, ih.hex(), list(got)))
                fed.append(time.perf_counter())
            if len(fed) >= FEED_ALONE:
                feeder_alone.set()

    def serial_runs():
        i = 0
        while not stop.is_set():
            k = kats[i % len(kats)]
            got = proofofwork.run(k['target'], bytes.fromhex(k['ih']))
            if got != [k['trial'], k['nonce']]:
                bad.append(('run', k['note'], got))
            serial[0] += 1
            i += 1

    def crypto(me):
        i = me * len(wl) // CRYPTO_THREADS  # different offsets: different entry points meet
        while not stop.is_set():
            w = wl[i % len(wl)]
            t0 = time.perf_counter()
            got = w()
            took = time.perf_counter() - t0
            if got != base[w.name]:
                bad.append(('crypto', w.name, me))
            with lock:
                checks[w.name].append(me)
                beside[w.name].append(took)
                if covered():
                    stop.set()
            i += 1

    svc = worker.PowService().start()
    threads = []
    trials0 = trials_hashed(gpulib)
    t_start = time.perf_counter()
    try:
        ballast = svc.submit_many([(0, bytes([7]) * 64), (0, bytes([8]) * 64)])  # target 0: they never finish
        rng = random.Random(31 + len(layout))
        threads = [threading.Thread(target=guard(feeder, crashed, stop), args=(svc, rng), name='feeder'),
                   threading.Thread(target=guard(serial_runs, crashed, stop), name='serial')]
        for x in threads:
            x.start()
        # the feeder's rate with no crypto caller (a thread that crashed ends the wait through `stop`)
        while not (feeder_alone.is_set() or stop.is_set()) and time.perf_counter() - t_start < HANG_S:
            feeder_alone.wait(0.05)
        reached = feeder_alone.is_set()
        t_crypto = time.perf_counter()
        if reached and not stop.is_set():
            threads += [threading.Thread(target=guard(crypto, crashed, stop), args=(k,), name='crypto%d' % k)
                        for k in range(CRYPTO_THREADS)]
            for x in threads[2:]:
                x.start()
            reached = stop.wait(HANG_S)
        t_end = time.perf_counter()
        join_all(threads, gpulib, stop)
        advanced = trials_hashed(gpulib) - trials0
    finally:
        stop.set()
        svc.stop(30)
    # the ballast was failed by the stop: the expected outcome
    ballast_failed = [f.exception(timeout=10) is not None for f in ballast]

    n_before = sum(1 for t in fed if t <= t_crypto)
    n_beside = len(fed) - n_before
    print('together layout=%s split=%s: %.1f s; checks per workload %s; feeder %d answers alone (%.0f/s), %d beside the '
          'crypto threads (%.0f/s); serial run() calls %d; trials hashed %d'
          % (layout, split, t_end - t_start, {k: len(v) for k, v in checks.items()}, n_before,
             n_before / max(t_crypto - t_start, 1e-9), n_beside, n_beside / max(t_end - t_crypto, 1e-9), serial[0], advanced),
          flush=True)
    print('together layout=%s median ms per call alone / beside the service: %s'
          % (layout, {w.name: (median_ms([alone[w.name]]), median_ms(beside[w.name])) for w in wl}), flush=True)
    assert not crashed, crashed
    assert not bad, bad[:4]
    assert reached, 'the phase did not reach its end within %d s: %s' % (HANG_S, {k: len(v) for k, v in checks.items()})
    assert covered(), checks
    assert n_beside >= 1, 'the feeder checked no answer while the crypto threads ran'
    assert serial[0] >= 1
    assert advanced > 0, 'the trial counter did not advance: the engine was idle'
    assert all(ballast_failed)


# ------------------------------------------------------------------ b. abort with several subsystems in flight
def test_abort_with_several_subsystems_in_flight(gpulib, base):
    wl = workloads.workloads()
    stop, warm, settled = threading.Event(), threading.Event(), threading.Event()
    lock = threading.Lock()
    crashed, bad = [], []
    done = [0] * CRYPTO_THREADS       # calls finished before the abort, per thread
    observed = set()                  # threads that have seen E_ABORTED
    after = [0] * CRYPTO_THREADS      # calls started once every thread had seen it, per thread
    outcomes = {'baseline': 0, 'aborted': 0}

    def crypto(me):
        i = me * len(wl) // CRYPTO_THREADS
        while not stop.is_set():
            w = wl[i % len(wl)]
            with lock:
                all_saw = len(observed) == CRYPTO_THREADS
            try:
                got = w()
            except _lib.BmpowError as e:
                if e.code != _lib.E_ABORTED:
                    raise
                got = None
            with lock:
                if got is None:
                    observed.add(me)
                    outcomes['aborted'] += 1
                elif got == base[w.name]:
                    outcomes['baseline'] += 1
                    if all_saw:
                        bad.append(('returned under the flag every thread had seen', w.name, me))
                else:
                    bad.append(('neither the baseline nor E_ABORTED', w.name, me))
                if all_saw:
                    after[me] += 1
                done[me] += 1
                if min(done) >= 2:
                    warm.set()
                # every thread starts every workload once more under the flag all have seen
                if min(after) >= len(wl):
                    settled.set()
            i += 1

    threads = [threading.Thread(target=guard(crypto, crashed, stop), args=(k,), name='crypto%d' % k)
               for k in range(CRYPTO_THREADS)]
    try:
        for x in threads:
            x.start()
        warmed = warm.wait(HANG_S) and not stop.is_set()
        before = dict(outcomes)
        gpulib.bmpow_abort()
        ended = warmed and settled.wait(HANG_S)
        join_all(threads, gpulib, stop)
    finally:
        stop.set()
        gpulib.bmpow_clear_abort()
    print('abort: before the flag %s; in all %s; calls started after every thread saw it %s' % (before, outcomes, after),
          flush=True)
    assert not crashed, crashed
    assert not bad, bad[:4]
    assert warmed and ended
    assert before['aborted'] == 0 and before['baseline'] >= 2 * CRYPTO_THREADS
    assert workloads.round_equals_baseline() == []


def test_every_run_under_the_flag_leaves_by_e_aborted(gpulib, base):
    """One thread, the flag set before the call: every workload's run() reaches a device call, whatever its inputs,
    and leaves by E_ABORTED -- those included that first make an inventory set or a dispatcher, which neither
    reads the flag nor fails under it; what was made under the flag works once it is cleared."""
    from pybitmessage_amd import inventory, processor
    key = bytes(range(32))
    gpulib.bmpow_abort()
    try:
        for w in workloads.workloads():
            with pytest.raises(_lib.BmpowError) as err:
                w.run()
            assert err.value.code == _lib.E_ABORTED, w.name
        made = inventory.InventorySet(64, seed=1), processor.Dispatcher(seed=2)
    finally:
        gpulib.bmpow_clear_abort()
    with made[0] as s, made[1] as d:
        assert s.add([key])[0].tolist() == [inventory.ADDED] and key in s
        assert d.watch([key]).all() and d.dispatch([bytes(16) + key], processor.OBJECT_MSG).ack.tolist() == [processor.FOUND]
    assert workloads.round_equals_baseline() == []


# ------------------------------------------------------------------ c. a non-default layout, engine idle
def test_every_workload_in_another_layout_and_back(gpulib, shards, base):
    shards([0, 0, 0, 0])
    assert workloads.round_equals_baseline() == []
    assert gpulib.bmpow_set_devices(None, 0) >= 1  # the default layout: one shard per device
    assert workloads.round_equals_baseline() == []
