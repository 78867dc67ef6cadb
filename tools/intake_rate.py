#!/usr/bin/env python3
"""Rate of the batched object intake (bmpow_intake_batch) beside the verification of the same flood
and beside hashlib.

    python tools/intake_rate.py --objects 500000 --out profiles/intake/rate_n500000.json

The flood is bench.py's verify leg's size mix (half acks of 54 B, a quarter pubkey-size objects of 208 B,
a quarter msgs of 0.5 - 16 KB), seeded, with headers that decode (type 2, version 1, stream 1), so every
object is uploaded.  In one process, after a warm-up call of each:

* ``intake.check_objects`` from host buffers: wall time per call, the library's own split of it
  (``bmpow_intake_get_stats``: host build / run / status ms) and the intake kernel's event time;
* ``verify.isProofOfWorkSufficient_batch`` on the same list: wall time per call, its split and the
  verification kernel's event time;
* the compressions either kernel runs over the flood (nblk + nblk2 + 3 against nblk + 2 per object), so
  the kernels' time ratio can be read against the work ratio.

CPU leg: hashlib doing both hashes of every object (the inventory hash and the PoW's three SHA-512s) in
as many processes as the CPU quota allows (16 at most), each for --cpu-seconds.

Prints one JSON line (and writes it to --out).  Without a device the GPU leg raises (there is no
fallback); --cpu-only runs the CPU leg alone."""
import argparse
import ctypes
import hashlib
import json
import multiprocessing
import os
import random
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SEED = 20250216
NOW = 1700000000


def flood(n, seed=SEED + 1000):
    rng = random.Random(seed)
    head = (NOW + 345600).to_bytes(8, 'big') + (2).to_bytes(4, 'big') + b'\x01\x01'
    objs = []
    for i in range(n):
        r = i % 4
        L = 54 if r in (0, 1) else (208 if r == 2 else rng.randrange(520, 16393))
        objs.append(rng.randbytes(8) + head + rng.randbytes(L - 22))
    return objs


def compressions(objs):
    """(intake, verification) SHA-512 compressions over the flood."""
    a = b = 0
    for o in objs:
        nblk = (len(o) - 8 + 17 + 127) // 128
        nblk2 = (len(o) + 17 + 127) // 128
        a += nblk + nblk2 + 3
        b += nblk + 2
    return a, b


def gpu_leg(objs, reps):
    from pybitmessage_amd import _lib, intake, verify
    lib = _lib.get()
    n = len(objs)
    res = intake.check_objects(objs, now=NOW)  # warm-up: buffers, and a spot check against hashlib
    for i in range(0, n, max(1, n // 500)):
        assert res.inventory_hash(i) == hashlib.sha512(hashlib.sha512(objs[i]).digest()).digest()[:32], i
    ok = verify.isProofOfWorkSufficient_batch(objs, recvTime=NOW)
    assert (res.status == intake.OK).tolist() == [bool(v) for v in ok]

    def best(rows):
        return min(rows, key=lambda r: r['wall_ms'])
    irows, vrows = [], []
    for _ in range(reps):
        intake.reset_stats()
        t0 = time.perf_counter()
        intake.check_objects(objs, now=NOW)
        wall = (time.perf_counter() - t0) * 1e3
        st = intake.stats()
        irows.append({'wall_ms': round(wall, 2), 'kernel_ms': round(st['kernel_ms'], 3),
                      'host_build_ms': round(st['host_build_ms'], 2), 'host_run_ms': round(st['host_run_ms'], 2),
                      'host_status_ms': round(st['host_status_ms'], 2),
                      'marshal_ms': round(wall - st['host_build_ms'] - st['host_run_ms'] - st['host_status_ms'], 2)})
        lib.bmpow_reset_stats()
        t0 = time.perf_counter()
        verify.isProofOfWorkSufficient_batch(objs, recvTime=NOW)
        wall = (time.perf_counter() - t0) * 1e3
        s2 = _lib.BmpowStats()
        lib.bmpow_get_stats(ctypes.byref(s2))
        vrows.append({'wall_ms': round(wall, 2), 'kernel_ms': round(s2.verify_kernel_ms, 3),
                      'host_build_ms': round(s2.verify_host_build_ms, 2), 'host_run_ms': round(s2.verify_host_run_ms, 2),
                      'host_verdict_ms': round(s2.verify_host_verdict_ms, 2),
                      'marshal_ms': round(wall - s2.verify_host_build_ms - s2.verify_host_run_ms
                                          - s2.verify_host_verdict_ms, 2),
                      'fast_marshalling': verify._fast() is not None})
    bi, bv = best(irows), best(vrows)
    ci, cv = compressions(objs)
    ik = min(r['kernel_ms'] for r in irows)
    vk = min(r['kernel_ms'] for r in vrows)
    return {'library': lib.bmpow_version().decode(), 'reps': reps,
            'intake': dict(bi, kernel_ms_min=ik, kernel_objects_per_s=n / (ik / 1e3), call_objects_per_s=n / (bi['wall_ms'] / 1e3)),
            'verify': dict(bv, kernel_ms_min=vk, kernel_objects_per_s=n / (vk / 1e3), call_objects_per_s=n / (bv['wall_ms'] / 1e3)),
            'compressions': {'intake': ci, 'verify': cv, 'ratio': ci / cv},
            'kernel_time_ratio': ik / vk, 'call_time_ratio': bi['wall_ms'] / bv['wall_ms'],
            'accepted': int((res.status == intake.OK).sum())}


def _cpu_worker(args):
    objs, seconds = args
    done = 0
    sha = hashlib.sha512
    end = time.perf_counter() + seconds
    while time.perf_counter() < end:
        for o in objs:
            sha(sha(o).digest()).digest()                          # calculateInventoryHash
            sha(sha(o[:8] + sha(o[8:]).digest()).digest()).digest()  # isProofOfWorkSufficient's POW
            done += 1
    return done, time.perf_counter() - (end - seconds)


def cpu_leg(objs, seconds):
    procs = max(1, min(16, len(os.sched_getaffinity(0)), int(os.environ.get('OMP_NUM_THREADS', '16'))))
    sample = objs[:4096]
    with multiprocessing.get_context('spawn').Pool(procs) as pool:
        res = pool.map(_cpu_worker, [(sample, seconds)] * procs)
    rate = sum(d / s for d, s in res)
    return {'processes': procs, 'seconds': seconds, 'objects': sum(d for d, _ in res), 'objects_per_s': rate,
            'what': 'hashlib: inventory hash + POW value per object, the first 4096 objects of the flood in turn'}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--objects', type=int, default=500000)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--cpu-seconds', type=float, default=3.0)
    ap.add_argument('--no-cpu', action='store_true')
    ap.add_argument('--cpu-only', action='store_true')
    ap.add_argument('--out', help='also write the JSON line to this file')
    a = ap.parse_args()
    objs = flood(a.objects)
    out = {'objects': a.objects, 'bytes': sum(map(len, objs))}
    if not a.no_cpu:  # first: its worker processes start before this one opens the device
        out['cpu'] = cpu_leg(objs, a.cpu_seconds)
    if not a.cpu_only:
        out['gpu'] = gpu_leg(objs, a.reps)
    if 'gpu' in out and 'cpu' in out:
        out['speedup_call'] = out['gpu']['intake']['call_objects_per_s'] / out['cpu']['objects_per_s']
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
