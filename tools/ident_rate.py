#!/usr/bin/env python3
"""Rate of the batched sender identification (bmpow_ident_derive) beside the same work on the CPU.

    python tools/ident_rate.py --rows 500000

GPU leg: N rows (two public keys, an address version, a stream) through ``addresses.derive_batch``'s C call,
from host buffers to host records, after a warm-up call of the same shape.  The kernel time comes from the
library's own device events around the launches (``bmpow_ident_get_stats``); the call's wall time (upload of
144 bytes per row, the launches, download of 180 bytes per row) is reported beside it as the end-to-end
figure.  The N rows cycle through 4,096 distinct ones; the records are cleared before every timed call and a
sample of the last call's is compared with the CPU leg's code.

CPU leg: the reference's statements per object -- SHA-512 of the two keys, RIPEMD-160 (``src/
class_objectProcessor.py:877-879``), the double SHA-512 of the tag (``:889-892``) and ``encodeAddress``
(``src/addresses.py:146-180``) -- with hashlib's SHA-512 and libcrypto's RIPEMD-160 through the oracle's
binding, in as many processes as the CPU quota allows (16 at most), each for --cpu-seconds.

Prints one JSON line and writes it to --out (default profiles/ident/rate_n<N>.json).  Without a device the
GPU leg raises (there is no fallback); --cpu-only runs the CPU leg alone."""
import argparse
import hashlib
import json
import multiprocessing
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DISTINCT = 4096


def make_inputs(n, seed=20251020):
    """(keys (n, 128) uint8, versions, streams): the keys are random bytes (the hashes read nothing else)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    m = min(n, DISTINCT)
    keys = rng.integers(0, 256, size=(m, 128), dtype=np.uint8)
    versions = np.array([(4, 3, 2, 4)[i % 4] for i in range(m)], dtype=np.uint64)
    streams = np.array([(1, 1, 2, 300, 70000)[i % 5] for i in range(m)], dtype=np.uint64)
    rep = np.arange(n) % m
    return np.ascontiguousarray(keys[rep]), np.ascontiguousarray(versions[rep]), np.ascontiguousarray(streams[rep])


def cpu_row(ripemd160, key128, version, stream):
    """What the reference computes per object: (ripe, tag, address)."""
    from pybitmessage_amd.addressgen import encodeAddress, encodeVarint
    ripe = ripemd160(hashlib.sha512(b'\x04' + key128[:64] + b'\x04' + key128[64:]).digest())
    data = encodeVarint(version) + encodeVarint(stream) + ripe
    tag = hashlib.sha512(hashlib.sha512(data).digest()).digest()[32:]
    return ripe, tag, encodeAddress(version, stream, ripe)


def gpu_leg(keys, versions, streams, reps):
    import ctypes

    import numpy as np
    from oracle.addrgen_oracle import OpenSSLRipemd160
    from pybitmessage_amd import _lib, addresses
    lib = _lib.get()
    n = len(keys)
    recs = np.zeros(n, dtype=addresses.REC)
    p64 = ctypes.POINTER(ctypes.c_uint64)

    def call():
        _lib.check(lib, lib.bmpow_ident_derive(n, keys.ctypes.data, versions.ctypes.data_as(p64),
                                               streams.ctypes.data_as(p64), recs.ctypes.data), 'bmpow_ident_derive')
    call()  # warm-up: the same shape as the timed calls
    lib.bmpow_ident_reset_stats()
    walls = []
    for _ in range(reps):
        recs[:] = 0  # every timed call fills the records again
        t0 = time.perf_counter()
        call()
        walls.append(time.perf_counter() - t0)
    res = addresses.Identified(recs)
    rmd = OpenSSLRipemd160()
    for i in list(range(0, min(n, DISTINCT), 61)) + [n - 1]:
        ripe, tag, addr = cpu_row(rmd, keys[i].tobytes(), int(versions[i]), int(streams[i]))
        if (res.ripe[i].tobytes(), res.tag[i].tobytes(), res.address(i)) != (ripe, tag, addr):
            raise SystemExit('bmpow_ident_derive disagrees with the CPU at row %d' % i)
    if not np.array_equal(recs[DISTINCT:2 * DISTINCT], recs[:DISTINCT][:len(recs[DISTINCT:2 * DISTINCT])]):
        raise SystemExit('bmpow_ident_derive: equal rows gave different records')
    st = addresses.stats()
    return {'calls': reps, 'rows': st['rows'], 'sets': st['sets'], 'launches': st['launches'],
            'kernel_ms': round(st['kernel_ms'] / reps, 4), 'host_ms': round(st['host_ms'] / reps, 3),
            'rows_per_s_kernel': st['rows'] / (st['kernel_ms'] / 1e3), 'wall_s': [round(w, 5) for w in walls],
            'rows_per_s_wall': n / min(walls), 'bytes_in_per_row': 144, 'bytes_out_per_row': addresses.REC.itemsize}


def _cpu_worker(args):
    rows, seconds = args
    from oracle.addrgen_oracle import OpenSSLRipemd160
    rmd = OpenSSLRipemd160()
    done = 0
    end = time.perf_counter() + seconds
    while time.perf_counter() < end:
        for key, version, stream in rows:
            cpu_row(rmd, key, version, stream)
            done += 1
    return done, time.perf_counter() - (end - seconds)


def cpu_leg(keys, versions, streams, seconds):
    procs = max(1, min(16, len(os.sched_getaffinity(0)), int(os.environ.get('OMP_NUM_THREADS', '16'))))
    sample = [(keys[i].tobytes(), int(versions[i]), int(streams[i])) for i in range(min(len(keys), 1024))]
    with multiprocessing.get_context('spawn').Pool(procs) as pool:
        res = pool.map(_cpu_worker, [(sample, seconds)] * procs)
    rate = sum(d / s for d, s in res)
    return {'processes': procs, 'seconds': seconds, 'rows': sum(d for d, _ in res), 'rows_per_s': rate,
            'us_per_row_one_core': 1e6 * procs / rate}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--rows', type=int, default=500000)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--cpu-seconds', type=float, default=2.0)
    ap.add_argument('--no-cpu', action='store_true')
    ap.add_argument('--cpu-only', action='store_true')
    ap.add_argument('--out', default=None, help='where the JSON line is written as well')
    a = ap.parse_args()
    keys, versions, streams = make_inputs(a.rows)
    out = {'rows': a.rows}
    if not a.cpu_only:
        out['gpu'] = gpu_leg(keys, versions, streams, a.reps)
    if not a.no_cpu:
        out['cpu'] = cpu_leg(keys, versions, streams, a.cpu_seconds)
    if 'gpu' in out and 'cpu' in out:
        out['speedup_kernel'] = out['gpu']['rows_per_s_kernel'] / out['cpu']['rows_per_s']
        out['speedup_wall'] = out['gpu']['rows_per_s_wall'] / out['cpu']['rows_per_s']
    line = json.dumps(out)
    print(line)
    path = a.out or os.path.join(ROOT, 'profiles', 'ident', 'rate_n%d.json' % a.rows)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
