#!/usr/bin/env python3
"""Rate of the batched ECIES trial decryption (bmpow_ecies_match) beside the same try on the CPU.

    python tools/ecies_rate.py --objects 500000 --keys 10 --len 200

GPU leg: N payloads of L bytes against K keys through ``bmpow_ecies_match``, after a warm-up call of the
same shapes.  The rates come from the library's own device events, recorded on the stream around each
launch while the set's objects are resident (``bmpow_ecies_get_stats``): pairs/s over the three
kernels' time, ms per (ladder + MAC) launch, objects/s at K keys; the wall time of the call (parsing,
padding, upload, launches) is reported beside them as the end-to-end figure.  One payload in a
thousand is addressed to key 0, the rest to nobody, as on the network.  The N payloads cycle through
4,096 distinct byte strings; the library pads, uploads and tries every one of the N on its own.

CPU leg: the reference's try (EC_POINT_set_affine_coordinates, ECDH_compute_key, SHA-512, HMAC-SHA256
over the blob: src/pyelliptic/ecc.py:203-257, :484-499) through libcrypto, in as many processes as
the CPU quota allows (16 at most), each for --cpu-seconds.

Prints one JSON line.  Without a device the GPU leg raises (there is no fallback); --cpu-only runs the
CPU leg alone."""
import argparse
import ctypes
import ctypes.util
import hashlib
import hmac
import json
import multiprocessing
import os
import random
import struct
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

P = 2 ** 256 - 2 ** 32 - 977
N_ORDER = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
G = (0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798,
     0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8)
DISTINCT = 4096


def ec_add(a, b):
    if a is None:
        return b
    if b is None:
        return a
    if a[0] == b[0]:
        if (a[1] + b[1]) % P == 0:
            return None
        lam = 3 * a[0] * a[0] * pow(2 * a[1], -1, P) % P
    else:
        lam = (b[1] - a[1]) * pow(b[0] - a[0], -1, P) % P
    x = (lam * lam - a[0] - b[0]) % P
    return x, (lam * (a[0] - x) - a[1]) % P


def ec_mul(k, pt):
    acc = None
    while k:
        if k & 1:
            acc = ec_add(acc, pt)
        pt = ec_add(pt, pt)
        k >>= 1
    return acc


def make_inputs(n, nkeys, length, seed=20250216):
    """(payloads, keys, expected match per payload): every payload is ``length`` bytes."""
    if length < 118:
        raise SystemExit('--len must be at least 118 (16 iv + 70 key header + 32 MAC)')
    rng = random.Random(seed)
    keys = [rng.randrange(1, N_ORDER) for _ in range(nkeys)]
    points = [ec_mul(rng.randrange(1, N_ORDER), G) for _ in range(64)]
    shared = [ec_mul(keys[0], pt)[0] for pt in points]
    distinct, want = [], []
    for i in range(min(n, DISTINCT)):
        j = i % 64
        x, y = points[j]
        head = (rng.getrandbits(128).to_bytes(16, 'big') + struct.pack('!HH', 714, 32) + x.to_bytes(32, 'big') +
                struct.pack('!H', 32) + y.to_bytes(32, 'big') + rng.getrandbits(8 * (length - 118)).to_bytes(length - 118, 'big'))
        mine = i % 1000 == 999
        km = hashlib.sha512((shared[j] if mine else rng.getrandbits(256)).to_bytes(32, 'big')).digest()[32:]
        distinct.append(head + hmac.new(km, head, hashlib.sha256).digest())
        want.append(0 if mine else -1)
    reps = (n + len(distinct) - 1) // len(distinct)
    return (distinct * reps)[:n], [k.to_bytes(32, 'big') for k in keys], (want * reps)[:n]


def gpu_leg(payloads, keys, want, reps):
    import numpy as np
    from pybitmessage_amd import _lib
    lib = _lib.get()
    n, nk = len(payloads), len(keys)
    ptrs = (ctypes.c_char_p * n)(*payloads)
    lens = np.fromiter(map(len, payloads), dtype=np.uint64, count=n)
    match = np.zeros(n, dtype=np.int32)
    kb = b''.join(keys)

    def call(m):
        _lib.check(lib, lib.bmpow_ecies_match(m, ctypes.cast(ptrs, ctypes.c_void_p),
                                              lens.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), nk, kb,
                                              match.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), None),
                   'bmpow_ecies_match')
    call(n)  # warm-up: the same shapes as the timed calls
    if (match != np.asarray(want, dtype=np.int32)).any():
        raise SystemExit('bmpow_ecies_match disagrees with the expected matches')
    lib.bmpow_ecies_reset_stats()
    walls = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call(n)
        walls.append(time.perf_counter() - t0)
    st = _lib.BmpowEciesStats()
    _lib.check(lib, lib.bmpow_ecies_get_stats(ctypes.byref(st)), 'bmpow_ecies_get_stats')
    dev_ms = st.prep_ms + st.ecdh_ms + st.mac_ms
    return {'calls': reps, 'pairs': st.pairs, 'launches': st.launches,
            'prep_ms': round(st.prep_ms / reps, 3), 'ecdh_ms': round(st.ecdh_ms / reps, 3),
            'mac_ms': round(st.mac_ms / reps, 3), 'ms_per_launch': round((st.ecdh_ms + st.mac_ms) / st.launches, 3),
            'pairs_per_s': st.pairs / (dev_ms / 1e3), 'objects_per_s': st.objects / (dev_ms / 1e3),
            'ecdh_pairs_per_s': st.pairs / (st.ecdh_ms / 1e3),
            'wall_s': [round(w, 4) for w in walls], 'wall_objects_per_s': n / min(walls),
            'wall_pairs_per_s': n * nk / min(walls), 'matches': int((match >= 0).sum())}


def _cpu_worker(args):
    payloads, key, seconds = args
    lc = ctypes.CDLL(ctypes.util.find_library('crypto') or 'libcrypto.so.3')
    vp = ctypes.c_void_p
    for name, res, argt in [('EC_GROUP_new_by_curve_name', vp, [ctypes.c_int]), ('EC_POINT_new', vp, [vp]),
                            ('EC_POINT_free', None, [vp]), ('BN_bin2bn', vp, [ctypes.c_char_p, ctypes.c_int, vp]),
                            ('BN_free', None, [vp]), ('EC_KEY_new_by_curve_name', vp, [ctypes.c_int]),
                            ('EC_KEY_set_private_key', ctypes.c_int, [vp, vp]),
                            ('EC_POINT_set_affine_coordinates', ctypes.c_int, [vp, vp, vp, vp, vp]),
                            ('ECDH_compute_key', ctypes.c_int, [ctypes.c_char_p, ctypes.c_size_t, vp, vp, vp])]:
        fn = getattr(lc, name)
        fn.restype, fn.argtypes = res, argt
    group = lc.EC_GROUP_new_by_curve_name(714)
    own = lc.EC_KEY_new_by_curve_name(714)
    bn = lc.BN_bin2bn(key, 32, None)
    assert lc.EC_KEY_set_private_key(own, bn) == 1
    buf = ctypes.create_string_buffer(32)
    tries = matches = 0
    end = time.perf_counter() + seconds
    while time.perf_counter() < end:
        for data in payloads:
            xl = struct.unpack('!H', data[18:20])[0]
            yl = struct.unpack('!H', data[20 + xl:22 + xl])[0]
            bx = lc.BN_bin2bn(data[20:20 + xl], xl, None)
            by = lc.BN_bin2bn(data[22 + xl:22 + xl + yl], yl, None)
            pt = lc.EC_POINT_new(group)
            if lc.EC_POINT_set_affine_coordinates(group, pt, bx, by, None) == 1 and \
                    lc.ECDH_compute_key(buf, 32, pt, own, None) == 32:
                km = hashlib.sha512(buf.raw).digest()[32:]
                matches += hmac.new(km, data[:-32], hashlib.sha256).digest() == data[-32:]
            lc.EC_POINT_free(pt)
            lc.BN_free(bx)
            lc.BN_free(by)
            tries += 1
    return tries, matches, time.perf_counter() - (end - seconds)


def cpu_leg(payloads, keys, seconds):
    procs = max(1, min(16, len(os.sched_getaffinity(0)), int(os.environ.get('OMP_NUM_THREADS', '16'))))
    sample = payloads[:256]
    with multiprocessing.get_context('spawn').Pool(procs) as pool:
        res = pool.map(_cpu_worker, [(sample, keys[0], seconds)] * procs)
    rate = sum(t / s for t, _, s in res)
    return {'processes': procs, 'seconds': seconds, 'tries': sum(t for t, _, _ in res), 'pairs_per_s': rate,
            'ms_per_try_one_core': 1e3 * procs / rate}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--objects', type=int, default=500000)
    ap.add_argument('--keys', type=int, default=10)
    ap.add_argument('--len', type=int, default=200, dest='length', help='payload bytes, MAC included')
    ap.add_argument('--reps', type=int, default=2)
    ap.add_argument('--cpu-seconds', type=float, default=3.0)
    ap.add_argument('--no-cpu', action='store_true')
    ap.add_argument('--cpu-only', action='store_true')
    a = ap.parse_args()
    payloads, keys, want = make_inputs(a.objects, a.keys, a.length)
    out = {'objects': a.objects, 'keys': a.keys, 'len': a.length}
    if not a.cpu_only:
        out['gpu'] = gpu_leg(payloads, keys, want, a.reps)
    if not a.no_cpu:
        out['cpu'] = cpu_leg(payloads, keys, a.cpu_seconds)
    if 'gpu' in out and 'cpu' in out:
        out['speedup_device'] = out['gpu']['pairs_per_s'] / out['cpu']['pairs_per_s']
        out['speedup_wall'] = out['gpu']['wall_pairs_per_s'] / out['cpu']['pairs_per_s']
    print(json.dumps(out))


if __name__ == '__main__':
    main()
