#!/usr/bin/env python3
"""Rate of the batched signature verification (bmpow_sig_verify) beside the same check on the CPU.

    python tools/sig_rate.py --sigs 500000 --len 200

GPU leg: N (message, signature, key) triples over messages of L bytes through ``bmpow_sig_verify``, after
a warm-up call of the same shapes.  The rates come from the library's own device events, recorded on
the stream around each phase's launches (``bmpow_sig_get_stats``): signatures/s over the three phases'
time and each phase's share; the wall time of the call (parsing, padding, upload, launches) is reported
beside them as the end-to-end figure.  The signatures are made under SHA-256, today's signing default,
so every one takes both tries, as in the reference; one in a thousand is invalid (its message altered).
The N triples cycle through 4,096 distinct ones under 64 keys; the library parses, pads, uploads and
verifies every one of the N on its own.

CPU leg: the reference's check (``highlevelcrypto.verify``, src/highlevelcrypto.py:88-108: per try a key
object built and checked, the digest, ``ECDSA_verify``; SHA-1 first, then SHA-256:
src/pyelliptic/ecc.py:387-440) through libcrypto, in as many processes as the CPU quota allows (16 at
most), each for --cpu-seconds.

Prints one JSON line.  Without a device the GPU leg raises (there is no fallback); --cpu-only runs the
CPU leg alone."""
import argparse
import ctypes
import ctypes.util
import hashlib
import json
import multiprocessing
import os
import random
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DISTINCT = 4096
KEYS = 64
NID_SECP256K1 = 714


def libcrypto():
    lc = ctypes.CDLL(ctypes.util.find_library('crypto') or 'libcrypto.so.3')
    vp = ctypes.c_void_p
    for name, res, argt in [('EC_KEY_new_by_curve_name', vp, [ctypes.c_int]), ('EC_KEY_free', None, [vp]),
                            ('EC_KEY_generate_key', ctypes.c_int, [vp]), ('EC_KEY_get0_group', vp, [vp]),
                            ('EC_KEY_get0_public_key', vp, [vp]), ('EC_KEY_set_public_key', ctypes.c_int, [vp, vp]),
                            ('EC_KEY_check_key', ctypes.c_int, [vp]), ('EC_POINT_new', vp, [vp]),
                            ('EC_POINT_free', None, [vp]), ('BN_bin2bn', vp, [ctypes.c_char_p, ctypes.c_int, vp]),
                            ('BN_free', None, [vp]),
                            ('EC_POINT_set_affine_coordinates', ctypes.c_int, [vp, vp, vp, vp, vp]),
                            ('EC_POINT_point2oct', ctypes.c_size_t,
                             [vp, vp, ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t, vp]),
                            ('ECDSA_sign', ctypes.c_int, [ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p,
                                                          ctypes.POINTER(ctypes.c_uint), vp]),
                            ('ECDSA_verify', ctypes.c_int, [ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p,
                                                            ctypes.c_int, vp])]:
        fn = getattr(lc, name)
        fn.restype, fn.argtypes = res, argt
    return lc


def make_inputs(n, length, seed=20251019):
    """(msgs, sigs, keys, expected code per triple): every message is ``length`` bytes."""
    lc = libcrypto()
    rng = random.Random(seed)
    signers = []
    for _ in range(KEYS):
        k = lc.EC_KEY_new_by_curve_name(NID_SECP256K1)
        assert lc.EC_KEY_generate_key(k) == 1
        buf = ctypes.create_string_buffer(65)
        assert lc.EC_POINT_point2oct(lc.EC_KEY_get0_group(k), lc.EC_KEY_get0_public_key(k), 4, buf, 65, None) == 65
        signers.append((k, buf.raw[1:]))
    msgs, sigs, keys, want = [], [], [], []
    for i in range(min(n, DISTINCT)):
        k, pub = signers[i % KEYS]
        msg = rng.getrandbits(8 * length).to_bytes(length, 'big') if length else b''
        sig = ctypes.create_string_buffer(80)
        slen = ctypes.c_uint(0)
        assert lc.ECDSA_sign(0, hashlib.sha256(msg).digest(), 32, sig, ctypes.byref(slen), k) == 1
        bad = i % 1000 == 999
        msgs.append(msg[:-1] + bytes([msg[-1] ^ 1]) if bad and length else msg)
        sigs.append(sig.raw[:slen.value])
        keys.append(pub)
        want.append(0 if bad and length else 2)
    for k, _ in signers:
        lc.EC_KEY_free(k)
    reps = (n + len(msgs) - 1) // len(msgs)
    return (msgs * reps)[:n], (sigs * reps)[:n], (keys * reps)[:n], (want * reps)[:n]


def gpu_leg(msgs, sigs, keys, want, reps):
    import numpy as np
    from pybitmessage_amd import _lib
    lib = _lib.get()
    n = len(msgs)
    mp = (ctypes.c_char_p * n)(*msgs)
    sp = (ctypes.c_char_p * n)(*sigs)
    ml = np.fromiter(map(len, msgs), dtype=np.uint64, count=n)
    sl = np.fromiter(map(len, sigs), dtype=np.uint64, count=n)
    kb = b''.join(keys)
    verdict = np.zeros(n, dtype=np.uint8)
    p64, pu8 = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint8)

    def call():
        _lib.check(lib, lib.bmpow_sig_verify(n, ctypes.cast(mp, ctypes.c_void_p), ml.ctypes.data_as(p64),
                                             ctypes.cast(sp, ctypes.c_void_p), sl.ctypes.data_as(p64), kb,
                                             verdict.ctypes.data_as(pu8)), 'bmpow_sig_verify')
    call()  # warm-up: the same shapes as the timed calls (and the comb table's build)
    if (verdict != np.asarray(want, dtype=np.uint8)).any():
        raise SystemExit('bmpow_sig_verify disagrees with the expected verdicts')
    lib.bmpow_sig_reset_stats()
    walls = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        walls.append(time.perf_counter() - t0)
    st = _lib.BmpowSigStats()
    _lib.check(lib, lib.bmpow_sig_get_stats(ctypes.byref(st)), 'bmpow_sig_get_stats')
    dev_ms = st.hash_ms + st.scalar_ms + st.curve_ms
    return {'calls': reps, 'uploaded': st.uploaded, 'ladders': st.ladders, 'launches': st.launches,
            'hash_ms': round(st.hash_ms / reps, 3), 'scalar_ms': round(st.scalar_ms / reps, 3),
            'curve_ms': round(st.curve_ms / reps, 3), 'host_ms': round(st.host_ms / reps, 3),
            'sigs_per_s': st.uploaded / (dev_ms / 1e3), 'curve_sigs_per_s': st.uploaded / (st.curve_ms / 1e3),
            'wall_s': [round(w, 4) for w in walls], 'wall_sigs_per_s': n / min(walls),
            'invalid': int((verdict == 0).sum())}


def _cpu_worker(args):
    triples, seconds = args
    lc = libcrypto()

    def one(msg, sig, key, digest):
        k = lc.EC_KEY_new_by_curve_name(NID_SECP256K1)
        bx, by = lc.BN_bin2bn(key[:32], 32, None), lc.BN_bin2bn(key[32:], 32, None)
        group = lc.EC_KEY_get0_group(k)
        pt = lc.EC_POINT_new(group)
        ok = (lc.EC_POINT_set_affine_coordinates(group, pt, bx, by, None) == 1 and lc.EC_KEY_set_public_key(k, pt) == 1 and
              lc.EC_KEY_check_key(k) == 1)
        if ok:
            d = digest(msg).digest()
            ok = lc.ECDSA_verify(0, d, len(d), sig, len(sig), k) == 1
        lc.EC_KEY_free(k)
        lc.BN_free(bx)
        lc.BN_free(by)
        lc.EC_POINT_free(pt)
        return ok

    done = valid = 0
    end = time.perf_counter() + seconds
    while time.perf_counter() < end:
        for msg, sig, key in triples:
            valid += one(msg, sig, key, hashlib.sha1) or one(msg, sig, key, hashlib.sha256)
            done += 1
    return done, valid, time.perf_counter() - (end - seconds)


def cpu_leg(msgs, sigs, keys, seconds):
    procs = max(1, min(16, len(os.sched_getaffinity(0)), int(os.environ.get('OMP_NUM_THREADS', '16'))))
    sample = list(zip(msgs[:256], sigs[:256], keys[:256]))
    with multiprocessing.get_context('spawn').Pool(procs) as pool:
        res = pool.map(_cpu_worker, [(sample, seconds)] * procs)
    rate = sum(t / s for t, _, s in res)
    return {'processes': procs, 'seconds': seconds, 'sigs': sum(t for t, _, _ in res), 'sigs_per_s': rate,
            'ms_per_sig_one_core': 1e3 * procs / rate}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--sigs', type=int, default=500000)
    ap.add_argument('--len', type=int, default=200, dest='length', help='message bytes')
    ap.add_argument('--reps', type=int, default=2)
    ap.add_argument('--cpu-seconds', type=float, default=3.0)
    ap.add_argument('--no-cpu', action='store_true')
    ap.add_argument('--cpu-only', action='store_true')
    a = ap.parse_args()
    msgs, sigs, keys, want = make_inputs(a.sigs, a.length)
    out = {'sigs': a.sigs, 'len': a.length}
    if not a.cpu_only:
        out['gpu'] = gpu_leg(msgs, sigs, keys, want, a.reps)
    if not a.no_cpu:
        out['cpu'] = cpu_leg(msgs, sigs, keys, a.cpu_seconds)
    if 'gpu' in out and 'cpu' in out:
        out['speedup_device'] = out['gpu']['sigs_per_s'] / out['cpu']['sigs_per_s']
        out['speedup_wall'] = out['gpu']['wall_sigs_per_s'] / out['cpu']['sigs_per_s']
    print(json.dumps(out))


if __name__ == '__main__':
    main()
