#!/usr/bin/env python3
"""Rate of the batched signing and ECIES encryption (bmpow_sig_sign, bmpow_ecies_encrypt) beside the same
steps on the CPU.

    python tools/send_rate.py --rows 500000 --len 200

GPU leg: N messages of L bytes through ``bmpow_sig_sign`` (SHA-256, the nonces drawn by the library) and N
plaintexts of L bytes through ``bmpow_ecies_encrypt`` (ephemeral keys and IVs drawn by the library), from
host buffers, each after a warm-up call of the same shapes whose results the receive side checks (a sample
through ``bmpow_sig_verify`` and ``bmpow_ecies_match`` + ``bmpow_ecies_decrypt``).  The per-phase times are
the library's own device events (``bmpow_send_get_stats``): rows/s over the kernels' time; ``seal_ms`` is
the host's AES + HMAC pass; the wall time of the call (draws, padding, upload, launches, the seal) is
reported beside them as the end-to-end figure.  The N rows cycle through 4,096 distinct messages under 64
keys; the library draws, pads, uploads and computes every one of the N on its own.

CPU leg: the reference's steps through libcrypto, in as many processes as the CPU quota allows (16 at
most), each for --cpu-seconds: SHA-256 + ``ECDSA_sign`` (src/pyelliptic/ecc.py:319-385), and for ECIES a
generated key pair, ``ECDH_compute_key``, SHA-512, AES-256-CBC and HMAC-SHA256 (:462-482).

Prints one JSON line.  Without a device the GPU leg raises (there is no fallback); --cpu-only runs the
CPU leg alone.

    python tools/send_rate.py --rows 500000 --len 200 --seal both --out profiles/send/seal_ab_l200.json

--seal host|device|both measures ``bmpow_ecies_encrypt`` alone with the blobs sealed on the host's threads or
by the seal kernel (``bmpow_send_set_seal``): under the same seeded ephemeral keys and IVs, each mode warmed,
then --reps timed calls each (three at least), the modes taking turns in one process.  The JSON holds every
repetition's wall time, the per-call split of ``bmpow_send_stats`` and ``bmpow_seal_stats``, a byte-for-byte
comparison of the two modes' blobs, and the verdict of the rule that decides the library's default: the device
mode's median must beat the host mode's by more than the spread of the host's own repetitions and by 1 %."""
import argparse
import ctypes
import ctypes.util
import hashlib
import hmac
import json
import multiprocessing
import os
import random
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N_ORDER = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
DISTINCT = 4096
KEYS = 64
NID_SECP256K1 = 714


def libcrypto():
    lc = ctypes.CDLL(ctypes.util.find_library('crypto') or 'libcrypto.so.3')
    vp, cp, ci = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int
    for name, res, argt in [('EC_KEY_new_by_curve_name', vp, [ci]), ('EC_KEY_free', None, [vp]),
                            ('EC_KEY_generate_key', ci, [vp]), ('EC_KEY_get0_group', vp, [vp]),
                            ('EC_KEY_get0_public_key', vp, [vp]), ('EC_KEY_set_private_key', ci, [vp, vp]),
                            ('EC_POINT_new', vp, [vp]), ('EC_POINT_free', None, [vp]),
                            ('EC_POINT_mul', ci, [vp, vp, vp, vp, vp, vp]), ('BN_bin2bn', vp, [cp, ci, vp]),
                            ('BN_free', None, [vp]), ('EC_POINT_set_affine_coordinates', ci, [vp, vp, vp, vp, vp]),
                            ('EC_POINT_point2oct', ctypes.c_size_t, [vp, vp, ci, cp, ctypes.c_size_t, vp]),
                            ('ECDSA_sign', ci, [ci, cp, ci, cp, ctypes.POINTER(ctypes.c_uint), vp]),
                            ('ECDH_compute_key', ci, [cp, ctypes.c_size_t, vp, vp, vp]),
                            ('EVP_CIPHER_CTX_new', vp, []), ('EVP_CIPHER_CTX_free', None, [vp]), ('EVP_aes_256_cbc', vp, []),
                            ('EVP_EncryptInit_ex', ci, [vp, vp, vp, cp, cp]),
                            ('EVP_EncryptUpdate', ci, [vp, cp, ctypes.POINTER(ci), cp, ci]),
                            ('EVP_EncryptFinal_ex', ci, [vp, cp, ctypes.POINTER(ci)]), ('RAND_bytes', ci, [cp, ci])]:
        fn = getattr(lc, name)
        fn.restype, fn.argtypes = res, argt
    return lc


def make_inputs(n, length, seed=20251019):
    """(messages, private keys, the keys' public halves X || Y): every message is ``length`` bytes."""
    lc = libcrypto()
    rng = random.Random(seed)
    privs, pubs = [], []
    for _ in range(KEYS):
        d = rng.randrange(1, N_ORDER).to_bytes(32, 'big')
        k = lc.EC_KEY_new_by_curve_name(NID_SECP256K1)
        group = lc.EC_KEY_get0_group(k)
        bn, pt = lc.BN_bin2bn(d, 32, None), lc.EC_POINT_new(group)
        assert lc.EC_POINT_mul(group, pt, bn, None, None, None) == 1
        buf = ctypes.create_string_buffer(65)
        assert lc.EC_POINT_point2oct(group, pt, 4, buf, 65, None) == 65
        privs.append(d)
        pubs.append(buf.raw[1:])
        lc.EC_POINT_free(pt)
        lc.BN_free(bn)
        lc.EC_KEY_free(k)
    msgs = [rng.getrandbits(8 * length).to_bytes(length, 'big') if length else b'' for _ in range(min(n, DISTINCT))]
    reps = (n + len(msgs) - 1) // len(msgs)
    return (msgs * reps)[:n], [privs[i % KEYS] for i in range(n)], [pubs[i % KEYS] for i in range(n)]


def gpu_leg(msgs, privs, pubs, reps):
    import numpy as np
    from pybitmessage_amd import _lib, ecies, signatures
    lib = _lib.get()
    n = len(msgs)
    p64, pu8 = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint8)
    mp = (ctypes.c_char_p * n)(*msgs)
    ml = np.fromiter(map(len, msgs), dtype=np.uint64, count=n)
    pk, qk = b''.join(privs), b''.join(pubs)
    sig = np.zeros((n, 72), dtype=np.uint8)
    sl = np.zeros(n, dtype=np.uint8)
    caps = 118 + 16 * (ml // 16 + 1)
    offs = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(caps, out=offs[1:])
    arena = np.zeros(int(offs[-1]), dtype=np.uint8)
    outs = (arena.ctypes.data + offs[:-1]).astype(np.uint64)
    got = np.zeros(n, dtype=np.uint64)

    def sign():
        _lib.check(lib, lib.bmpow_sig_sign(n, ctypes.cast(mp, ctypes.c_void_p), ml.ctypes.data_as(p64), pk, 2, None,
                                           sig.ctypes.data_as(pu8), sl.ctypes.data_as(pu8)), 'bmpow_sig_sign')

    def encrypt():
        _lib.check(lib, lib.bmpow_ecies_encrypt(n, ctypes.cast(mp, ctypes.c_void_p), ml.ctypes.data_as(p64), qk, None, None,
                                                outs.ctypes.data_as(ctypes.c_void_p), caps.ctypes.data_as(p64),
                                                got.ctypes.data_as(p64)), 'bmpow_ecies_encrypt')

    def timed(call):
        call()  # warm-up: the same shapes as the timed calls (and the comb table's build)
        lib.bmpow_send_reset_stats()
        walls = []
        for _ in range(reps):
            t0 = time.perf_counter()
            call()
            walls.append(time.perf_counter() - t0)
        st = _lib.BmpowSendStats()
        _lib.check(lib, lib.bmpow_send_get_stats(ctypes.byref(st)), 'bmpow_send_get_stats')
        dev_ms = st.hash_ms + st.comb_ms + st.scalar_ms + st.ladder_ms
        out = {f: round(getattr(st, f) / reps, 3) for f in ('hash_ms', 'comb_ms', 'scalar_ms', 'ladder_ms', 'seal_ms', 'host_ms')}
        out.update({'calls': reps, 'rows': st.rows, 'sets': st.sets, 'launches': st.launches,
                    'rows_per_s': st.rows / (dev_ms / 1e3), 'kernel_us_per_row': 1e3 * dev_ms / st.rows,
                    'wall_s': [round(w, 4) for w in walls], 'wall_rows_per_s': n / min(walls)})
        return out

    res = {'sign': timed(sign)}
    pick = list(range(0, n, max(1, n // 256)))[:256]
    sigs = [sig[i, :int(sl[i])].tobytes() for i in pick]
    if signatures.verify_batch_digest([msgs[i] for i in pick], sigs, [pubs[i] for i in pick]) != [2] * len(pick):
        raise SystemExit('bmpow_sig_verify refuses a signature bmpow_sig_sign made')
    res['encrypt'] = timed(encrypt)
    blobs = [arena[int(offs[i]):int(offs[i]) + int(got[i])].tobytes() for i in pick]
    if ecies.decrypt_batch(blobs, privs[:KEYS]) != [(i % KEYS, msgs[i]) for i in pick]:
        raise SystemExit('bmpow_ecies_match / decrypt does not open a blob bmpow_ecies_encrypt made')
    return res


def seal_ab(msgs, privs, pubs, reps, which):
    """``bmpow_ecies_encrypt`` under each seal mode in turn, same seeded ephemeral keys and IVs."""
    import numpy as np
    from pybitmessage_amd import _lib, ecies
    lib = _lib.get()
    n = len(msgs)
    reps = max(3, reps)
    p64, pu8 = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint8)
    rng = np.random.default_rng(20261020)
    eph = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    eph[:, 0] &= 0x7f  # below the group order
    eph[:, 31] |= 1    # and not zero
    ivs = rng.integers(0, 256, size=(n, 16), dtype=np.uint8)
    mp = (ctypes.c_char_p * n)(*msgs)
    ml = np.fromiter(map(len, msgs), dtype=np.uint64, count=n)
    qk = b''.join(pubs)
    caps = 118 + 16 * (ml // 16 + 1)
    offs = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(caps, out=offs[1:])
    modes = {'host': 0, 'device': 1}
    names = ['host', 'device'] if which == 'both' else [which]
    arena = {m: np.zeros(int(offs[-1]), dtype=np.uint8) for m in names}
    got = {m: np.zeros(n, dtype=np.uint64) for m in names}

    def call(m):
        outs = (arena[m].ctypes.data + offs[:-1]).astype(np.uint64)
        lib.bmpow_send_set_seal(modes[m])
        t0 = time.perf_counter()
        _lib.check(lib, lib.bmpow_ecies_encrypt(n, ctypes.cast(mp, ctypes.c_void_p), ml.ctypes.data_as(p64), qk,
                                                eph.ctypes.data_as(ctypes.c_char_p), ivs.ctypes.data_as(ctypes.c_char_p),
                                                outs.ctypes.data_as(ctypes.c_void_p), caps.ctypes.data_as(p64),
                                                got[m].ctypes.data_as(p64)), 'bmpow_ecies_encrypt')
        return time.perf_counter() - t0

    first = lib.bmpow_send_set_seal(-1)
    res = {m: {'wall_s': [], 'send': {}, 'seal': {}} for m in names}
    try:
        for m in names:
            call(m)  # warm-up: the same shapes (and the comb table's build)
        for _ in range(reps):
            for m in names:
                lib.bmpow_send_reset_stats()
                lib.bmpow_seal_reset_stats()
                res[m]['wall_s'].append(round(call(m), 5))
                st, sl = _lib.BmpowSendStats(), _lib.BmpowSealStats()
                _lib.check(lib, lib.bmpow_send_get_stats(ctypes.byref(st)), 'bmpow_send_get_stats')
                _lib.check(lib, lib.bmpow_seal_get_stats(ctypes.byref(sl)), 'bmpow_seal_get_stats')
                for f in ('comb_ms', 'scalar_ms', 'ladder_ms', 'seal_ms', 'host_ms'):
                    res[m]['send'].setdefault(f, []).append(round(getattr(st, f), 3))
                for f, _ in sl._fields_:
                    res[m]['seal'].setdefault(f, []).append(round(getattr(sl, f), 3))
    finally:
        lib.bmpow_send_set_seal(first)
    out = {'reps': reps, 'default_mode': 'device' if first else 'host', 'modes': res}
    for m in names:
        w = sorted(res[m]['wall_s'])
        res[m]['median_s'] = w[len(w) // 2] if len(w) % 2 else (w[len(w) // 2 - 1] + w[len(w) // 2]) / 2
        res[m]['spread_s'] = round(w[-1] - w[0], 5)
        res[m]['blobs_made'] = int(np.count_nonzero(got[m]))
    pick = list(range(0, n, max(1, n // 256)))[:256]
    m0 = names[-1]
    blobs = [arena[m0][int(offs[i]):int(offs[i]) + int(got[m0][i])].tobytes() for i in pick]
    if ecies.decrypt_batch(blobs, privs[:KEYS]) != [(i % KEYS, msgs[i]) for i in pick]:
        raise SystemExit('bmpow_ecies_match / decrypt does not open a blob bmpow_ecies_encrypt (%s) made' % m0)
    if which == 'both':
        same = bool(np.array_equal(got['host'], got['device']) and np.array_equal(arena['host'], arena['device']))
        h, d = res['host'], res['device']
        gain = h['median_s'] - d['median_s']
        out['blobs_identical'] = same
        out['blob_bytes_compared'] = int(got['host'].sum())
        out['device_gain_s'] = round(gain, 5)
        out['device_gain_pct'] = round(100 * gain / h['median_s'], 2)
        out['device_wins'] = bool(same and gain > h['spread_s'] and gain >= 0.01 * h['median_s'])
    return out


def _cpu_worker(args):
    kind, msgs, privs, pubs, seconds = args
    lc = libcrypto()
    keys = []
    for d, q in zip(privs, pubs):
        k = lc.EC_KEY_new_by_curve_name(NID_SECP256K1)
        assert lc.EC_KEY_set_private_key(k, lc.BN_bin2bn(d, 32, None)) == 1
        keys.append((k, q))
    done = 0
    end = time.perf_counter() + seconds
    sig = ctypes.create_string_buffer(80)
    slen = ctypes.c_uint(0)
    shared = ctypes.create_string_buffer(32)
    iv = ctypes.create_string_buffer(16)
    n1, n2 = ctypes.c_int(0), ctypes.c_int(0)
    while time.perf_counter() < end:
        for i, msg in enumerate(msgs):
            k, q = keys[i % len(keys)]
            if kind == 'sign':
                assert lc.ECDSA_sign(0, hashlib.sha256(msg).digest(), 32, sig, ctypes.byref(slen), k) == 1
            else:
                eph = lc.EC_KEY_new_by_curve_name(NID_SECP256K1)
                assert lc.EC_KEY_generate_key(eph) == 1
                group = lc.EC_KEY_get0_group(eph)
                head = ctypes.create_string_buffer(65)
                lc.EC_POINT_point2oct(group, lc.EC_KEY_get0_public_key(eph), 4, head, 65, None)
                bx, by, pt = lc.BN_bin2bn(q[:32], 32, None), lc.BN_bin2bn(q[32:], 32, None), lc.EC_POINT_new(group)
                assert lc.EC_POINT_set_affine_coordinates(group, pt, bx, by, None) == 1
                assert lc.ECDH_compute_key(shared, 32, pt, eph, None) == 32
                key = hashlib.sha512(shared.raw).digest()
                lc.RAND_bytes(iv, 16)
                ct = ctypes.create_string_buffer(len(msg) + 16)
                ctx = lc.EVP_CIPHER_CTX_new()
                lc.EVP_EncryptInit_ex(ctx, lc.EVP_aes_256_cbc(), None, key[:32], iv.raw)
                lc.EVP_EncryptUpdate(ctx, ct, ctypes.byref(n1), msg, len(msg))
                lc.EVP_EncryptFinal_ex(ctx, ctypes.cast(ctypes.addressof(ct) + n1.value, ctypes.c_char_p), ctypes.byref(n2))
                lc.EVP_CIPHER_CTX_free(ctx)
                body = iv.raw + b'\x02\xca\x00\x20' + head.raw[1:33] + b'\x00\x20' + head.raw[33:] + ct.raw[:n1.value + n2.value]
                hmac.new(key[32:], body, hashlib.sha256).digest()
                lc.EC_POINT_free(pt)
                lc.BN_free(bx)
                lc.BN_free(by)
                lc.EC_KEY_free(eph)
            done += 1
    return done, time.perf_counter() - (end - seconds)


def cpu_leg(kind, msgs, privs, pubs, seconds):
    procs = max(1, min(16, len(os.sched_getaffinity(0)), int(os.environ.get('OMP_NUM_THREADS', '16'))))
    with multiprocessing.get_context('spawn').Pool(procs) as pool:
        res = pool.map(_cpu_worker, [(kind, msgs[:256], privs[:KEYS], pubs[:KEYS], seconds)] * procs)
    rate = sum(t / s for t, s in res)
    return {'processes': procs, 'seconds': seconds, 'rows': sum(t for t, _ in res), 'rows_per_s': rate,
            'ms_per_row_one_core': 1e3 * procs / rate}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--rows', type=int, default=500000)
    ap.add_argument('--len', type=int, default=200, dest='length', help='message / plaintext bytes')
    ap.add_argument('--reps', type=int, default=2)
    ap.add_argument('--cpu-seconds', type=float, default=3.0)
    ap.add_argument('--no-cpu', action='store_true')
    ap.add_argument('--cpu-only', action='store_true')
    ap.add_argument('--seal', choices=('host', 'device', 'both'),
                    help='measure bmpow_ecies_encrypt alone under this seal mode (both: A/B in one process)')
    ap.add_argument('--out', help='with --seal: also write the JSON to this file')
    a = ap.parse_args()
    msgs, privs, pubs = make_inputs(a.rows, a.length)
    out = {'rows': a.rows, 'len': a.length}
    if a.seal:
        out['seal_ab'] = seal_ab(msgs, privs, pubs, a.reps, a.seal)
        if a.out:
            with open(a.out, 'w') as f:
                json.dump(out, f, indent=1)
                f.write('\n')
        print(json.dumps(out))
        return
    if not a.cpu_only:
        out['gpu'] = gpu_leg(msgs, privs, pubs, a.reps)
    if not a.no_cpu:
        out['cpu'] = {kind: cpu_leg(kind, msgs, privs, pubs, a.cpu_seconds) for kind in ('sign', 'encrypt')}
    if 'gpu' in out and 'cpu' in out:
        for kind in ('sign', 'encrypt'):
            out['speedup_device_' + kind] = out['gpu'][kind]['rows_per_s'] / out['cpu'][kind]['rows_per_s']
            out['speedup_wall_' + kind] = out['gpu'][kind]['wall_rows_per_s'] / out['cpu'][kind]['rows_per_s']
    print(json.dumps(out))


if __name__ == '__main__':
    main()
