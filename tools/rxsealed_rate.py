#!/usr/bin/env python3
"""Rate of the one-call opening of received msgs (receive.process_sealed_msgs, bmpow_rx_sealed_msgs) beside the
composition of calls it replaces (receive.process_msgs: bmpow_ecies_match, bmpow_aes256_cbc, bmpow_rx_msgs), in
one process, taking turns.

    python tools/rxsealed_rate.py --msgs 200000 --len 200 --mine 1.0
    python tools/rxsealed_rate.py --msgs 200000 --len 2000 --mine 0.01

N msg objects as they come off the wire, whose message field is L bytes (v4 senders, stream 1, no ackData),
signed (``sender.sign_batch``) and sealed (``sender.encrypt_batch``) on the device.  The user holds 10 keys; a
fraction --mine of the objects is sealed to one of them, the rest to keys the user does not hold (a flood that
is mostly not for the user).  One in a thousand of the user's has a byte of its message altered.  The N cycle
through 4,096 distinct objects; both legs try every key against every one of the N and process every match on
its own.

Each leg is warmed once with the same inputs; then the legs alternate for --reps timed calls each, and the
results (the whole list of ``Msg`` / None) are asserted identical.  A difference between the legs counts when it
exceeds the spread (max - min) of the composition's own calls.  The device time of the phases and the bytes
that cross the bus come from the library's counters.  Prints one JSON line (and writes it to --out).  Without a
device it raises (there is no fallback)."""
import argparse
import ctypes
import hashlib
import json
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DISTINCT = 4096
SENDERS = 64
USER_KEYS = 10


def make_inputs(n, length, mine, seed=20261020):
    from pybitmessage_amd import sender
    from pybitmessage_amd.addressgen import encodeVarint as ev
    rng = random.Random(seed)
    key = lambda: rng.getrandbits(255).to_bytes(32, 'big')  # noqa: E731
    sender_privs = [key() for _ in range(2 * SENDERS)]
    sender_pubs = sender.priv_to_pub(sender_privs)
    user_privs = [key() for _ in range(USER_KEYS)]
    foreign_privs = [key() for _ in range(USER_KEYS)]
    user_pubs = [p[1:] for p in sender.priv_to_pub(user_privs)]
    foreign_pubs = [p[1:] for p in sender.priv_to_pub(foreign_privs)]
    ripes = [hashlib.sha1(b'address %d' % k).digest() for k in range(USER_KEYS)]
    distinct = min(n, DISTINCT)
    every = max(1, int(round(1 / mine))) if mine > 0 else 0
    heads, bodies, to = [], [], []
    for i in range(distinct):
        k = i % SENDERS
        is_mine = every and i % every == 0
        which = rng.randrange(USER_KEYS)
        heads.append(rng.getrandbits(128).to_bytes(16, 'big') + b'\x00\x00\x00\x02' + ev(1) + ev(1))
        message = rng.getrandbits(8 * length).to_bytes(length, 'big') if length else b''
        bodies.append(ev(4) + ev(1) + b'\x00\x00\x00\x01' + sender_pubs[2 * k][1:] + sender_pubs[2 * k + 1][1:] + ev(1000) +
                      ev(1000) + ripes[which] + ev(2) + ev(length) + message + ev(0))
        to.append(user_pubs[which] if is_mine else foreign_pubs[which])
    sigs = sender.sign_batch([h[8:20] + ev(1) + ev(1) + b for h, b in zip(heads, bodies)],
                             [sender_privs[2 * (i % SENDERS)] for i in range(distinct)])
    plains = []
    for i, (b, s) in enumerate(zip(bodies, sigs)):
        if i % 1000 == 999 and length:
            at = len(b) - 2  # the message's last byte
            b = b[:at] + bytes([b[at] ^ 1]) + b[at + 1:]
        plains.append(b + ev(len(s)) + s)
    blobs = sender.encrypt_batch(plains, to, ephemeral=[key() for _ in range(distinct)],
                                 ivs=[rng.getrandbits(128).to_bytes(16, 'big') for _ in range(distinct)])
    objs = [h + b for h, b in zip(heads, blobs)]
    reps = (n + distinct - 1) // distinct
    return (objs * reps)[:n], dict(zip(ripes, user_privs)), len(plains[0])


def spread(xs):
    return {'median_s': round(statistics.median(xs), 4), 'min_s': round(min(xs), 4), 'max_s': round(max(xs), 4),
            'calls_s': [round(x, 4) for x in xs]}


def ecies_stats(lib):
    from pybitmessage_amd import _lib
    st = _lib.BmpowEciesStats()
    _lib.check(lib, lib.bmpow_ecies_get_stats(ctypes.byref(st)), 'bmpow_ecies_get_stats')
    return {f: getattr(st, f) for f, _ in st._fields_}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--msgs', type=int, default=200000)
    ap.add_argument('--len', type=int, default=200, dest='length', help='bytes of the message field')
    ap.add_argument('--mine', type=float, default=1.0, help='fraction of the objects sealed to one of the user\'s keys')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', help='also write the JSON line to this file')
    a = ap.parse_args()
    from pybitmessage_amd import _lib, receive, sender
    objs, keys, plain_len = make_inputs(a.msgs, a.length, a.mine)
    lib = _lib.get()
    want = receive.process_msgs(objs, keys)  # warm-ups, and the comparison
    if receive.process_sealed_msgs(objs, keys) != want:
        raise SystemExit('process_sealed_msgs disagrees with the composition')
    receive.sealed_reset_stats()
    receive.reset_stats()
    sender.reset_seal_stats()
    lib.bmpow_ecies_reset_stats()
    t_one, t_comp = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        got = receive.process_sealed_msgs(objs, keys)
        t_one.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        ref = receive.process_msgs(objs, keys)
        t_comp.append(time.perf_counter() - t0)
        if ref != want or got != want:
            raise SystemExit('a timed call disagrees with the warm-up')
    st, rx, ec, sl = receive.sealed_stats(), receive.stats(), ecies_stats(lib), sender.seal_stats()
    per = lambda v: round(v / a.reps, 3)  # noqa: E731
    diff = statistics.median(t_comp) - statistics.median(t_one)
    matched = st['matched'] // a.reps
    payload_bytes = sum(map(len, objs))
    out = {'msgs': a.msgs, 'len': a.length, 'keys': USER_KEYS, 'mine': a.mine, 'plaintext_bytes': plain_len,
           'object_bytes': len(objs[0]), 'matched_per_call': matched, 'accepted': sum(m is not None for m in want),
           'reps': a.reps,
           'one_call': dict(spread(t_one), msgs_per_s=round(a.msgs / statistics.median(t_one))),
           'composition': dict(spread(t_comp), msgs_per_s=round(a.msgs / statistics.median(t_comp))),
           'composition_spread_s': round(max(t_comp) - min(t_comp), 4), 'median_difference_s': round(diff, 4),
           'difference_exceeds_spread': abs(diff) > max(t_comp) - min(t_comp),
           'one_call_device_ms': {k: per(st[k]) for k in ('match_ms', 'open_ms', 'walk_ms', 'hash_ms', 'scalar_ms', 'curve_ms',
                                                          'ident_ms', 'finish_ms', 'host_ms')},
           'one_call_bytes': {'up': st['bytes_up'] // a.reps, 'down': st['bytes_down'] // a.reps,
                              'objects': payload_bytes},
           'one_call_launches': st['launches'] // a.reps, 'sets_per_call': st['sets'] // a.reps,
           'composition_device_ms': {'match_ms': per(ec['prep_ms'] + ec['ecdh_ms'] + ec['mac_ms']), 'match_host_ms': per(ec['host_ms']),
                                     'aes_kernel_ms': per(sl['seal_kernel_ms']), 'aes_copy_ms': per(sl['copy_ms']),
                                     'aes_pack_scatter_ms': per(sl['pack_ms'] + sl['scatter_ms']),
                                     'walk_ms': per(rx['walk_ms']), 'hash_ms': per(rx['hash_ms']),
                                     'scalar_ms': per(rx['scalar_ms']), 'curve_ms': per(rx['curve_ms']),
                                     'ident_ms': per(rx['ident_ms']), 'finish_ms': per(rx['finish_ms']),
                                     'rx_host_ms': per(rx['host_ms'])}}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
