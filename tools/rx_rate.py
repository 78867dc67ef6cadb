#!/usr/bin/env python3
"""Rate of the one-call msg processing (receive.open_msgs, bmpow_rx_msgs) beside the composition of calls it
replaces, in one process, taking turns.

    python tools/rx_rate.py --msgs 500000 --len 200

N decrypted msgs whose message field is L bytes (v4 senders, stream 1, no ackData), signed on the device
under SHA-256; one in a thousand has a byte of its message altered.  The N cycle through 4,096 distinct msgs
under 64 sender keys; both legs parse, hash and verify every one of the N on its own.

* ``open_msgs``: one ``receive.open_msgs`` call and ``accepted()``.
* ``composition``: what the library offered before: ``signatures.msg_signed_parts`` per object, the toRipe
  comparison, ``signatures.verify_batch_digest``, ``receive.identify`` for the rows that verified, hashlib for
  ``sigHash``.

Each leg is warmed once with the same inputs; then the legs alternate for --reps timed calls each, and the
results (accepted rows, digest, fromAddress, ripe, sigHash) are asserted identical.  A difference between the
legs counts when it exceeds the spread (max - min) of the composition's own calls.  The device time of the
phases comes from the library's events (``bmpow_rx_get_stats`` / ``bmpow_sig_get_stats``).  Prints one JSON
line.  Without a device it raises (there is no fallback)."""
import argparse
import hashlib
import json
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DISTINCT = 4096
KEYS = 64


def make_inputs(n, length, seed=20251024):
    from pybitmessage_amd import sender
    from pybitmessage_amd.addressgen import encodeVarint as ev
    rng = random.Random(seed)
    privs = [rng.getrandbits(255).to_bytes(32, 'big') for _ in range(2 * KEYS)]
    pubs = sender.priv_to_pub(privs)
    to_ripe = hashlib.sha1(b'the recipient').digest()
    heads, bodies = [], []
    for i in range(min(n, DISTINCT)):
        k = i % KEYS
        heads.append(rng.getrandbits(128).to_bytes(16, 'big') + b'\x00\x00\x00\x02' + ev(1) + ev(1))
        message = rng.getrandbits(8 * length).to_bytes(length, 'big') if length else b''
        bodies.append(ev(4) + ev(1) + b'\x00\x00\x00\x01' + pubs[2 * k][1:] + pubs[2 * k + 1][1:] + ev(1000) + ev(1000) +
                      to_ripe + ev(2) + ev(length) + message + ev(0))
    sigs = sender.sign_batch([h[8:20] + ev(1) + ev(1) + b for h, b in zip(heads, bodies)],
                             [privs[2 * (i % KEYS)] for i in range(len(heads))])
    objs, plains = [], []
    for i, (h, b, s) in enumerate(zip(heads, bodies, sigs)):
        if i % 1000 == 999 and length:
            at = len(b) - 2  # the message's last byte
            b = b[:at] + bytes([b[at] ^ 1]) + b[at + 1:]
        objs.append(h + b'the encrypted payload')
        plains.append(b + ev(len(s)) + s)
    reps = (n + len(objs) - 1) // len(objs)
    return (objs * reps)[:n], (plains * reps)[:n], [to_ripe] * n


def leg_open(objs, plains, ripes):
    from pybitmessage_amd import receive
    res = receive.open_msgs(objs, plains, ripes)
    return res, res.accepted()


def rows_of_open(out):
    res, accepted = out
    return [(i, int(res.digest[i]), res.fromAddress(i), res.ripe(i), res.sigHash(i)) for i in accepted]


def sender_fields(plain):
    """(senderVersion, senderStream, endOfThePublicKeyPosition) of a plaintext msg_signed_parts accepted: the
    walk the caller of the composition makes for the toRipe comparison (:531) and for identify."""
    from pybitmessage_amd.ecies import _varint
    ver = _varint(plain[:10])
    stream = _varint(plain[ver[1]:ver[1] + 10])
    pos = ver[1] + stream[1] + 4 + 128
    if ver[0] >= 3:
        for _ in range(2):
            pos += _varint(plain[pos:pos + 10])[1]
    return ver[0], stream[0], pos


def leg_composition(objs, plains, ripes):
    from pybitmessage_amd import receive, signatures
    parts = [signatures.msg_signed_parts(o, p) for o, p in zip(objs, plains)]
    live, fields = [], {}
    for i, (p, plain) in enumerate(zip(parts, plains)):
        if p is None:
            continue
        fields[i] = sender_fields(plain)
        end = fields[i][2]
        if plain[end:end + 20] == ripes[i]:
            live.append(i)
    verdicts = signatures.verify_batch_digest([parts[i][0] for i in live], [parts[i][1] for i in live],
                                              [parts[i][2] for i in live])
    good = [(i, v) for i, v in zip(live, verdicts) if v]
    who = receive.identify([parts[i] for i, _ in good], [fields[i][0] for i, _ in good], [fields[i][1] for i, _ in good])
    return [(i, v, address, ripe, hashlib.sha512(hashlib.sha512(parts[i][1]).digest()).digest()[32:])
            for (i, v), (address, ripe) in zip(good, who)]


def spread(xs):
    return {'median_s': round(statistics.median(xs), 4), 'min_s': round(min(xs), 4), 'max_s': round(max(xs), 4),
            'calls_s': [round(x, 4) for x in xs]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--msgs', type=int, default=500000)
    ap.add_argument('--len', type=int, default=200, dest='length', help='bytes of the message field')
    ap.add_argument('--reps', type=int, default=5)
    a = ap.parse_args()
    from pybitmessage_amd import addresses, receive, signatures
    objs, plains, ripes = make_inputs(a.msgs, a.length)
    want = leg_composition(objs, plains, ripes)  # warm-ups, and the comparison
    if rows_of_open(leg_open(objs, plains, ripes)) != want:
        raise SystemExit('open_msgs disagrees with the composition')
    receive.reset_stats()
    signatures.reset_stats()
    addresses.reset_stats()
    t_open, t_comp = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        got = leg_open(objs, plains, ripes)
        t_open.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        ref = leg_composition(objs, plains, ripes)
        t_comp.append(time.perf_counter() - t0)
        if ref != want or got[1] != [r[0] for r in want]:
            raise SystemExit('a timed call disagrees with the warm-up')
    rx, sg, idn = receive.stats(), signatures.stats(), addresses.stats()
    per = lambda v: round(v / a.reps, 3)  # noqa: E731
    diff = statistics.median(t_comp) - statistics.median(t_open)
    out = {'msgs': a.msgs, 'len': a.length, 'plaintext_bytes': len(plains[0]), 'accepted': len(want), 'reps': a.reps,
           'open_msgs': dict(spread(t_open), msgs_per_s=round(a.msgs / statistics.median(t_open))),
           'composition': dict(spread(t_comp), msgs_per_s=round(a.msgs / statistics.median(t_comp))),
           'composition_spread_s': round(max(t_comp) - min(t_comp), 4), 'median_difference_s': round(diff, 4),
           'difference_exceeds_spread': abs(diff) > max(t_comp) - min(t_comp),
           'open_msgs_device_ms': {k: per(rx[k]) for k in ('walk_ms', 'hash_ms', 'scalar_ms', 'curve_ms', 'ident_ms',
                                                           'finish_ms', 'host_ms')},
           'composition_device_ms': {'hash_ms': per(sg['hash_ms']), 'scalar_ms': per(sg['scalar_ms']),
                                     'curve_ms': per(sg['curve_ms']), 'sig_host_ms': per(sg['host_ms']),
                                     'ident_ms': per(idn['kernel_ms']), 'ident_host_ms': per(idn['host_ms'])},
           'sets_per_call': rx['sets'] // a.reps}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
