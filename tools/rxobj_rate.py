#!/usr/bin/env python3
"""Rate of the one-call broadcast and pubkey processing (receive.open_objects, bmpow_rx_objects) beside the
composition of calls it replaces, in one process, taking turns.

    python tools/rxobj_rate.py --kind broadcast --rows 500000 --len 200
    python tools/rxobj_rate.py --kind pubkey --rows 500000

``broadcast``: N decrypted v5 broadcasts whose message is L bytes (v4 senders, stream 1), signed on the device
under SHA-256; one in a thousand has a byte of its message altered.  ``pubkey``: N clear v3 pubkeys; one in a
thousand has a byte of its encryption key altered.  The N cycle through 4,096 distinct objects under 64 sender
keys; both legs parse, hash and verify every one of the N on its own.

* ``open_objects``: one ``receive.open_objects`` call and ``accepted()``.
* ``composition``: what the library offered before.  Broadcasts: ``signatures.broadcast_signed_parts`` per
  object, ``signatures.verify_batch_digest``, ``addresses.derive_batch``, the tag comparison in Python, hashlib
  for ``sigHash`` (the body of ``receive.process_broadcasts`` behind its decryption).  Pubkeys:
  ``signatures.pubkey_v3_signed_parts`` per object, ``verify_batch_digest``, ``receive.identify``.

Each leg is warmed once with the same inputs; then the legs alternate for --reps timed calls each, and the
results (accepted rows, digest, fromAddress, ripe, sigHash) are asserted identical.  A difference between the
legs counts when it exceeds the spread (max - min) of the composition's own calls.  The device time of the
phases comes from the library's events.  Prints one JSON line and writes it to --out (default
profiles/rxobj/rate_<kind>_n<rows>[_l<len>].json).  Without a device it raises (there is no fallback)."""
import argparse
import hashlib
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DISTINCT = 4096
KEYS = 64
BROADCAST, PUBKEY = 0, 2  # receive.KIND_*


def make_inputs(kind, n, length, seed=20251025):
    from pybitmessage_amd import addresses, sender
    from pybitmessage_amd.addressgen import encodeVarint as ev
    rng = random.Random(seed)
    privs = [rng.getrandbits(255).to_bytes(32, 'big') for _ in range(2 * KEYS)]
    pubs = sender.priv_to_pub(privs)
    tags = addresses.derive_batch([pubs[2 * k][1:] for k in range(KEYS)], [pubs[2 * k + 1][1:] for k in range(KEYS)],
                                  [4] * KEYS, [1] * KEYS).tag
    heads, bodies = [], []
    for i in range(min(n, DISTINCT)):
        k = i % KEYS
        keys = b'\x00\x00\x00\x01' + pubs[2 * k][1:] + pubs[2 * k + 1][1:] + ev(1000) + ev(1000)
        head = rng.getrandbits(128).to_bytes(16, 'big')
        if kind == BROADCAST:
            message = rng.getrandbits(8 * length).to_bytes(length, 'big') if length else b''
            heads.append(head + b'\x00\x00\x00\x03' + ev(5) + ev(1) + tags[k].tobytes())
            bodies.append(ev(4) + ev(1) + keys + ev(2) + ev(length) + message)
        else:
            heads.append(head + b'\x00\x00\x00\x01' + ev(3) + ev(1))
            bodies.append(keys)
    sigs = sender.sign_batch([h[8:] + b for h, b in zip(heads, bodies)], [privs[2 * (i % KEYS)] for i in range(len(heads))])
    objs, plains = [], []
    for i, (h, b, s) in enumerate(zip(heads, bodies, sigs)):
        if i % 1000 == 999 and (length or kind == PUBKEY):
            at = len(b) - 1 if kind == BROADCAST else 4 + 64 + 7  # the message's last byte; inside the encryption key
            b = b[:at] + bytes([b[at] ^ 1]) + b[at + 1:]
        if kind == BROADCAST:
            objs.append(h + b'the encrypted payload')
            plains.append(b + ev(len(s)) + s)
        else:
            objs.append(h + b + ev(len(s)) + s)
            plains.append(None)
    reps = (n + len(objs) - 1) // len(objs)
    return (objs * reps)[:n], (plains * reps)[:n]


def leg_open(kind, objs, plains):
    from pybitmessage_amd import receive
    res = receive.open_objects(bytes([kind]) * len(objs), objs, plains, [None] * len(objs))
    return res, res.accepted()


def rows_of_open(kind, out):
    res, accepted = out
    return [(i, int(res.digest[i]), res.fromAddress(i), res.ripe(i), res.sigHash(i) if kind == BROADCAST else None)
            for i in accepted]


def leg_composition(kind, objs, plains):
    from pybitmessage_amd import addresses, receive, signatures
    if kind == PUBKEY:
        parts = [signatures.pubkey_v3_signed_parts(o) for o in objs]
        live = [i for i, p in enumerate(parts) if p is not None]
        verdicts = signatures.verify_batch_digest([parts[i][0] for i in live], [parts[i][1] for i in live],
                                                  [parts[i][2] for i in live])
        good = [(i, v) for i, v in zip(live, verdicts) if v]
        who = receive.identify([parts[i] for i, _ in good], [3] * len(good), [1] * len(good))
        return [(i, v, address, ripe, None) for (i, v), (address, ripe) in zip(good, who)]
    parts = [signatures.broadcast_signed_parts(o, p) for o, p in zip(objs, plains)]
    heads = [signatures.broadcast_header(o) for o in objs]
    live = [i for i, p in enumerate(parts) if p is not None and len(p.pubSigningKey64) == 64 and len(p.pubEncryptionKey64) == 64]
    verdicts = signatures.verify_batch_digest([parts[i].signedData for i in live], [parts[i].signature for i in live],
                                              [parts[i].pubSigningKey64 for i in live])
    ident = addresses.derive_batch([parts[i].pubSigningKey64 for i in live], [parts[i].pubEncryptionKey64 for i in live],
                                   [parts[i].senderVersion for i in live], [parts[i].senderStream for i in live])
    out = []
    for j, i in enumerate(live):
        if verdicts[j] and ident.tag[j].tobytes() == heads[i][2]:
            out.append((i, verdicts[j], ident.address(j), ident.ripe[j].tobytes(),
                        hashlib.sha512(hashlib.sha512(parts[i].signature).digest()).digest()[32:]))
    return out


def spread(xs):
    return {'median_s': round(statistics.median(xs), 4), 'min_s': round(min(xs), 4), 'max_s': round(max(xs), 4),
            'calls_s': [round(x, 4) for x in xs]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--kind', choices=('broadcast', 'pubkey'), default='broadcast')
    ap.add_argument('--rows', type=int, default=500000)
    ap.add_argument('--len', type=int, default=200, dest='length', help='bytes of a broadcast\'s message')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from pybitmessage_amd import addresses, receive, signatures
    kind = BROADCAST if a.kind == 'broadcast' else PUBKEY
    objs, plains = make_inputs(kind, a.rows, a.length)
    want = leg_composition(kind, objs, plains)  # warm-ups, and the comparison
    if rows_of_open(kind, leg_open(kind, objs, plains)) != want:
        raise SystemExit('open_objects disagrees with the composition')
    receive.obj_reset_stats()
    signatures.reset_stats()
    addresses.reset_stats()
    t_open, t_comp = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        got = leg_open(kind, objs, plains)
        t_open.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        ref = leg_composition(kind, objs, plains)
        t_comp.append(time.perf_counter() - t0)
        if ref != want or got[1] != [r[0] for r in want]:
            raise SystemExit('a timed call disagrees with the warm-up')
    rx, sg, idn = receive.obj_stats(), signatures.stats(), addresses.stats()
    per = lambda v: round(v / a.reps, 3)  # noqa: E731
    diff = statistics.median(t_comp) - statistics.median(t_open)
    out = {'kind': a.kind, 'rows': a.rows, 'len': a.length if kind == BROADCAST else None,
           'source_bytes': len(plains[0] if kind == BROADCAST else objs[0]), 'accepted': len(want), 'reps': a.reps,
           'open_objects': dict(spread(t_open), rows_per_s=round(a.rows / statistics.median(t_open))),
           'composition': dict(spread(t_comp), rows_per_s=round(a.rows / statistics.median(t_comp))),
           'composition_spread_s': round(max(t_comp) - min(t_comp), 4), 'median_difference_s': round(diff, 4),
           'difference_exceeds_spread': abs(diff) > max(t_comp) - min(t_comp),
           'open_objects_device_ms': {k: per(rx[k]) for k in ('walk_ms', 'hash_ms', 'scalar_ms', 'curve_ms', 'ident_ms',
                                                              'finish_ms', 'host_ms')},
           'composition_device_ms': {'hash_ms': per(sg['hash_ms']), 'scalar_ms': per(sg['scalar_ms']),
                                     'curve_ms': per(sg['curve_ms']), 'sig_host_ms': per(sg['host_ms']),
                                     'ident_ms': per(idn['kernel_ms']), 'ident_host_ms': per(idn['host_ms'])},
           'sets_per_call': rx['sets'] // a.reps}
    line = json.dumps(out)
    print(line)
    name = 'rate_%s_n%d%s.json' % (a.kind, a.rows, '_l%d' % a.length if kind == BROADCAST else '')
    path = a.out or os.path.join(ROOT, 'profiles', 'rxobj', name)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
