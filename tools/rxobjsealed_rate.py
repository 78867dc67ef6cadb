#!/usr/bin/env python3
"""Rate of the one-call opening of received broadcasts (receive.open_sealed_broadcasts, bmpow_rx_sealed_objects)
beside the composition it replaces (receive.open_broadcasts: one bmpow_rx_walk_object per object, one
bmpow_ecies_match + bmpow_aes256_cbc per distinct key, then bmpow_rx_objects), in one process, taking turns.

    python tools/rxobjsealed_rate.py --objects 200000 --len 200 --tags 10 --mine 1.0
    python tools/rxobjsealed_rate.py --objects 200000 --len 2000 --tags 1000 --mine 0.01

N v5 broadcasts as they come off the wire, whose message field is L bytes (v4 senders, stream 1), signed
(``sender.sign_batch``) and sealed (``sender.encrypt_batch``) on the device to the key their sender's address gives.
The user is subscribed to T v4 addresses; a fraction --mine of the objects comes from one of them, the rest from
senders the user is not subscribed to (their tags are in nobody's table, so neither leg tries a key on them).  One
in a thousand of the subscribed ones has a byte of its message altered.  The N cycle through 4,096 distinct
objects.

Each leg is warmed once with the same inputs; then the legs alternate for --reps timed calls each, and the records
and plaintexts are asserted identical.  A difference between the legs counts when it exceeds the spread
(max - min) of the composition's own calls.  Prints one JSON line (and writes it to --out).  Without a device it
raises (there is no fallback)."""
import argparse
import json
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DISTINCT = 4096


def make_inputs(n, length, tags, mine, seed=20261021):
    from pybitmessage_amd import addresses, ecies, sender
    from pybitmessage_amd.addressgen import encodeVarint as ev
    rng = random.Random(seed)
    key = lambda: rng.getrandbits(255).to_bytes(32, 'big')  # noqa: E731
    n_senders = 2 * tags  # the first half is subscribed to
    privs = [key() for _ in range(2 * n_senders)]
    pubs = sender.priv_to_pub(privs)
    sign, enc = [p[1:] for p in pubs[0::2]], [p[1:] for p in pubs[1::2]]
    ident = addresses.derive_batch(sign, enc, [4] * n_senders, [1] * n_senders)
    addrs = [ident.address(i) for i in range(n_senders)]
    addr_privs = [ecies._key32(k[5]) for k in addresses.address_keys(addrs)]
    addr_pubs = [p[1:] for p in sender.priv_to_pub(addr_privs)]
    distinct = min(n, DISTINCT)
    every = max(1, int(round(1 / mine))) if mine > 0 else 0
    heads, bodies, who = [], [], []
    for i in range(distinct):
        k = i % tags if every and i % every == 0 else tags + i % tags
        who.append(k)
        heads.append(rng.getrandbits(128).to_bytes(16, 'big') + b'\x00\x00\x00\x03' + ev(5) + ev(1) + ident.tag[k].tobytes())
        message = rng.getrandbits(8 * length).to_bytes(length, 'big') if length else b''
        bodies.append(ev(4) + ev(1) + b'\x00\x00\x00\x01' + sign[k] + enc[k] + ev(1000) + ev(1000) + ev(2) + ev(length) + message)
    sigs = sender.sign_batch([h[8:] + b for h, b in zip(heads, bodies)], [privs[2 * k] for k in who])
    plains = []
    for i, (b, s) in enumerate(zip(bodies, sigs)):
        if i % 1000 == 999 and length:
            b = b[:-1] + bytes([b[-1] ^ 1])
        plains.append(b + ev(len(s)) + s)
    blobs = sender.encrypt_batch(plains, [addr_pubs[k] for k in who], ephemeral=[key() for _ in range(distinct)],
                                 ivs=[rng.getrandbits(128).to_bytes(16, 'big') for _ in range(distinct)])
    objs = [h + b for h, b in zip(heads, blobs)]
    reps = (n + distinct - 1) // distinct
    return (objs * reps)[:n], addrs[:tags], len(plains[0])


def spread(xs):
    return {'median_s': round(statistics.median(xs), 4), 'min_s': round(min(xs), 4), 'max_s': round(max(xs), 4),
            'calls_s': [round(x, 4) for x in xs]}


def same(a, b):
    return a.recs.tobytes() == b.recs.tobytes() and list(a.plaintexts) == list(b.plaintexts)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--objects', type=int, default=200000)
    ap.add_argument('--len', type=int, default=200, dest='length', help='bytes of the message field')
    ap.add_argument('--tags', type=int, default=10, help='v4 addresses the user is subscribed to')
    ap.add_argument('--mine', type=float, default=1.0, help='fraction of the objects that come from a subscribed address')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', help='also write the JSON line to this file')
    a = ap.parse_args()
    from pybitmessage_amd import receive
    objs, subs, plain_len = make_inputs(a.objects, a.length, a.tags, a.mine)
    want = receive.open_broadcasts(objs, subs)  # warm-ups, and the comparison
    if not same(receive.open_sealed_broadcasts(objs, subs), want):
        raise SystemExit('open_sealed_broadcasts disagrees with the composition')
    receive.sealed_obj_reset_stats()
    receive.obj_reset_stats()
    t_one, t_comp = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        got = receive.open_sealed_broadcasts(objs, subs)
        t_one.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        ref = receive.open_broadcasts(objs, subs)
        t_comp.append(time.perf_counter() - t0)
        if not same(ref, want) or not same(got, want):
            raise SystemExit('a timed call disagrees with the warm-up')
    st, rx = receive.sealed_obj_stats(), receive.obj_stats()
    per = lambda v: round(v / a.reps, 3)  # noqa: E731
    diff = statistics.median(t_comp) - statistics.median(t_one)
    out = {'objects': a.objects, 'len': a.length, 'tags': a.tags, 'mine': a.mine, 'plaintext_bytes': plain_len,
           'object_bytes': len(objs[0]), 'matched_per_call': st['matched'] // a.reps, 'accepted': len(want.accepted()),
           'reps': a.reps,
           'one_call': dict(spread(t_one), objects_per_s=round(a.objects / statistics.median(t_one))),
           'composition': dict(spread(t_comp), objects_per_s=round(a.objects / statistics.median(t_comp))),
           'composition_spread_s': round(max(t_comp) - min(t_comp), 4), 'median_difference_s': round(diff, 4),
           'difference_exceeds_spread': abs(diff) > max(t_comp) - min(t_comp),
           'one_call_device_ms': {k: per(st[k]) for k in ('match_ms', 'open_ms', 'walk_ms', 'hash_ms', 'scalar_ms', 'curve_ms',
                                                          'ident_ms', 'finish_ms', 'host_ms')},
           'one_call_bytes': {'up': st['bytes_up'] // a.reps, 'down': st['bytes_down'] // a.reps, 'objects': sum(map(len, objs))},
           'one_call_launches': st['launches'] // a.reps, 'sets_per_call': st['sets'] // a.reps,
           'tagged_tries_per_call': st['tagged_tries'] // a.reps,
           'composition_rx_objects': {'calls': rx['calls'] // a.reps, 'walk_ms': per(rx['walk_ms']), 'hash_ms': per(rx['hash_ms']),
                                      'scalar_ms': per(rx['scalar_ms']), 'curve_ms': per(rx['curve_ms']),
                                      'ident_ms': per(rx['ident_ms']), 'finish_ms': per(rx['finish_ms']),
                                      'host_ms': per(rx['host_ms'])}}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
