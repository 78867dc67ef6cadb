#!/usr/bin/env python3
"""Rate of the one-call assembly of outgoing msgs (outgoing.build_objects, bmpow_tx_objects) beside the
composition of calls it replaces, in one process, taking turns.

    python tools/tx_rate.py --msgs 500000 --len 200

N msgs whose body is L bytes under a 14-byte head, to 64 recipient keys under 64 signing keys, with fixed
nonces, ephemeral keys and IVs, so that both legs make the same bytes.  The N cycle through 4,096 distinct
bodies; both legs sign, encrypt and hash every one of the N on its own.

* ``build_objects``: one ``outgoing.build_objects`` call; the payloads and ``initialHash`` values are read
  out of its result.
* ``composition``: what the library offered before: ``head + body`` per object, ``sender.sign_batch``,
  ``body + varint + signature`` per object, ``sender.encrypt_batch``, ``head + blob`` per object and
  ``hashlib.sha512`` over every payload.

Each leg is warmed once with the same inputs and the outputs are asserted byte-identical; then the legs
alternate for --reps timed calls each.  A difference between the legs counts when it exceeds the spread
(max - min) of the composition's own calls.  The device time of the phases comes from the library's events
(``bmpow_tx_get_stats`` / ``bmpow_send_get_stats`` / ``bmpow_seal_get_stats``).  Prints one JSON line and
writes it to --out (default profiles/tx/rate_n<N>_l<L>.json).  Without a device it raises (there is no
fallback)."""
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


def make_inputs(n, length, seed=20261020):
    from pybitmessage_amd import outgoing, sender
    rng = random.Random(seed)
    privs = [rng.getrandbits(255).to_bytes(32, 'big') for _ in range(KEYS)]
    recips = sender.priv_to_pub([rng.getrandbits(255).to_bytes(32, 'big') for _ in range(KEYS)])
    head = outgoing.msg_head(1790000000, 1)
    m = min(n, DISTINCT)
    bodies = [rng.getrandbits(8 * length).to_bytes(length, 'big') if length else b'' for _ in range(m)]
    reps = (n + m - 1) // m
    rand = lambda bits, size: [(rng.getrandbits(bits) | 1).to_bytes(size, 'big') for _ in range(n)]  # noqa: E731
    return {'heads': [head] * n, 'bodies': (bodies * reps)[:n], 'privs': [privs[i % KEYS] for i in range(n)],
            'pubs': [recips[(i // 7) % KEYS] for i in range(n)], 'nonces': rand(255, 32), 'ephemeral': rand(255, 32),
            'ivs': rand(128, 16)}


def leg_build(x):
    from pybitmessage_amd import outgoing
    n = len(x['heads'])
    built = outgoing.build_objects([outgoing.SEALED] * n, x['heads'], x['bodies'], x['privs'], x['pubs'], 'sha256', x['nonces'],
                                   x['ephemeral'], x['ivs'])
    hashes = built.recs['initial_hash']
    return [built.payload(i) for i in range(n)], [hashes[i].tobytes() for i in range(n)]


def leg_composition(x):
    from pybitmessage_amd import sender
    from pybitmessage_amd.worker import _varint
    sigs = sender.sign_batch([h + b for h, b in zip(x['heads'], x['bodies'])], x['privs'], 'sha256', x['nonces'])
    blobs = sender.encrypt_batch([b + _varint(len(s)) + s for b, s in zip(x['bodies'], sigs)], x['pubs'], x['ephemeral'],
                                 x['ivs'])
    payloads = [h + blob for h, blob in zip(x['heads'], blobs)]
    return payloads, [hashlib.sha512(p).digest() for p in payloads]


def spread(xs):
    return {'median_s': round(statistics.median(xs), 4), 'min_s': round(min(xs), 4), 'max_s': round(max(xs), 4),
            'calls_s': [round(v, 4) for v in xs]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--msgs', type=int, default=500000)
    ap.add_argument('--len', type=int, default=200, dest='length', help='bytes of the body')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from pybitmessage_amd import outgoing, sender
    x = make_inputs(a.msgs, a.length)
    want = leg_composition(x)  # warm-ups, and the comparison
    if leg_build(x) != want:
        raise SystemExit('build_objects disagrees with the composition')
    outgoing.reset_stats()
    sender.reset_stats()
    sender.reset_seal_stats()
    t_build, t_comp = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        got = leg_build(x)
        t_build.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        ref = leg_composition(x)
        t_comp.append(time.perf_counter() - t0)
        if ref != want or got != want:
            raise SystemExit('a timed call disagrees with the warm-up')
    tx, sd, sl = outgoing.stats(), sender.stats(), sender.seal_stats()
    per = lambda v: round(v / a.reps, 3)  # noqa: E731
    diff = statistics.median(t_comp) - statistics.median(t_build)
    out = {'msgs': a.msgs, 'len': a.length, 'payload_bytes': len(want[0][0]), 'reps': a.reps, 'identical': True,
           'build_objects': dict(spread(t_build), msgs_per_s=round(a.msgs / statistics.median(t_build))),
           'composition': dict(spread(t_comp), msgs_per_s=round(a.msgs / statistics.median(t_comp))),
           'composition_spread_s': round(max(t_comp) - min(t_comp), 4), 'median_difference_s': round(diff, 4),
           'difference_exceeds_spread': abs(diff) > max(t_comp) - min(t_comp),
           'build_objects_device_ms': {k: per(tx[k]) for k in ('pack_ms', 'hash_ms', 'sign_ms', 'ladder_ms', 'seal_ms',
                                                               'finish_ms', 'host_ms')},
           'composition_device_ms': {'hash_ms': per(sd['hash_ms']), 'comb_ms': per(sd['comb_ms']),
                                     'scalar_ms': per(sd['scalar_ms']), 'ladder_ms': per(sd['ladder_ms']),
                                     'seal_kernel_ms': per(sl['seal_kernel_ms']), 'send_host_ms': per(sd['host_ms'])},
           'sets_per_call': tx['sets'] // a.reps, 'launches_per_call': tx['launches'] // a.reps}
    line = json.dumps(out)
    print(line)
    path = a.out or os.path.join(ROOT, 'profiles', 'tx', 'rate_n%d_l%d.json' % (a.msgs, a.length))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
