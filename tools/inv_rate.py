#!/usr/bin/env python3
"""Rate of the device-resident inventory sets (inventory.check_invs, inventory.admit) beside the composition
they replace.

    python tools/inv_rate.py --objects 500000 --out profiles/inv/rate_n500000.json

The workload is tools/intake_rate.py's flood: its objects go through ``intake.check_objects`` once (their random
nonces solve no proof of work; a record that failed that check alone is taken as passed, for both sides), and
``have`` holds their inventory hashes.  64 connections then each announce 50,000 hashes in one ``inv`` packet: a fifth of
each packet are hashes we have, two fifths come from a pool every connection draws from (announced by several),
the rest are the connection's own.

Two legs, each against the composition it replaces, in one process, taking turns, --reps calls each after a
warm-up call of each:

* ``check_invs`` on the 64 payloads, against a Python loop that cuts 32 bytes at a time, tests a ``set`` for
  ``Inventory()`` and fills a ``dict`` for ``missingObjects`` (``_command_inv`` / ``handleReceivedInventory``);
* ``admit`` on the flood's intake records, against a Python loop over the same records with the same ``set``
  and ``dict`` (``checkAlreadyHave``, ``Inventory()[hash] = ...``, ``del missingObjects[hash]``).

Every turn starts from the same contents on both sides (the sets are cleared and refilled outside the timed
part), and before any time is reported the two sides' answers are asserted identical.  Reported: median and
spread (min, max) of the wall time per side, the sets' own counters -- kernel time per kernel, probes, the
longest probe seen -- and whether the gain exceeds the spread.  No threshold is applied.  Fails without a GPU:
there is no fallback."""
import argparse
import json
import os
import random
import statistics
import struct
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from intake_rate import NOW, flood  # noqa: E402

CONNECTIONS = 64
PER_PACKET = 50000
REACH = (0, 6, 7, 8)   # intake statuses behind checkAlreadyHave
STORED = (0, 8)        # ... and behind Inventory()[hash] = ...


def announcements(had, seed=20250620):
    """64 payloads of 50,000 hashes each: 10,000 we have, 20,000 from a pool of 100,000 shared among the
    connections, 20,000 of the connection's own; shuffled."""
    rng = random.Random(seed)
    pool = [rng.randbytes(32) for _ in range(100000)]
    out = []
    for _ in range(CONNECTIONS):
        items = rng.sample(had, min(10000, len(had))) + rng.sample(pool, 20000)
        items += [rng.randbytes(32) for _ in range(PER_PACKET - len(items))]
        rng.shuffle(items)
        out.append(b'\xfd' + struct.pack('>H', PER_PACKET) + b''.join(items))
    return out


def loop_invs(payloads, have, missing, now):
    """The loop a user of the library writes today: per item 0 = have, 1 = already missing, 2 = new."""
    states = bytearray()
    add = states.append
    for payload in payloads:
        count = struct.unpack_from('>H', payload, 1)[0]
        for at in range(3, 3 + 32 * count, 32):
            h = payload[at:at + 32]
            if h in have:
                add(0)
            elif h in missing:
                add(1)
            else:
                missing[h] = now
                add(2)
    return states


def loop_admit(status, raw, expires, stream, have, missing):
    """Per record: 0 = took no part, 1 = already had, 2 = looked up and not stored, 3 = stored."""
    out = bytearray()
    add = out.append
    for i, st in enumerate(status):
        if st not in REACH:
            add(0)
            continue
        h = raw[32 * i:32 * i + 32]
        missing.pop(h, None)
        if h in have:
            add(1)
        elif st in STORED:
            have[h] = (expires[i], stream[i])
            add(3)
        else:
            add(2)
    return out


def since(after, before):
    """One call's share of a set's counters: the times as differences, the rest as they stand after it."""
    return {k: v - before[k] if k.endswith('_ms') else v for k, v in after.items()}


def summary(values):
    return {'median': round(statistics.median(values), 2), 'min': round(min(values), 2), 'max': round(max(values), 2)}


def verdict(new, old):
    """Whether the medians differ by more than either side's spread."""
    gain = statistics.median(old) - statistics.median(new)
    spread = max(max(new) - min(new), max(old) - min(old))
    return {'gain_ms': round(gain, 2), 'spread_ms': round(spread, 2), 'gain_exceeds_spread': bool(abs(gain) > spread),
            'ratio': round(statistics.median(old) / statistics.median(new), 3)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--objects', type=int, default=500000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', help='also write the JSON line to this file')
    a = ap.parse_args()
    import numpy as np
    from pybitmessage_amd import _lib, intake, inventory
    lib = _lib.get()  # raises without a device
    res = intake.check_objects(flood(a.objects), now=NOW)
    # the flood's nonces are random: nobody solved 500,000 proofs of work for a benchmark.  A record that failed
    # that check alone is taken as passed here, for both sides, so that the legs see the flood's hashes.
    waived = res.status == intake.INSUFFICIENT_POW
    res.records['status'][waived] = intake.OK
    reach = np.isin(res.status, REACH)
    hashes = np.ascontiguousarray(res.inventoryHash[reach])
    raw_had = hashes.tobytes()
    had = sorted({raw_had[32 * i:32 * i + 32] for i in range(len(hashes))})
    payloads = announcements(had)
    have, missing = inventory.InventorySet(1 << 21), inventory.InventorySet(1 << 23)
    have_set = set(had)

    # ---- leg 1: check_invs ----
    have.add(hashes, expires=NOW + 1000, stream=1)
    new1, old1, stats1 = [], [], []
    for rep in range(a.reps + 1):
        missing.clear()
        s0 = (have.stats(), missing.stats())
        t0 = time.perf_counter()
        got = inventory.check_invs(payloads, inventory.INV, have, missing, NOW)
        t1 = time.perf_counter()
        s1 = (have.stats(), missing.stats())
        missing_dict = {}
        t2 = time.perf_counter()
        states = loop_invs(payloads, have_set, missing_dict, NOW)
        t3 = time.perf_counter()
        want = np.frombuffer(bytes(states), dtype=np.uint8)
        mine = np.select([got.item_state == inventory.HAVE, got.item_state == inventory.NEW], [0, 2], 1).astype(np.uint8)
        assert len(got) == len(want) == CONNECTIONS * PER_PACKET and (mine == want).all()
        assert np.isin(got.item_state, (inventory.HAVE, inventory.NEW, inventory.KNOWN, inventory.NEW_AGAIN)).all()
        assert len(missing) == len(missing_dict)
        if rep == 0:  # the warm-up, and the contents once
            listed = missing.unexpired_hashes_by_stream(0, 0)
            assert sorted(bytes(k) for k in listed) == sorted(missing_dict)
            continue
        new1.append((t1 - t0) * 1e3), old1.append((t3 - t2) * 1e3)
        stats1.append(tuple(since(x, y) for x, y in zip(s1, s0)))
    announced = len(missing)

    # ---- leg 2: admit ----
    everything = np.frombuffer(b''.join(sorted(missing_dict)), dtype=np.uint8).reshape(-1, 32)
    new2, old2, stats2 = [], [], []
    for rep in range(a.reps + 1):
        have.clear(), missing.clear()
        missing.add(everything, expires=NOW)
        missing.add(hashes, expires=NOW)
        s0 = (have.stats(), missing.stats())
        t0 = time.perf_counter()
        got = inventory.admit(res, have, missing)
        t1 = time.perf_counter()
        s1 = (have.stats(), missing.stats())
        have_dict, missing_dict2 = {}, dict.fromkeys(missing_dict, NOW)
        missing_dict2.update(dict.fromkeys(had, NOW))
        before = len(missing_dict2)
        t2 = time.perf_counter()
        out = loop_admit(res.status.tolist(), res.inventoryHash.tobytes(), res.expiresTime.tolist(),
                         res.streamNumber.tolist(), have_dict, missing_dict2)
        t3 = time.perf_counter()
        want = np.frombuffer(bytes(out), dtype=np.uint8)
        # a later copy inside the batch is DUP here and "already had" in the sequential loop
        mine = np.select([~reach, got.already | (got.state == inventory.DUP), got.state == inventory.ADDED], [0, 1, 3], 2)
        assert (mine.astype(np.uint8) == want).all()
        assert len(have) == len(have_dict) and len(missing) == len(missing_dict2) and before - len(missing_dict2) == len(had)
        if rep == 0:
            continue
        new2.append((t1 - t0) * 1e3), old2.append((t3 - t2) * 1e3)
        stats2.append(tuple(since(x, y) for x, y in zip(s1, s0)))

    def kernels(stats, which, keys):
        return {k: round(statistics.median(s[which][k] for s in stats), 3) for k in keys}
    out = {'library': lib.bmpow_version().decode(), 'objects': a.objects, 'have': len(had), 'connections': CONNECTIONS,
           'announced_hashes': CONNECTIONS * PER_PACKET, 'announced_distinct_new': announced,
           'payload_bytes': sum(map(len, payloads)), 'reps': a.reps, 'identical': True,
           'check_invs_ms': summary(new1), 'python_set_loop_ms': summary(old1), 'check_invs_verdict': verdict(new1, old1),
           'check_invs_kernels_ms': dict(kernels(stats1, 0, ('lookup_ms',)), **kernels(stats1, 1, ('claim_ms', 'finalize_ms'))),
           'admit_records': len(res), 'pow_waived': int(waived.sum()), 'admit_ms': summary(new2), 'python_dict_loop_ms': summary(old2),
           'admit_verdict': verdict(new2, old2),
           'admit_kernels_ms': dict(kernels(stats2, 0, ('lookup_ms', 'claim_ms', 'finalize_ms')),
                                    **{'missing_' + k: v for k, v in kernels(stats2, 1, ('lookup_ms', 'bury_ms')).items()}),
           'longest_probe': {'have': max(int(s[0]['longest_probe']) for s in stats1 + stats2),
                             'missing': max(int(s[1]['longest_probe']) for s in stats1 + stats2)},
           'slots': {'have': int(stats2[-1][0]['slots']), 'missing': int(stats1[-1][1]['slots'])}}
    have.close(), missing.close()
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
