#!/usr/bin/env python3
"""Rate of the packet framing (bmpow_packets_batch) beside the composition it replaces.

    python tools/packets_rate.py --objects 500000 --out profiles/packets/rate_n500000.json

The workload is tools/intake_rate.py's flood (the intake leg's size mix: half acks of 54 B, a quarter
pubkey-size objects of 208 B, a quarter msgs of 0.5 - 16 KB) as ``object`` packets dealt round-robin to 64
connection buffers, a few ``inv`` packets of 50,000 hashes among them, and one object in a thousand with a
spoiled checksum -- each of those at the end of its buffer's share so far, where the buffer is cut off: the
reference closes the connection there, and a read buffer holds nothing behind it.

Two sides, in one process, taking turns, --reps calls each after a warm-up call of each:

* ``packets.check_buffers`` on the 64 buffers;
* a Python loop over every buffer -- ``struct.unpack`` of the header, the magic, the length,
  ``hashlib.sha512(payload).digest()[:4]`` against the checksum, the command -- that collects the payloads of
  the valid ``object`` packets, then ``intake.check_objects`` on those slices.

Before any time is reported the two sides' results are asserted identical: the same packets in the same order
with the same checksums and verdicts, the same connections closed at the same offsets, and byte-equal intake
records.  Reported: median and spread (min, max) of the wall time per side, the library's own split of either
(``bmpow_packets_get_stats``, ``bmpow_intake_get_stats``) -- ``host_build_ms`` of both is the number that says
whether packing on the device beats the host's padding pass -- and the share of the composition's time spent in
its Python loop.  No threshold is applied.  Fails without a GPU: there is no fallback."""
import argparse
import hashlib
import json
import os
import statistics
import struct
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from intake_rate import NOW, flood  # noqa: E402

HEADER = struct.Struct('!L12sL4s')
CONNECTIONS = 64


def packet(command, payload, spoil=False):
    checksum = hashlib.sha512(payload).digest()[:4]
    if spoil:
        checksum = bytes([checksum[0] ^ 1]) + checksum[1:]
    return HEADER.pack(0xE9BEB4D9, command, len(payload), checksum) + payload


def buffers_of(objs, seed=20250412):
    """64 read buffers; a spoiled packet ends its buffer (what follows goes to a buffer of its own turn)."""
    import random
    rng = random.Random(seed)
    parts = [[] for _ in range(CONNECTIONS)]
    closed = [False] * CONNECTIONS
    spoiled = invs = 0
    for i, o in enumerate(objs):
        c = i % CONNECTIONS
        if closed[c]:
            c = next((k for k in range(CONNECTIONS) if not closed[k]), None)
            if c is None:
                break
        if i % 100000 == 50000:
            parts[c].append(packet(b'inv', b'\xfd\xc3\x50' + rng.randbytes(32 * 50000)))
            invs += 1
        spoil = i % 1000 == 999 and spoiled < CONNECTIONS // 2
        parts[c].append(packet(b'object', o, spoil))
        if spoil:
            closed[c] = True
            spoiled += 1
    return [b''.join(p) for p in parts], spoiled, invs


def composition(bufs):
    """The loop a user of the library writes today, then intake.check_objects on the slices."""
    from pybitmessage_amd import intake
    sha = hashlib.sha512
    unpack = HEADER.unpack_from
    rows, conns, slices = [], [], []
    t0 = time.perf_counter()
    for c, buf in enumerate(bufs):
        view = memoryview(buf)
        at, n, close = 0, len(buf), 0
        while n - at >= 24:
            magic, command, length, checksum = unpack(buf, at)
            if magic != 0xE9BEB4D9:
                close = 1
                break
            if n - at - 24 < length:
                break
            payload = view[at + 24:at + 24 + length]
            computed = sha(payload).digest()[:4] if length <= 1600100 else b'\x00' * 4
            bad = (1 if length > 1600100 else 0) | (2 if length <= 1600100 and computed != checksum else 0)
            is_object = command.rstrip(b'\x00').lower() == b'object'
            rows.append((c, at, length, computed, bad, is_object))
            if bad:
                close = 2
                break
            if is_object:
                slices.append(bytes(payload))
            at += 24 + length
        conns.append((at, close))
    t1 = time.perf_counter()
    res = intake.check_objects(slices, now=NOW)
    return rows, conns, res, (t1 - t0) * 1e3


def assert_identical(res, rows, conns, ires):
    from pybitmessage_amd import packets
    assert len(res) == len(rows), (len(res), len(rows))
    assert res.conn.tolist() == [r[0] for r in rows] and res.offset.tolist() == [r[1] for r in rows]
    assert res.length.tolist() == [r[2] for r in rows]
    assert res.computed.tolist() == [struct.unpack('>I', r[3])[0] for r in rows]
    assert res.status.tolist() == [r[4] for r in rows]
    assert [(int(a), int(b)) for a, b in zip(res.consumed, res.close)] == conns
    import numpy as np
    valid = np.flatnonzero((res.command == packets.OBJECT) & (res.status == packets.OK))
    assert len(valid) == len(ires) == sum(1 for r in rows if r[5] and not r[4])
    assert res.records['intake'][valid].tobytes() == ires.records.tobytes()


def summary(values):
    return {'median': round(statistics.median(values), 2), 'min': round(min(values), 2), 'max': round(max(values), 2)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--objects', type=int, default=500000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', help='also write the JSON line to this file')
    a = ap.parse_args()
    from pybitmessage_amd import _lib, intake, packets
    lib = _lib.get()  # raises without a device
    bufs, spoiled, invs = buffers_of(flood(a.objects))
    res = packets.check_buffers(bufs, now=NOW)  # warm-up of either side, and the comparison
    rows, conns, ires, _ = composition(bufs)
    assert_identical(res, rows, conns, ires)
    new, old, loop, psplit, isplit = [], [], [], [], []
    for _ in range(a.reps):
        packets.reset_stats()
        t0 = time.perf_counter()
        res = packets.check_buffers(bufs, now=NOW)
        new.append((time.perf_counter() - t0) * 1e3)
        psplit.append(packets.stats())
        intake.reset_stats()
        t0 = time.perf_counter()
        rows, conns, ires, loop_ms = composition(bufs)
        old.append((time.perf_counter() - t0) * 1e3)
        loop.append(loop_ms)
        isplit.append(intake.stats())
        assert_identical(res, rows, conns, ires)

    def med(stats, key):
        return round(statistics.median(s[key] for s in stats), 3)
    pkeys = ('pack_ms', 'object_ms', 'sum_ms', 'host_frame_ms', 'host_build_ms', 'host_run_ms', 'host_status_ms')
    ikeys = ('kernel_ms', 'host_build_ms', 'host_run_ms', 'host_status_ms')
    out = {'library': lib.bmpow_version().decode(), 'objects': a.objects, 'connections': CONNECTIONS, 'packets': len(res),
           'bytes': sum(map(len, bufs)), 'spoiled': spoiled, 'inv_packets': invs, 'reps': a.reps,
           'identical': True,
           'check_buffers_ms': summary(new), 'composition_ms': summary(old), 'composition_python_loop_ms': summary(loop),
           'packets_stats_median': dict({k: med(psplit, k) for k in pkeys},
                                        **{k: int(psplit[-1][k]) for k in ('packets', 'object_rows', 'sum_rows', 'host_rows',
                                                                            'empty_rows', 'blocks')}),
           'intake_stats_median': {k: med(isplit, k) for k in ikeys},
           'host_build_ms': {'packets_pack_on_device': med(psplit, 'host_build_ms'),
                             'intake_pad_on_host': med(isplit, 'host_build_ms')}}
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
