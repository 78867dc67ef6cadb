#!/usr/bin/env python3
"""Rate of the object processor's dispatch (processor.Dispatcher.dispatch) beside the composition it replaces.

    python tools/proc_rate.py --objects 500000 --out profiles/proc/rate_n500000.json

The workload is a flood as a node's objectProcessorQueue sees it, seeded: of every 20 objects 10 are 54-byte acks
(msgs), 6 are msgs of 300 - 2,000 bytes, 2 are pubkey-size objects of 208 bytes, 1 is a getpubkey (every tenth
of them for one of my 20 addresses, the others for strangers, a few malformed) and 1 is a broadcast -- every
fiftieth of those an onionpeer instead.  1,000 ack keys are watched; 1,200 of the acks carry one of them, so 200
are repeats the reference has deleted the key for by then.

The composition is the reference's loop written in plain Python here: ``checkackdata`` over a ``dict``,
``processgetpubkey`` over two address dicts and ``processonion`` with ``checkIPAddress``'s classes, statement by
statement (src/class_objectProcessor.py:129-268, src/protocol.py:150-227), with ``struct`` for the varints.

Both run in one process taking turns, --reps calls each after a warm-up call of each; every turn starts from the
same watched keys (re-added outside the timed part).  Before any time is reported the two sides' answers are
asserted identical: the ack verdict (FOUND_EARLIER is the reference's "not bound for me"), the status and the
address row of every object.  Reported: median and spread (min, max) of the wall time per side, the dispatcher's
own counters -- kernel ms per launch kind, rows and bytes uploaded -- and whether the gain exceeds the spread.  No
threshold is applied.  Fails without a GPU: there is no fallback."""
import argparse
import json
import os
import random
import statistics
import struct
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SEED = 20251021
NOW = 1700000000
WATCHED, CARRIED, ADDRESSES = 1000, 1200, 20
MAPPED = bytes(10) + b'\xff\xff'
ONION_PREFIX = bytes.fromhex('fd87d87eeb43')


def varint(v):
    if v < 253:
        return struct.pack('>B', v)
    if v < 65536:
        return b'\xfd' + struct.pack('>H', v)
    if v < 4294967296:
        return b'\xfe' + struct.pack('>I', v)
    return b'\xff' + struct.pack('>Q', v)


def workload(n, seed=SEED):
    """(objects, types, watched keys, address tuples)."""
    from pybitmessage_amd import processor as P
    rng = random.Random(seed)
    mine = [(3 if k % 2 else 4, 1, rng.randbytes(20), k == 7, NOW - 3000000 if k != 9 else NOW - 5) for k in range(ADDRESSES)]
    keys = [rng.randbytes(38) for _ in range(WATCHED)]
    objs, types, ack_at = [], [], []
    head = lambda t: rng.randbytes(8) + (NOW + 345600).to_bytes(8, 'big') + (t & 0xffffffff).to_bytes(4, 'big')  # noqa: E731
    for i in range(n):
        r = i % 20
        if r < 10:
            ack_at.append(i)
            objs.append(rng.randbytes(54)), types.append(P.OBJECT_MSG)
        elif r < 16:
            objs.append(head(2) + b'\x01\x01' + rng.randbytes(rng.randrange(278, 1978))), types.append(P.OBJECT_MSG)
        elif r < 18:
            objs.append(head(1) + b'\x04\x01' + rng.randbytes(186)), types.append(P.OBJECT_PUBKEY)
        elif r == 18:
            k = i // 20
            if k % 10 == 0:
                version, stream, ripe = mine[(k // 10) % ADDRESSES][:3]
                want = ripe if version == 3 else P.tag_of(version, stream, ripe)
            else:
                version, want = (3, rng.randbytes(20)) if k % 2 else (4, rng.randbytes(32))
            body = varint(version) + varint(1 if k % 7 else 2) + want
            if k % 97 == 0:
                body = b'\xfd\x00\x03' + body[1:]
            if k % 89 == 0:
                body = body[:-3]
            objs.append(head(0) + body), types.append(P.OBJECT_GETPUBKEY)
        elif (i // 20) % 50 == 0:
            k = i // 1000
            host = [MAPPED + bytes([8 + k % 200, 8, 4, 4]), MAPPED + b'\x0a\x01\x02\x03', ONION_PREFIX + rng.randbytes(10),
                    rng.randbytes(16), b'\xfe\x80' + rng.randbytes(14), MAPPED + b'\x01\x02\x03'][k % 6]
            objs.append(head(P.OBJECT_ONIONPEER) + varint(3) + varint(1) + varint(8444 + k % 3 * 70000) + host)
            types.append(P.OBJECT_ONIONPEER)
        else:
            objs.append(head(3) + b'\x05\x01' + rng.randbytes(300)), types.append(P.OBJECT_BROADCAST)
    for j, i in enumerate(rng.sample(ack_at, min(CARRIED, len(ack_at)))):
        objs[i] = objs[i][:16] + keys[j % WATCHED]
    return objs, types, keys, mine


def decode_varint(data):
    """addresses.decodeVarint with struct; None for varintDecodeError."""
    if not data:
        return 0, 0
    first = data[0]
    if first < 253:
        return first, 1
    need, fmt, least = {253: (3, '>H', 253), 254: (5, '>I', 65536), 255: (9, '>Q', 4294967296)}[first]
    if len(data) < need:
        return None
    value, = struct.unpack(fmt, data[1:need])
    return None if value < least else (value, need)


def py_getpubkey(data, by_hash, by_tag, rows, now, P):
    if len(data) > 200:
        return P.TOO_LONG, P.NO_ROW
    at = 20
    v = decode_varint(data[at:at + 10])
    if v is None:
        return P.MALFORMED, P.NO_ROW
    version, used = v
    at += used
    v = decode_varint(data[at:at + 10])
    if v is None:
        return P.MALFORMED, P.NO_ROW
    stream, used = v
    at += used
    if version == 0:
        return P.VERSION_ZERO, P.NO_ROW
    if version == 1:
        return P.VERSION_ONE, P.NO_ROW
    if version > 4:
        return P.VERSION_TOO_HIGH, P.NO_ROW
    row = None
    if version <= 3:
        want = data[at:at + 20]
        if len(want) != 20:
            return P.SHORT_HASH, P.NO_ROW
        if want in by_hash:
            row = by_hash[want]
    else:
        want = data[at:at + 32]
        if len(want) != 32:
            return P.SHORT_TAG, P.NO_ROW
        if want in by_tag:
            row = by_tag[want]
    if row is None:
        return P.NOT_MINE, P.NO_ROW
    my_version, my_stream, _, chan, last = rows[row]
    if my_version != version:
        return P.VERSION_MISMATCH, row
    if my_stream != stream:
        return P.STREAM_MISMATCH, row
    if chan:
        return P.CHAN, row
    if last > now - 2419200:
        return P.SENT_RECENTLY, row
    return {2: P.SEND_V2, 3: P.SEND_V3, 4: P.SEND_V4}[version], row


def py_onion(data, P):
    at = 20
    for _ in range(2):
        v = decode_varint(data[at:at + 10])
        if v is None:
            return P.MALFORMED
        at += v[1]
    v = decode_varint(data[at:at + 10])
    if v is None:
        return P.MALFORMED
    host = data[at + v[1]:]
    if host[0:12] == MAPPED:
        if len(host) != 16:
            return P.RAISES
        h = host[12:]
        if h[0:1] in (b'\x7f', b'\x0a') or h[0:2] == b'\xc0\xa8' or b'\xac\x10' <= h[0:2] < b'\xac\x20':
            return P.NO_HOST
        return P.PEER
    if host[0:6] == ONION_PREFIX:
        return P.PEER
    if len(host) != 16 or host == bytes(15) + b'\x01':
        return P.NO_HOST
    if (host[0] == 0xfe and host[1] & 0xc0 == 0x80) or host[0] & 0xfe == 0xfc:
        return P.NO_HOST
    return P.PEER


def loop(objs, types, watch, by_hash, by_tag, rows, now, P):
    """objectProcessor.run's own work per object: (ack, status, address row)."""
    ack, status, address = bytearray(), bytearray(), []
    for t, data in zip(types, objs):
        a = P.NOT_CHECKED
        if len(data) >= 32:
            tail = data[16:]
            if tail in watch:
                del watch[tail]
                a = P.FOUND
            else:
                a = P.NOT_WATCHED
        ack.append(a)
        if t == P.OBJECT_GETPUBKEY:
            s, row = py_getpubkey(data, by_hash, by_tag, rows, now, P)
        elif t == P.OBJECT_ONIONPEER:
            s, row = py_onion(data, P), P.NO_ROW
        else:
            s, row = P.NONE, P.NO_ROW
        status.append(s), address.append(row)
    return ack, status, address


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
    from pybitmessage_amd import _lib, processor as P
    lib = _lib.get()  # raises without a device
    objs, types, keys, mine = workload(a.objects)
    table = P.address_rows(mine)
    by_hash = {m[2]: i for i, m in enumerate(mine)}
    by_tag = {P.tag_of(m[0], m[1], m[2]): i for i, m in enumerate(mine)}
    kinds = np.array(types, dtype=np.uint32)
    new, old, stats = [], [], []
    with P.Dispatcher() as d:
        d.set_addresses(table)
        for rep in range(a.reps + 1):
            d.clear()
            d.watch(keys, aux=range(len(keys)))
            s0 = d.stats()
            t0 = time.perf_counter()
            got = d.dispatch(objs, kinds, now=NOW)
            t1 = time.perf_counter()
            s1 = d.stats()
            watch = dict.fromkeys(keys, 0)
            t2 = time.perf_counter()
            ack, status, address = loop(objs, types, watch, by_hash, by_tag, mine, NOW, P)
            t3 = time.perf_counter()
            mine_ack = np.where(got.ack == P.FOUND_EARLIER, P.NOT_WATCHED, got.ack).astype(np.uint8)
            assert (mine_ack == np.frombuffer(bytes(ack), dtype=np.uint8)).all()
            assert (got.status.astype(np.uint8) == np.frombuffer(bytes(status), dtype=np.uint8)).all()
            assert (got.address == np.array(address, dtype=np.uint32)).all()
            assert len(d) == len(watch)
            if rep == 0:  # the warm-up
                continue
            new.append((t1 - t0) * 1e3), old.append((t3 - t2) * 1e3)
            stats.append({k: s1[k] - s0[k] for k in ('rows_uploaded', 'ack_rows', 'bytes_uploaded', 'launches', 'found',
                                                     'table_uploads', 'rows_ms', 'finish_ms', 'host_ms')})
        counts = {name: int((got.status == getattr(P, name)).sum()) for name in
                  ('SEND_V3', 'SEND_V4', 'NOT_MINE', 'MALFORMED', 'STREAM_MISMATCH', 'CHAN', 'SENT_RECENTLY', 'PEER', 'NO_HOST',
                   'RAISES')}
        acks = {'found': int((got.ack == P.FOUND).sum()), 'found_earlier': int((got.ack == P.FOUND_EARLIER).sum())}

    def med(key, digits=3):
        return round(statistics.median(s[key] for s in stats), digits)
    out = {'library': lib.bmpow_version().decode(), 'objects': a.objects, 'object_bytes': sum(map(len, objs)),
           'watched': len(keys), 'addresses': len(mine), 'reps': a.reps, 'identical': True, 'acks': acks, 'statuses': counts,
           'dispatch_ms': summary(new), 'python_loop_ms': summary(old), 'verdict': verdict(new, old),
           'kernels_ms': {'rows': med('rows_ms'), 'ack_finish': med('finish_ms')}, 'library_ms': med('host_ms', 2),
           'rows_uploaded': int(med('rows_uploaded')), 'ack_rows': int(med('ack_rows')),
           'bytes_uploaded': int(med('bytes_uploaded')), 'launches': int(med('launches')),
           'table_uploads': int(med('table_uploads'))}
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
