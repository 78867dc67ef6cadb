"""Packet framing on the GPU: ``packets.check_buffers`` against hashlib for every payload length and source
alignment the pack can meet, against the reference-made fixture ``tests/golden/packet_kats.json``
(tests/golden/make_packet_golden.py) record for record, and against ``intake.check_objects`` -- the existing
path is the yardstick for the records of ``object`` packets; ``packets.check_acks`` against
``receive.ack_has_valid_header``.  Every malformed input here is a defined status: nothing provokes a fault."""
import hashlib
import random
import struct

import numpy as np
import pytest

from pybitmessage_amd import _lib, intake, packets, receive
from tests.golden.make_intake_golden import regen as regen_object
from tests.golden.make_packet_golden import regen_buffer

pytestmark = pytest.mark.gpu

NOW = 1700000000


def sum4(payload):
    return struct.unpack('>I', hashlib.sha512(payload).digest()[:4])[0]


def packet(command, payload, spoil=False):
    checksum = hashlib.sha512(payload).digest()[:4]
    if spoil:
        checksum = bytes([checksum[0] ^ 1]) + checksum[1:]
    return struct.pack('!L12sL4s', 0xE9BEB4D9, command, len(payload), checksum) + payload


def object_bytes(rng, length):
    """An object of ``length`` bytes whose header decodes whenever 20 bytes are there: random nonce, time and type,
    version 1, stream 1."""
    return (rng.randbytes(20) + b'\x01\x01' + rng.randbytes(max(length - 22, 0)))[:length]


def same_as_intake(res, rows, **params):
    """The embedded intake records of packets ``rows`` are byte-equal to what intake.check_objects fills for
    their payloads."""
    want = intake.check_objects([res.payload(i) for i in rows], **params)
    assert res.records['intake'][rows].tobytes() == want.records.tobytes()


@pytest.fixture(scope='module')
def kats(golden):
    return golden('packet_kats.json')


@pytest.fixture(scope='module')
def intake_objects(golden):
    return {k['name']: regen_object(k) for k in golden('intake_kats.json')['kats']}


@pytest.mark.parametrize('kind', ['sum', 'object'])
def test_every_length_at_every_source_residue(gpulib, kind):
    """Payload lengths 0 .. 300 (the 111 | 112 and 239 | 240 padding edges of either chain) each at all 16
    alignments of its first byte in the uploaded arena: a datagram buffer, where bytes that are no magic in
    front of a packet are skipped one by one, puts every payload where it is wanted."""
    rng = random.Random(300 + len(kind))
    buf, payloads, starts = bytearray(), [], []
    for length in range(301):
        for residue in range(16):
            buf += bytes((residue - len(buf) - 24) % 16)
            p = object_bytes(rng, length) if kind == 'object' else rng.randbytes(length)
            buf += packet(b'object' if kind == 'object' else b'ping', p)
            payloads.append(p)
            starts.append(len(buf) - length)
    assert {(len(p), s % 16) for p, s in zip(payloads, starts)} == {(L, r) for L in range(301) for r in range(16)}
    packets.reset_stats()
    res = packets.check_buffers([bytes(buf)], datagram=True, now=NOW)
    assert len(res) == len(payloads) == 4816 and int(res.close[0]) == packets.OPEN and int(res.consumed[0]) == len(buf)
    assert (res.offset + 24).tolist() == starts
    assert res.computed.tolist() == [sum4(p) for p in payloads]
    assert not res.status.any()
    st = packets.stats()
    n_obj = 16 * (301 - 20) if kind == 'object' else 0
    assert (st['object_rows'], st['sum_rows'], st['empty_rows'], st['host_rows']) == (n_obj, 4816 - 16 - n_obj, 16, 0)
    assert st['calls'] == 1 and st['packets'] == 4816 and st['pack_ms'] > 0
    if kind == 'object':
        assert (res.intake.status[:16 * 20] == intake.MALFORMED).all() and (res.intake.status[16 * 20:] != intake.MALFORMED).all()
        same_as_intake(res, np.arange(len(res)), now=NOW)


@pytest.mark.parametrize('rows', [1, 3, 4, 5, 63, 64, 65])
def test_row_counts_around_the_packs_four_rows_per_wave(gpulib, rows):
    rng = random.Random(rows)
    objs = [object_bytes(rng, rng.choice([20, 119, 120, 247, 248, rng.randrange(20, 700)])) for _ in range(rows)]
    pings = [rng.randbytes(rng.choice([1, 111, 112, 239, 240, rng.randrange(1, 700)])) for _ in range(rows)]
    res = packets.check_buffers([b''.join(packet(b'object', o) for o in objs), b''.join(packet(b'ping', p) for p in pings)],
                                now=NOW)
    assert res.count.tolist() == [rows, rows] and res.first.tolist() == [0, rows] and not res.status.any()
    assert res.computed.tolist() == [sum4(p) for p in objs + pings]
    same_as_intake(res, np.arange(rows), now=NOW)
    assert not res.records['intake'][rows:].tobytes().strip(b'\x00')


def check_case(case, res, c, buf):
    want = case['batch']
    idx = list(res.of_connection(c))
    assert len(idx) == len(want['records']), case['name']
    for i, w in zip(idx, want['records']):
        r = res.records[i]
        assert int(r['conn']) == c
        got = {f: int(r[f]) for f in ('offset', 'length', 'command', 'exact', 'checksum', 'status')}
        assert got == {f: w[f] for f in got}, (case['name'], w)
        # the payload of a TOO_LONG packet is not hashed
        assert int(r['computed']) == (0 if w['status'] & packets.TOO_LONG else w['computed']), (case['name'], w)
        assert res.payload(i) == buf[w['offset'] + 24:w['offset'] + 24 + w['length']]
    assert (int(res.consumed[c]), int(res.close[c])) == (want['consumed'], want['close']), case['name']


def test_the_fixture_is_reproduced_record_for_record(gpulib, kats, intake_objects):
    groups = {}
    for case in kats['connections']:
        groups.setdefault((case['now'], tuple(case['streams'])), []).append(case)
    assert len(groups) >= 4
    for (now, streams), cases in groups.items():
        bufs = [regen_buffer(c, intake_objects) for c in cases]
        for case, buf in zip(cases, bufs):
            assert hashlib.sha512(buf).hexdigest() == case['sha512'], case['name']
        res = packets.check_buffers(bufs, [c['established'] for c in cases], [c['datagram'] for c in cases],
                                    streams=streams, now=now)
        assert len(res) == sum(len(c['batch']['records']) for c in cases)
        for c, (case, buf) in enumerate(zip(cases, bufs)):
            check_case(case, res, c, buf)
            if 'intake_status' in case:
                rows = list(res.of_connection(c))
                assert res.intake.status[rows].tolist() == case['intake_status'], case['name']
                assert [res.command_name(i) for i in rows] == [b'object'] * len(rows)
        # the yardstick: the same objects through the existing path, byte for byte
        valid = np.flatnonzero((res.command == packets.OBJECT) & (res.status == packets.OK))
        same_as_intake(res, valid, streams=streams, now=now)
        others = np.setdiff1d(np.arange(len(res)), valid)
        assert not res.records['intake'][others].tobytes().strip(b'\x00')
        assert res.objects().tolist() == [int(i) for i in valid if res.intake.status[i] == intake.OK]
    # one buffer alone gives what it gives among others
    case = next(c for c in kats['connections'] if c['name'] == 'spoiled_second_stream')
    buf = regen_buffer(case, intake_objects)
    check_case(case, packets.check_buffers([buf], now=NOW), 0, buf)


def test_check_acks_agrees_with_the_host_check_on_every_fixture_ack(gpulib, kats, intake_objects):
    acks = [regen_buffer(a, intake_objects) for a in kats['acks']]
    for a, ack in zip(kats['acks'], acks):
        assert hashlib.sha512(ack).hexdigest() == a['sha512'], a['name']
    valid, res = packets.check_acks(acks, now=NOW)
    assert valid.tolist() == [a['valid'] for a in kats['acks']] == [receive.ack_has_valid_header(a) for a in acks]
    assert valid.sum() >= 3
    rows = np.flatnonzero(valid)
    want = intake.check_objects([acks[i][24:] for i in rows], now=NOW)
    assert res.records[rows].tobytes() == want.records.tobytes()
    assert not res.records[~valid].tobytes().strip(b'\x00')
    assert res.tag(int(rows[0])) == acks[rows[0]][24:][int(want.payloadOffset[0]):][:32]

    class Opened(object):  # what receive.check_opened_acks asks of an OpenedMsgs
        def accepted(self):
            return [1, 3, 4]

        def ackData(self, i):
            return acks[i]

    picked, ok, recs = receive.check_opened_acks(Opened(), now=NOW)
    assert picked == [1, 3, 4] and ok.tolist() == [bool(valid[i]) for i in picked] and len(recs) == 3


def test_one_longest_object_among_63_short_ones(gpulib):
    rng = random.Random(1 << 18)
    objs = [object_bytes(rng, rng.randrange(20, 300)) for _ in range(63)]
    objs.insert(17, object_bytes(rng, 22 + (1 << 18)))  # 2^18 bytes after its header: the longest the intake accepts
    objs.append(object_bytes(rng, 1 << 18))
    res = packets.check_buffers([b''.join(packet(b'object', o) for o in objs)], now=NOW)
    assert len(res) == 65 and not res.status.any() and int(res.close[0]) == packets.OPEN
    assert res.computed.tolist() == [sum4(o) for o in objs]
    assert (res.intake.status != intake.TOO_LARGE).all()
    same_as_intake(res, np.arange(65), now=NOW)


def test_payloads_above_the_devices_limit_are_hashed_on_the_host(gpulib):
    rng = random.Random(1600100)
    parts = [(b'ping', rng.randbytes(100)), (b'inv', rng.randbytes((1 << 18) + 38)), (b'inv', rng.randbytes((1 << 18) + 39)),
             (b'object', object_bytes(rng, 200)), (b'getdata', rng.randbytes(1600100)), (b'pong', rng.randbytes(7)),
             (b'object', object_bytes(rng, (1 << 18) + 39 + 100))]
    packets.reset_stats()
    res = packets.check_buffers([b''.join(packet(c, p) for c, p in parts)], now=NOW)
    assert len(res) == len(parts) and not res.status.any()
    assert res.computed.tolist() == [sum4(p) for _, p in parts]
    st = packets.stats()
    assert (st['host_rows'], st['object_rows'], st['sum_rows']) == (3, 1, 3)
    assert res.intake.status[6] == intake.TOO_LARGE and int(res.close[0]) == packets.OPEN


def test_a_too_large_object_with_a_good_checksum_keeps_its_connection(gpulib):
    rng = random.Random(23)
    big = object_bytes(rng, 22 + (1 << 18) + 1)
    tail = rng.randbytes(9)
    res = packets.check_buffers([packet(b'object', big) + packet(b'ping', tail),
                                 packet(b'object', big, spoil=True) + packet(b'ping', tail)], now=NOW)
    assert res.count.tolist() == [2, 1] and res.close.tolist() == [packets.OPEN, packets.INVALID_COMMAND]
    assert res.status.tolist() == [packets.OK, packets.OK, packets.BAD_CHECKSUM]
    assert res.intake.status[0] == intake.TOO_LARGE and not res.records['intake'][2].tobytes().strip(b'\x00')
    assert res.consumed.tolist() == [2 * 24 + len(big) + 9, 0] and len(res.objects()) == 0
    same_as_intake(res, [0], now=NOW)


@pytest.mark.parametrize('ids', [[0], [0, 0, 0]])
def test_sorted_and_binned_launches_agree(gpulib, shards, monkeypatch, ids):
    rng = random.Random(3000)
    bufs, payloads = [], []
    for _ in range(6):
        parts = []
        for _ in range(500):
            if rng.random() < 0.8:
                parts.append((b'object', object_bytes(rng, rng.choice([20, 54, 119, 120, 247, 248, rng.randrange(20, 3000)]))))
            else:
                parts.append((b'addr', rng.randbytes(rng.randrange(0, 2000))))
        parts.append((b'object', object_bytes(rng, rng.choice([20000, 16384, 8191]))))
        bufs.append(b''.join(packet(c, p) for c, p in parts))
        payloads += [p for _, p in parts]
    shards(ids)
    seen = []
    for binned in ('0', '1'):
        monkeypatch.setenv('BMPOW_VBINNED', binned)
        packets.reset_stats()
        res = packets.check_buffers(bufs, now=NOW)
        assert len(res) == len(payloads) == 3006 and not res.status.any(), binned
        assert res.computed.tolist() == [sum4(p) for p in payloads], binned
        st = packets.stats()
        assert st['calls'] == 1 and st['object_rows'] > 2000 and st['object_ms'] > 0 and st['sum_ms'] > 0
        seen.append(res.records.tobytes())
    assert seen[0] == seen[1]
    same_as_intake(res, np.flatnonzero(res.command == packets.OBJECT), now=NOW)


def test_abort_an_empty_call_and_a_connection_of_zero_bytes(gpulib):
    buf = packet(b'ping', b'abc') + packet(b'object', object_bytes(random.Random(5), 100))
    gpulib.bmpow_abort()
    try:
        with pytest.raises(_lib.BmpowError) as e:
            packets.check_buffers([buf], now=NOW)
        assert e.value.code == _lib.E_ABORTED
        with pytest.raises(_lib.BmpowError) as e:
            packets.check_acks([buf[27:]], now=NOW)  # the object packet alone: a well-formed ack
        assert e.value.code == _lib.E_ABORTED
    finally:
        gpulib.bmpow_clear_abort()
    packets.reset_stats()
    assert len(packets.check_buffers([])) == 0
    res = packets.check_buffers([b'', buf, b'', b'\x00' * 30], now=NOW)
    assert res.count.tolist() == [0, 2, 0, 0] and res.first.tolist() == [0, 0, 2, 2]
    assert res.close.tolist() == [packets.OPEN, packets.OPEN, packets.OPEN, packets.BAD_MAGIC]
    assert res.consumed.tolist() == [0, len(buf), 0, 0] and res.computed.tolist() == [sum4(b'abc'), sum4(buf[51:])]
    res = packets.check_buffers([b'', b'\x01' * 23], datagram=True)
    assert len(res) == 0 and res.consumed.tolist() == [0, 0]
    assert packets.stats()['calls'] == 1  # only the call that had packets reached the device
    conns = np.zeros(1, dtype=packets.CONN_DTYPE)
    assert gpulib.bmpow_packets_batch(0, None, None, None, None, None, 0, conns.ctypes.data) == 0
