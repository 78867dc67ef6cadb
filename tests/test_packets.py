"""Packet framing without a GPU: the walk over a connection buffer's headers through its host-only entry point
``bmpow_packets_frame`` against tests/golden/packet_kats.json (made by running the reference's primitives and a
line-by-line restatement of its state machine, tests/golden/make_packet_golden.py), the same walk over every
prefix of every fixture buffer, and the row plan's block counts against direct padding."""
import hashlib

import numpy as np
import pytest

from pybitmessage_amd import _lib, packets
from tests.golden.make_intake_golden import regen as regen_object
from tests.golden.make_packet_golden import regen_buffer

FRAME_FIELDS = ('offset', 'length', 'command', 'exact', 'checksum', 'status')


@pytest.fixture(scope='module')
def kats(golden):
    return golden('packet_kats.json')


@pytest.fixture(scope='module')
def buffers(golden, kats):
    """Every fixture connection's bytes, rebuilt once from seeds and pinned by their SHA-512."""
    objects = {k['name']: regen_object(k) for k in golden('intake_kats.json')['kats']}
    out = {}
    for case in kats['connections']:
        buf = regen_buffer(case, objects)
        assert len(buf) == case['len'] and hashlib.sha512(buf).hexdigest() == case['sha512'], case['name']
        out[case['name']] = buf
    return out


def rows_of(result, fields=FRAME_FIELDS):
    return [{f: int(r[f]) for f in fields} for r in result.records]


def test_record_layouts():
    import ctypes
    assert ctypes.sizeof(_lib.BmpowPacketRec) == 120 and packets.REC_DTYPE.itemsize == 120
    assert packets.REC_DTYPE.fields['intake'][1] == 32 and _lib.BmpowPacketRec.intake.offset == 32
    assert ctypes.sizeof(_lib.BmpowPacketConn) == 24
    for name, _ in _lib.BmpowPacketRec._fields_:
        assert packets.REC_DTYPE.fields[name][1] == getattr(_lib.BmpowPacketRec, name).offset, name
    assert list(packets.COMMANDS[1:]) == ['error', 'getdata', 'inv', 'dinv', 'object', 'addr', 'portcheck', 'ping', 'pong',
                                          'verack', 'version']


def test_frame_reproduces_every_fixture_connection(kats, buffers):
    assert list(packets.COMMANDS[1:]) == kats['handlers'] and packets.MAX_MESSAGE_SIZE == kats['max_message_size']
    for case in kats['connections']:
        res = packets.frame(buffers[case['name']], case['established'], case['datagram'])
        want = case['frame']
        assert rows_of(res) == want['records'], case['name']
        assert (int(res.consumed[0]), int(res.close[0])) == (want['consumed'], want['close']), case['name']
        assert int(res.first[0]) == 0 and int(res.count[0]) == len(want['records']) == len(res)
        assert not res.records['computed'].any() and not res.records['intake'].tobytes().strip(b'\x00')


def test_accessors_cut_the_callers_buffer(kats, buffers):
    case = next(c for c in kats['connections'] if c['name'] == 'object_nul_x')
    buf = buffers[case['name']]
    res = packets.frame(buf)
    assert res.command_name(0) == b'object\x00x' and res.command_name(1) == b'ping'
    assert res.payload(0) == buf[24:24 + int(res.length[0])] and res.payload(1) == b''
    assert list(res.of_connection(0)) == [0, 1]
    res = packets.frame(bytearray(buffers['object_in_capitals']))
    assert res.command_name(0) == b'OBJECT' and int(res.command[0]) == packets.OBJECT and int(res.exact[0]) == 0


def test_every_prefix_frames_a_prefix_and_resumes(kats, buffers):
    """A read buffer grows as bytes arrive: at whatever length 0 .. len it is cut, the walk frames a prefix of the
    whole buffer's packets, and fed again from ``consumed`` on with the rest it frames the remainder.  The cuts
    are lengths over one copy of the buffer and the walks from each ``consumed`` are kept, so that the sweep of
    the fixture's megabyte buffers stays a matter of seconds."""
    import ctypes
    lib = _lib.host()
    conn = _lib.BmpowPacketConn()
    cuts = 0
    for case in kats['connections']:
        buf = buffers[case['name']]
        flags = (1 if case['established'] else 0) | (2 if case['datagram'] else 0)
        full = packets.frame(buf, case['established'], case['datagram'])
        whole, n_all = full.records.tobytes(), len(full)
        end = (int(full.consumed[0]), int(full.close[0]))
        base = ctypes.cast(ctypes.c_char_p(buf), ctypes.c_void_p).value
        recs = np.zeros(n_all + 1, dtype=packets.REC_DTYPE)
        size = packets.REC_DTYPE.itemsize
        resumed = {}

        def rest_from(consumed):
            """(records with their offsets in the whole buffer, consumed, close) of the walk over buf[consumed:]"""
            if consumed not in resumed:
                rest = packets.frame(buf[consumed:], case['established'], case['datagram'])
                rest.records['offset'] += consumed
                resumed[consumed] = (rest.records.tobytes(), (int(rest.consumed[0]) + consumed, int(rest.close[0])))
            return resumed[consumed]

        for cut in range(len(buf) + 1):
            n = lib.bmpow_packets_frame(base, cut, flags, recs.ctypes.data, n_all + 1, ctypes.byref(conn))
            assert 0 <= n <= n_all and conn.count == n and conn.consumed <= cut, (case['name'], cut)
            got = recs[:n].tobytes()
            assert got == whole[:n * size], (case['name'], cut)
            if conn.close != packets.OPEN:  # closed, or waiting for the caller: where the whole buffer ends too
                assert n == n_all and (conn.consumed, conn.close) == end, (case['name'], cut)
                continue
            tail, tail_end = rest_from(conn.consumed)
            assert got + tail == whole and tail_end == end, (case['name'], cut)
        cuts += len(buf) + 1
    assert cuts > 10000


def test_row_plan_matches_direct_padding():
    """Blocks of a row = the SHA-512 padding of what the device hashes from the pool: object[8:] for an object
    row, the whole payload for a sum row, for every length across the one- and two-block edges."""
    for length in range(442):
        assert packets.row_blocks(length, False) == (length + 1 + 16 + 127) // 128, length
        want = 0 if length < 8 else (length - 8 + 1 + 16 + 127) // 128
        assert packets.row_blocks(length, True) == want, length
    assert packets.row_blocks(111, False) == 1 and packets.row_blocks(112, False) == 2
    assert packets.row_blocks(119, True) == 1 and packets.row_blocks(120, True) == 2
    assert packets.row_blocks(packets.MAX_MESSAGE_SIZE, False) == 12501  # 1,600,100 + 17 bytes in 128-byte blocks


def test_python_level_checks_need_no_device():
    res = packets.check_buffers([])
    assert len(res) == 0 and len(res.connections) == 0 and len(res.objects()) == 0
    valid, recs = packets.check_acks([])
    assert len(valid) == 0 and len(recs) == 0
    with pytest.raises(ValueError):
        packets._flags([True], 2, 1)
    assert packets._flags(True, 3, 2).tolist() == [2, 2, 2] and packets._flags([1, 0], 2, 1).tolist() == [1, 0]
    assert np.dtype(packets.CONN_DTYPE).names == ('consumed', 'first', 'count', 'close', 'reserved')
