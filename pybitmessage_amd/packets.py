"""Framing received packets on the GPU: ``network/bmproto.py``'s header and checksum states for whole
connection buffers.

The reference's network thread sees connection read buffers.  For every packet in them it unpacks the
header and checks the magic and the length (``state_bm_header``, ``src/network/bmproto.py:85-104``),
compares ``hashlib.sha512(payload).digest()[0:4]`` with the header's checksum (``state_bm_command``,
``:106-111``) and only then runs the command's handler.  :func:`check_buffers` does that for a list of
buffers as they came off the sockets with one upload and one pass over the device
(``bmpow_packets_batch``, include/bmpow_packets.h): per packet the reference's verdict, and per ``object``
packet the record :func:`pybitmessage_amd.intake.check_objects` would give for its payload -- the checksum
comes out of the same hash chain as the inventory hash.  :func:`check_acks` is
``objectProcessor.ackDataHasAValidHeader`` for a batch of acknowledgements, and :func:`frame` the walk alone,
on the host.  The item lists of ``inv`` / ``dinv`` / ``getdata`` packets go on to
:func:`pybitmessage_amd.inventory.check_invs`, which takes a :class:`PacketResult` as it is; the other handlers
(``addr``, ``version`` ...) stay with the caller.
No CPU fallback: without the HIP library the device calls raise :class:`BmpowUnavailable`.
"""
import ctypes

import numpy as np

from . import _lib, intake
from .verify import P64, _pointers

#: ``bmpow_packet_rec.status``: 0, or the reasons the reference sets ``self.invalid`` for, or'ed
OK, TOO_LONG, BAD_CHECKSUM, NOT_ESTABLISHED = 0, 1, 2, 4
#: ``bmpow_packet_conn.close``
OPEN, BAD_MAGIC, INVALID_COMMAND, HANDSHAKE = 0, 1, 2, 3
CLOSE_NAMES = {OPEN: 'OPEN', BAD_MAGIC: 'BAD_MAGIC', INVALID_COMMAND: 'INVALID_COMMAND', HANDSHAKE: 'HANDSHAKE'}
#: ``bmpow_packet_rec.command``: index into the handlers ``bm_command_*`` has, 0 for any other command
COMMANDS = (None, 'error', 'getdata', 'inv', 'dinv', 'object', 'addr', 'portcheck', 'ping', 'pong', 'verack',
            'version')
UNIMPLEMENTED, OBJECT = 0, COMMANDS.index('object')
HEADER_SIZE = 24
MAX_MESSAGE_SIZE = 1600100
_ESTABLISHED, _DATAGRAM = 1, 2

#: ``bmpow_packet_rec`` and ``bmpow_packet_conn`` as numpy records
REC_DTYPE = np.dtype([('conn', '<u4'), ('offset', '<u4'), ('length', '<u4'), ('command', 'u1'), ('exact', 'u1'),
                      ('reserved', '<u2'), ('checksum', '<u4'), ('computed', '<u4'), ('status', '<u4'),
                      ('reserved2', '<u4'), ('intake', intake.REC_DTYPE)])
CONN_DTYPE = np.dtype([('consumed', '<u8'), ('first', '<u4'), ('count', '<u4'), ('close', '<u4'),
                       ('reserved', '<u4')])
assert REC_DTYPE.itemsize == ctypes.sizeof(_lib.BmpowPacketRec)
assert CONN_DTYPE.itemsize == ctypes.sizeof(_lib.BmpowPacketConn)


def _flags(value, n, bit):
    if not np.ndim(value):
        return np.full(n, bit if value else 0, dtype=np.uint32)
    out = np.where(np.asarray(list(value), dtype=bool), np.uint32(bit), np.uint32(0)).astype(np.uint32)
    if len(out) != n:
        raise ValueError('one flag per buffer')
    return out


class PacketResult(object):
    """What :func:`check_buffers` or :func:`frame` found: numpy columns over the packet records (``conn``,
    ``offset``, ``length``, ``command``, ``checksum``, ``computed``, ``status``) and over the per-connection
    table (``consumed``, ``first``, ``count``, ``close``).  ``intake`` is an
    :class:`pybitmessage_amd.intake.IntakeResult` over the same rows: filled for the valid ``object``
    packets, zeros elsewhere."""

    def __init__(self, buffers, recs, conns):
        self._buffers = buffers
        self.records, self.connections = recs, conns
        self.conn, self.offset, self.length = recs['conn'], recs['offset'], recs['length']
        self.command, self.exact = recs['command'], recs['exact']
        self.checksum, self.computed, self.status = recs['checksum'], recs['computed'], recs['status']
        self.consumed, self.first, self.count, self.close = (conns['consumed'], conns['first'], conns['count'],
                                                             conns['close'])
        self.intake = intake.IntakeResult(_Payloads(self), recs['intake'])

    def __len__(self):
        return len(self.records)

    def payload(self, i):
        """Packet i's payload, cut from the caller's buffer."""
        r = self.records[i]
        at = int(r['offset']) + HEADER_SIZE
        return self._buffers[int(r['conn'])][at:at + int(r['length'])]

    def command_name(self, i):
        """The command as the reference's ``self.command`` holds it: the 12 bytes without their trailing
        NULs."""
        r = self.records[i]
        at = int(r['offset']) + 4
        return bytes(self._buffers[int(r['conn'])][at:at + 12]).rstrip(b'\x00')

    def objects(self):
        """Indices of the packets whose object goes to the ``objectProcessorQueue``: valid ``object``
        packets every intake check passed."""
        return np.flatnonzero((self.command == OBJECT) & (self.status == OK) & (self.intake.status == intake.OK))

    def of_connection(self, c):
        """The record indices of buffer c's packets."""
        first = int(self.first[c])
        return range(first, first + int(self.count[c]))


class _Payloads(object):
    """The packets' payloads as the sequence an ``IntakeResult`` slices tags from."""

    def __init__(self, result):
        self._result = result

    def __getitem__(self, i):
        return self._result.payload(i)

    def __len__(self):
        return len(self._result)


def _as_buffers(buffers):
    bufs = buffers if type(buffers) is list else list(buffers)
    if set(map(type, bufs)) - {bytes}:  # bytearray / memoryview: one bytes copy each
        bufs = [b if type(b) is bytes else bytes(b) for b in bufs]
    return bufs


def frame(buffer, established=True, datagram=False):
    """Host only (``bmpow_packets_frame``).  The walk of ``state_bm_header`` / ``state_bm_command`` over one
    buffer with every checksum taken for good: a :class:`PacketResult` of one connection, its records
    carrying the header fields and the status that needs no hash."""
    buf = bytes(buffer)
    lib = _lib.host()
    flags = (_ESTABLISHED if established else 0) | (_DATAGRAM if datagram else 0)
    conns = np.zeros(1, dtype=CONN_DTYPE)
    raw = ctypes.cast(ctypes.c_char_p(buf), ctypes.c_void_p)
    cp = conns.ctypes.data_as(ctypes.POINTER(_lib.BmpowPacketConn))
    n = _lib.check(lib, lib.bmpow_packets_frame(raw, len(buf), flags, None, 0, cp), 'bmpow_packets_frame')
    recs = np.zeros(n, dtype=REC_DTYPE)
    _lib.check(lib, lib.bmpow_packets_frame(raw, len(buf), flags, recs.ctypes.data, n, cp), 'bmpow_packets_frame')
    return PacketResult([buf], recs, conns)


def row_blocks(length, as_object):
    """Host only.  The 128-byte pool blocks the row plan gives a payload of ``length`` bytes."""
    return int(_lib.host().bmpow_packets_row_blocks(1 if as_object else 0, int(length)))


def _params(streams, nonceTrialsPerByte, payloadLengthExtraBytes, recvTime, now):
    st = np.ascontiguousarray(np.asarray(list(streams), dtype=np.uint64))
    return st, _lib.BmpowIntakeParams(int(now), int(recvTime), int(nonceTrialsPerByte), int(payloadLengthExtraBytes),
                                      st.ctypes.data_as(P64), len(st))


def check_buffers(buffers, established=True, datagram=False, streams=(1,), nonceTrialsPerByte=0,
                  payloadLengthExtraBytes=0, recvTime=0, now=0):
    """Frame, hash and judge a list of connection read buffers in one call.  ``established``
    (``fullyEstablished``) and ``datagram`` (a ``SOCK_DGRAM`` socket) are one value for all or one per
    buffer; the other parameters are :func:`pybitmessage_amd.intake.check_objects`'.  Returns a
    :class:`PacketResult`: per buffer its packets up to the first that closes the connection, ``consumed``
    (what to cut off the read buffer) and ``close``; a buffer that stopped at ``HANDSHAKE`` is fed again,
    from ``consumed`` on, once the caller has run the ``version`` / ``verack`` handler."""
    bufs = _as_buffers(buffers)
    n = len(bufs)
    conns = np.zeros(n, dtype=CONN_DTYPE)
    if n == 0:
        return PacketResult(bufs, np.zeros(0, dtype=REC_DTYPE), conns)
    flags = _flags(established, n, _ESTABLISHED) | _flags(datagram, n, _DATAGRAM)
    host = _lib.host()
    ptrs = _pointers(bufs)
    lens = np.fromiter(map(len, bufs), dtype=np.uint64, count=n)
    # the walk alone sizes the records (no device)
    cap = _lib.check(host, host.bmpow_packets_count(n, ptrs.ctypes.data, lens.ctypes.data_as(P64), flags.ctypes.data),
                     'bmpow_packets_count')
    lib = _lib.get()
    recs = np.zeros(cap, dtype=REC_DTYPE)
    st, prm = _params(streams, nonceTrialsPerByte, payloadLengthExtraBytes, recvTime, now)
    got = _lib.check(lib, lib.bmpow_packets_batch(n, ptrs.ctypes.data, lens.ctypes.data_as(P64), flags.ctypes.data,
                                                  ctypes.byref(prm), recs.ctypes.data, cap, conns.ctypes.data),
                     'bmpow_packets_batch')
    return PacketResult(bufs, recs[:got], conns)


def check_acks(ackDatas, streams=(1,), nonceTrialsPerByte=0, payloadLengthExtraBytes=0, recvTime=0, now=0):
    """``[objectProcessor.ackDataHasAValidHeader(a) for a in ackDatas]`` in one call
    (``bmpow_packets_ack_batch``), and what ``bm_command_object`` will say to each valid one when it is sent
    on: returns ``(valid, IntakeResult)``, a bool array and the intake records of ``ackData[24:]`` (zeros
    for the acks that are not valid)."""
    acks = _as_buffers(ackDatas)
    n = len(acks)
    valid = np.zeros(n, dtype=np.uint8)
    recs = np.zeros(n, dtype=intake.REC_DTYPE)
    objs = [a[HEADER_SIZE:] for a in acks]
    if n == 0:
        return valid.astype(bool), intake.IntakeResult(objs, recs)
    lib = _lib.get()
    ptrs = _pointers(acks)
    lens = np.fromiter(map(len, acks), dtype=np.uint64, count=n)
    st, prm = _params(streams, nonceTrialsPerByte, payloadLengthExtraBytes, recvTime, now)
    _lib.check(lib, lib.bmpow_packets_ack_batch(n, ptrs.ctypes.data, lens.ctypes.data_as(P64), ctypes.byref(prm),
                                                valid.ctypes.data, recs.ctypes.data), 'bmpow_packets_ack_batch')
    return valid.astype(bool), intake.IntakeResult(objs, recs)


def stats():
    s = _lib.BmpowPacketsStats()
    lib = _lib.get()
    _lib.check(lib, lib.bmpow_packets_get_stats(ctypes.byref(s)), 'bmpow_packets_get_stats')
    return {f: getattr(s, f) for f, _ in s._fields_}


def reset_stats():
    _lib.get().bmpow_packets_reset_stats()
