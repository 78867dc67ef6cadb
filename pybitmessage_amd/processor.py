"""The object processor's queue on the GPU: ``objectProcessor.run`` for a whole flood in one call.

The reference's objectProcessor thread takes one ``(objectType, data)`` pair at a time off its queue
(``src/class_objectProcessor.py:64-110``).  For every object it runs ``checkackdata`` (``:129-154``: is
``data[16:]`` a key of ``state.ackdataForWhichImWatching``?) and then routes by type (``:72-95``) to
``processgetpubkey`` (``:176-268``), ``processonion`` (``:156-174``, with ``protocol.checkIPAddress``,
``src/protocol.py:150-227``) or to the handlers :mod:`pybitmessage_amd.receive` has as batch calls.  A
:class:`Dispatcher` holds the watched ack data and my addresses (include/bmpow_proc.h); :meth:`Dispatcher.dispatch`
judges a list of objects in one call and returns one record per object.  The SQL update, the UI signal,
``knownnodes``, the worker queue and the host string stay with the caller.
No CPU fallback: without the HIP library the device calls raise :class:`BmpowUnavailable`.
"""
import base64
import ctypes
import hashlib
import socket

import numpy as np

from . import _lib, addresses, packets
from .verify import P64, _fast, _pointers

#: object types (``protocol.OBJECT_*``)
OBJECT_GETPUBKEY, OBJECT_PUBKEY, OBJECT_MSG, OBJECT_BROADCAST, OBJECT_ONIONPEER = 0, 1, 2, 3, 0x746f72
#: ``route``
GETPUBKEY, PUBKEY, MSG, BROADCAST, ONIONPEER, UNKNOWN_TYPE = 0, 1, 2, 3, 4, 5
#: ``ack``
NOT_CHECKED, NOT_WATCHED, FOUND, FOUND_EARLIER = 0, 1, 2, 3
#: ``status``
(NONE, TOO_LONG, MALFORMED, VERSION_ZERO, VERSION_ONE, VERSION_TOO_HIGH, SHORT_HASH, SHORT_TAG, NOT_MINE,
 VERSION_MISMATCH, STREAM_MISMATCH, CHAN, SENT_RECENTLY, SEND_V2, SEND_V3, SEND_V4, NO_HOST, RAISES, PEER) = range(19)
#: ``host_class``
HOST_NONE, V4, ONION, V6 = 0, 1, 2, 3
NO_ROW = 0xffffffff
#: the worker command behind each ``SEND_*`` (``:263-268``)
COMMANDS = {SEND_V2: 'doPOWForMyV2Pubkey', SEND_V3: 'sendOutOrStoreMyV3Pubkey', SEND_V4: 'sendOutOrStoreMyV4Pubkey'}

REC_DTYPE = np.dtype([('version', '<u8'), ('stream', '<u8'), ('port', '<u8'), ('route', '<u4'), ('ack', '<u4'),
                      ('ack_aux', '<u4'), ('ack_first', '<u4'), ('status', '<u4'), ('key_off', '<u4'),
                      ('key_len', '<u4'), ('address', '<u4'), ('host_off', '<u4'), ('host_len', '<u4'),
                      ('host_class', '<u4'), ('reserved', '<u4')])
ADDRESS_DTYPE = np.dtype([('ripe', np.uint8, 20), ('tag', np.uint8, 32), ('version', '<u4'), ('stream', '<u8'),
                          ('last_pubkey_send_time', '<i8'), ('chan', '<u4'), ('reserved', '<u4')])
assert REC_DTYPE.itemsize == ctypes.sizeof(_lib.BmpowProcRec) == 72
assert ADDRESS_DTYPE.itemsize == ctypes.sizeof(_lib.BmpowProcAddress) == 80


def tag_of(version, stream, ripe):
    """The tag ``shared.reloadMyAddressHashes`` keeps an address under (``src/shared.py:135-138``)."""
    data = addresses.encodeVarint(int(version)) + addresses.encodeVarint(int(stream)) + bytes(ripe)
    return hashlib.sha512(hashlib.sha512(data).digest()).digest()[32:]


def address_rows(rows):
    """An ``ADDRESS_DTYPE`` array from ``(version, stream, ripe, chan, last_pubkey_send_time)`` tuples; the tag of
    each is computed here."""
    rows = list(rows)
    out = np.zeros(len(rows), dtype=ADDRESS_DTYPE)
    for i, (version, stream, ripe, chan, last) in enumerate(rows):
        ripe = bytes(ripe)
        if len(ripe) != 20:
            raise ValueError('a ripe is 20 bytes')
        out[i] = (np.frombuffer(ripe, dtype=np.uint8), np.frombuffer(tag_of(version, stream, ripe), dtype=np.uint8),
                  version, stream, last, 1 if chan else 0, 0)
    return out


def rows_from_addresses(entries):
    """The same from ``(address, chan, last_pubkey_send_time)`` as ``keys.dat`` holds them, decoded with
    :func:`pybitmessage_amd.addresses.decodeAddress`; an address that does not decode raises ``ValueError``."""
    rows = []
    for address, chan, last in entries:
        status, version, stream, ripe = addresses.decodeAddress(address)
        if status != 'success':
            raise ValueError('%s: %s' % (address, status))
        rows.append((version, stream, ripe, chan, last))
    return address_rows(rows)


def _packed(keys):
    """(n, bytes, offsets) of a list of byte strings, as the watch calls take them."""
    keys = [bytes(k) for k in keys]
    offs = np.zeros(len(keys) + 1, dtype=np.uint64)
    if keys:
        offs[1:] = np.cumsum(np.fromiter(map(len, keys), dtype=np.uint64, count=len(keys)))
    return len(keys), b''.join(keys), offs


def watch_slot(seed, log2_slots, key):
    """Host only (``bmpow_proc_watch_slot``): the slot a watched key's probe starts from."""
    key = bytes(key)
    return int(_lib.host().bmpow_proc_watch_slot(int(seed), int(log2_slots), key, len(key)))


def _rec_from(struct):
    return np.frombuffer(bytes(struct), dtype=REC_DTYPE)[0]


def walk(object_type, data, address_table=None, now=0):
    """Host only (``bmpow_proc_walk``): one object's record without the ack fields, from the functions the
    kernel runs.  ``address_table`` is an ``ADDRESS_DTYPE`` array (:func:`address_rows`)."""
    data = bytes(data)
    table = np.zeros(0, dtype=ADDRESS_DTYPE) if address_table is None else np.ascontiguousarray(address_table, dtype=ADDRESS_DTYPE)
    out = _lib.BmpowProcRec()
    lib = _lib.host()
    _lib.check(lib, lib.bmpow_proc_walk(int(object_type) & 0xffffffff, data, len(data), len(table),
                                        table.ctypes.data if len(table) else None, int(now), ctypes.byref(out)),
               'bmpow_proc_walk')
    return _rec_from(out)


def host_string(data, rec):
    """``hostStandardFormat`` of a ``PEER`` record, as ``checkIPAddress`` formats it (``src/protocol.py:156-166``;
    the onion branch with Python 2's ``str`` from ``b32encode``)."""
    host = bytes(data[int(rec['host_off']):int(rec['host_off']) + int(rec['host_len'])])
    if rec['host_class'] == V4:
        return socket.inet_ntop(socket.AF_INET, host[12:])
    if rec['host_class'] == ONION:
        return base64.b32encode(host[6:]).decode('ascii').lower() + '.onion'
    return socket.inet_ntop(socket.AF_INET6, host)


class DispatchResult(object):
    """What :meth:`Dispatcher.dispatch` found, one row per object: numpy columns over ``REC_DTYPE`` (``route``,
    ``ack``, ``ack_aux``, ``ack_first``, ``status``, ``version``, ``stream``, ``port``, ``key_off``, ``key_len``,
    ``address``, ``host_off``, ``host_len``, ``host_class``) and index helpers."""

    def __init__(self, objects, types, recs, address_table):
        self._objects, self.types, self.records, self._addresses = objects, types, recs, address_table
        for name in REC_DTYPE.names:
            setattr(self, name, recs[name])

    def __len__(self):
        return len(self.records)

    def acks(self):
        """Rows whose tail was a watched key: what ``checkackdata`` goes on to mark ``ackreceived``."""
        return np.flatnonzero(self.ack == FOUND)

    def ack_key(self, i):
        return bytes(self._objects[i][16:])

    def msgs(self):
        return np.flatnonzero(self.route == MSG)

    def broadcasts(self):
        return np.flatnonzero(self.route == BROADCAST)

    def pubkeys(self):
        return np.flatnonzero(self.route == PUBKEY)

    def requested_key(self, i):
        """The hash or tag a getpubkey asks for (shorter than 20 / 32 bytes under ``SHORT_*``)."""
        at = int(self.key_off[i])
        return bytes(self._objects[i][at:at + int(self.key_len[i])])

    def pubkey_requests(self):
        """``(row, command, argument)`` per accepted getpubkey, in the reference's form (``:263-268``): the
        requested hash for v2 and v3, for v4 the address row (``address_table[row]``)."""
        out = []
        for i in np.flatnonzero(np.isin(self.status, list(COMMANDS))):
            st = int(self.status[i])
            out.append((int(i), COMMANDS[st], int(self.address[i]) if st == SEND_V4 else self.requested_key(i)))
        return out

    def peers(self):
        """``(row, stream, host_class, host bytes, port)`` per ``PEER`` row; :func:`host_string` formats the
        host."""
        out = []
        for i in np.flatnonzero(self.status == PEER):
            at = int(self.host_off[i])
            out.append((int(i), int(self.stream[i]), int(self.host_class[i]),
                        bytes(self._objects[i][at:at + int(self.host_len[i])]), int(self.port[i])))
        return out


class Dispatcher(object):
    """``state.ackdataForWhichImWatching`` and ``shared.myAddressesByHash`` / ``myAddressesByTag`` behind one
    handle.  ``seed`` picks the watch index's start slots (0: drawn at random).  ``host_only`` makes a dispatcher
    that touches no device: everything works but :meth:`dispatch`.  A device dispatcher belongs to the device
    selection it was made under: after ``_lib.reset()`` every call but :meth:`close` raises ``BmpowError``
    (``E_STATE``)."""

    def __init__(self, seed=0, host_only=False):
        self._lib = _lib.host() if host_only else _lib.get()
        self._h = self._lib.bmpow_proc_create(int(seed), 1 if host_only else 0)
        if not self._h:
            _lib.check(self._lib, _lib.E_HIP, 'bmpow_proc_create')
        self._addresses = np.zeros(0, dtype=ADDRESS_DTYPE)

    def _handle(self):
        if not self._h:
            raise ValueError('the dispatcher is closed')
        return self._h

    def close(self):
        if self._h:
            self._lib.bmpow_proc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __len__(self):
        return int(_lib.check(self._lib, self._lib.bmpow_proc_watch_len(self._handle()), 'bmpow_proc_watch_len'))

    # ---- the watch set ----
    def watch(self, keys, aux=None):
        """``ackdataForWhichImWatching[key] = aux`` for each key (byte strings of any length); a bool array of
        which were new."""
        n, raw, offs = _packed(keys)
        a = None if aux is None else (np.full(n, aux, dtype=np.uint32) if not np.ndim(aux)
                                      else np.ascontiguousarray(aux, dtype=np.uint32))
        if a is not None and len(a) != n:
            raise ValueError('one aux per key')
        added = np.zeros(n, dtype=np.uint8)
        _lib.check(self._lib, self._lib.bmpow_proc_watch_add(self._handle(), n, raw, offs.ctypes.data_as(P64),
                                                             None if a is None else a.ctypes.data, added.ctypes.data),
                   'bmpow_proc_watch_add')
        return added.astype(bool)

    def unwatch(self, keys):
        """``del`` for each key; a bool array of which were watched."""
        n, raw, offs = _packed(keys)
        present = np.zeros(n, dtype=np.uint8)
        _lib.check(self._lib, self._lib.bmpow_proc_watch_discard(self._handle(), n, raw, offs.ctypes.data_as(P64),
                                                                 present.ctypes.data), 'bmpow_proc_watch_discard')
        return present.astype(bool)

    def watching(self, key, aux=False):
        """``key in ackdataForWhichImWatching``; with ``aux`` the pair ``(present, aux)``."""
        n, raw, offs = _packed([key])
        present, a = np.zeros(1, dtype=np.uint8), np.zeros(1, dtype=np.uint32)
        _lib.check(self._lib, self._lib.bmpow_proc_watch_contains(self._handle(), n, raw, offs.ctypes.data_as(P64),
                                                                  present.ctypes.data, a.ctypes.data),
                   'bmpow_proc_watch_contains')
        return (bool(present[0]), int(a[0])) if aux else bool(present[0])

    __contains__ = watching

    def clear(self):
        _lib.check(self._lib, self._lib.bmpow_proc_watch_clear(self._handle()), 'bmpow_proc_watch_clear')

    # ---- my addresses ----
    def set_addresses(self, rows):
        """The whole table: an ``ADDRESS_DTYPE`` array (:func:`address_rows`, :func:`rows_from_addresses`).  Two
        rows with one ripe or one tag raise ``BmpowError`` (``E_ARG``) and leave the table as it was."""
        rows = np.ascontiguousarray(rows, dtype=ADDRESS_DTYPE)
        _lib.check(self._lib, self._lib.bmpow_proc_set_addresses(self._handle(), len(rows),
                                                                 rows.ctypes.data if len(rows) else None),
                   'bmpow_proc_set_addresses')
        self._addresses = rows.copy()

    @property
    def address_table(self):
        return self._addresses

    # ---- the batch ----
    def dispatch(self, objects, types, now=0, rows_per_launch=0):
        """``objectProcessor.run``'s own work for ``objects`` with their ``types`` (one for all or one each; the
        intake record's ``object_type``), in one call.  The ack verdicts are those of a sequential run in row
        order; the ``FOUND`` keys have left the watch set when the call returns."""
        objs = objects if type(objects) is list else list(objects)
        n = len(objs)
        if isinstance(types, np.ndarray) and types.dtype == np.uint32:
            kinds = np.ascontiguousarray(types)
        else:
            kinds = (np.full(n, types, dtype=np.uint32) if not np.ndim(types)
                     else np.ascontiguousarray(np.asarray(types, dtype=np.uint64) & 0xffffffff, dtype=np.uint32))
        if kinds.shape != (n,):
            raise ValueError('one type per object')
        recs = np.zeros(n, dtype=REC_DTYPE)
        params = _lib.BmpowProcParams(int(now), int(rows_per_launch), 0)
        fast = _fast()
        if n and fast is not None and hasattr(fast, 'proc_list'):
            # the list walked in C, the call with the GIL released (csrc/bmpow_pyext.c)
            addr = ctypes.cast(self._lib.bmpow_proc_batch, ctypes.c_void_p).value
            args = (kinds.ctypes.data, ctypes.addressof(params), recs.ctypes.data)
            try:
                rc = fast.proc_list(addr, self._handle(), objs, *args)
            except TypeError:  # bytearray / memoryview items: one bytes copy each
                objs = packets._as_buffers(objs)
                rc = fast.proc_list(addr, self._handle(), objs, *args)
            _lib.check(self._lib, rc, 'bmpow_proc_batch')
        elif n:
            objs = packets._as_buffers(objs)
            ptrs = np.ascontiguousarray(_pointers(objs), dtype=np.uint64)
            lens = np.fromiter(map(len, objs), dtype=np.uint64, count=n)
            _lib.check(self._lib, self._lib.bmpow_proc_batch(self._handle(), n, ptrs.ctypes.data, lens.ctypes.data_as(P64),
                                                             kinds.ctypes.data, ctypes.byref(params), recs.ctypes.data),
                       'bmpow_proc_batch')
        else:  # the state checks of an empty call
            _lib.check(self._lib, self._lib.bmpow_proc_batch(self._handle(), 0, None, None, None, None, None),
                       'bmpow_proc_batch')
        return DispatchResult(objs, kinds, recs, self._addresses)

    def dispatch_packets(self, result, now=0):
        """The accepted objects of a :class:`pybitmessage_amd.packets.PacketResult` or an
        :class:`pybitmessage_amd.intake.IntakeResult` with their recorded types: what the reference puts on the
        ``objectProcessorQueue`` (``bmproto.py:431-435``).  ``DispatchResult.source_index`` names their rows."""
        if isinstance(result, packets.PacketResult):
            index = result.objects()
            objs = [bytes(result.payload(int(i))) for i in index]
            kinds = result.intake.objectType[index]
        else:
            index = result.accepted()
            objs = [bytes(result._objects[int(i)]) for i in index]
            kinds = result.objectType[index]
        out = self.dispatch(objs, kinds if len(index) else 0, now)
        out.source_index = index
        return out

    def stats(self):
        s = _lib.BmpowProcStats()
        _lib.check(self._lib, self._lib.bmpow_proc_stats_get(self._handle(), ctypes.byref(s)), 'bmpow_proc_stats_get')
        return {f: getattr(s, f) for f, _ in s._fields_}

    def reset_stats(self):
        _lib.check(self._lib, self._lib.bmpow_proc_stats_reset(self._handle()), 'bmpow_proc_stats_reset')
