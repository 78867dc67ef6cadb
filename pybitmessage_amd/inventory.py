"""The inventory's hashes on the GPU: ``Inventory()`` and ``missingObjects`` as device-resident sets.

The reference's network thread asks two sets the same question one hash at a time.  ``_command_inv``
(``src/network/bmproto.py:344-367``) tests ``i in Inventory()`` for every announced hash and hands the rest to
``handleReceivedInventory`` (``src/network/objectracker.py:88-99``), which sets ``missingObjects[i]``;
``bm_command_object`` (``:393-435``) runs ``checkAlreadyHave``, stores the object and takes its hash out of
``missingObjects``.  Here both sets are :class:`InventorySet` objects, open-addressing tables on the device
(include/bmpow_inv.h): :func:`check_invs` judges the ``inv`` / ``dinv`` / ``getdata`` packets of a whole flood
in one call, reading the hashes where they lie in the payloads, and :func:`admit` is the step behind
:func:`pybitmessage_amd.intake.check_objects` and :func:`pybitmessage_amd.packets.check_buffers`.  Only the
membership is here: the objects' bytes, the SQL store and the sockets stay with the caller.
No CPU fallback: without the HIP library the calls raise :class:`BmpowUnavailable`.
"""
import ctypes

import numpy as np

from . import _lib, intake, packets
from .verify import P64, _pointers

#: ``state`` of :meth:`InventorySet.add` and of :func:`admit`
ABSENT, PRESENT, ADDED, DUP = 0, 1, 2, 3
#: packet kinds
INV, DINV, GETDATA = 0, 1, 2
KIND_OF_COMMAND = {'inv': INV, 'dinv': DINV, 'getdata': GETDATA}
#: ``InvResult.status`` per packet
OK, MALFORMED, TOO_MANY, IGNORED = 0, 1, 2, 3
#: ``InvResult.item_state`` per item
NOT_HAVE, HAVE, KNOWN, NEW, NEW_AGAIN, SHORT = 0, 1, 2, 3, 4, 5
MAX_OBJECT_COUNT = 50000

VALUE_DTYPE = np.dtype([('expires', '<u8'), ('stream', '<u4'), ('aux', '<u4')])
PKT_DTYPE = np.dtype([('count', '<u8'), ('first_item', '<u4'), ('n_items', '<u4'), ('item_offset', '<u4'),
                      ('status', '<i4')])
assert VALUE_DTYPE.itemsize == ctypes.sizeof(_lib.BmpowInvValue)
assert PKT_DTYPE.itemsize == ctypes.sizeof(_lib.BmpowInvPkt)

#: the intake statuses behind which the reference stores the object: every check passed, ``checkObjectByType``
#: failed (``bmproto.py:414-419``: the exception is swallowed), and a stream we are not in only under
#: ``acceptmismatch`` (``:401-409``); an invalid stream re-raises (``:410-412``)
STORED = (intake.OK, intake.INVALID_FOR_TYPE)
STORED_WITH_MISMATCH = STORED + (intake.UNWANTED_STREAM,)


def _keys(keys):
    """(n, 32) uint8, C-contiguous, from a list of 32-byte strings or an array."""
    if isinstance(keys, np.ndarray):
        arr = np.ascontiguousarray(keys, dtype=np.uint8)
        if arr.ndim != 2 or arr.shape[1] != 32:
            raise ValueError('keys as an array are (n, 32) uint8')
        return arr
    keys = list(keys)
    raw = b''.join(keys)
    if len(raw) != 32 * len(keys) or any(len(k) != 32 for k in keys):
        raise ValueError('every key is 32 bytes')
    return np.frombuffer(raw, dtype=np.uint8).reshape(len(keys), 32)


def _column(value, n, dtype):
    if value is None:
        return None
    if not np.ndim(value):
        return np.full(n, value, dtype=dtype)
    out = np.ascontiguousarray(value, dtype=dtype)
    if len(out) != n:
        raise ValueError('one value per key')
    return out


def _addr(arr):
    return None if arr is None else arr.ctypes.data


def slot_of(seed, log2_slots, key):
    """Host only (``bmpow_invset_slot``): the slot a key's probe starts from."""
    return int(_lib.host().bmpow_invset_slot(int(seed), int(log2_slots), bytes(key)))


class InventorySet(object):
    """A set of 32-byte hashes on the device, each with ``(expires, stream, aux)``.  ``slots`` is a hint: the
    table grows as it fills.  ``seed`` picks the start slots (0: drawn at random).  A set belongs to the device
    selection it was made under: after ``_lib.reset()`` every call but :meth:`close` raises ``BmpowError``
    (``E_STATE``)."""

    def __init__(self, slots=1 << 16, seed=0):
        self._lib = _lib.get()
        self._h = self._lib.bmpow_invset_create(int(slots), int(seed))
        if not self._h:
            _lib.check(self._lib, _lib.E_HIP, 'bmpow_invset_create')

    def _handle(self):
        if not self._h:
            raise ValueError('the set is closed')
        return self._h

    def close(self):
        if self._h:
            self._lib.bmpow_invset_destroy(self._h)
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
        return int(_lib.check(self._lib, self._lib.bmpow_invset_len(self._handle()), 'bmpow_invset_len'))

    def clear(self):
        _lib.check(self._lib, self._lib.bmpow_invset_clear(self._handle()), 'bmpow_invset_clear')

    def add(self, keys, expires=None, stream=None, aux=None):
        """Insert the keys.  Returns ``(state, first)``: per row ``PRESENT`` (in the set before the call),
        ``ADDED`` (the lowest row of this call carrying the key; its value is stored) or ``DUP`` with ``first``
        naming that row -- a sequential insert's answers."""
        k = _keys(keys)
        n = len(k)
        state, first = np.zeros(n, dtype=np.uint8), np.arange(n, dtype=np.uint32)
        e, s, a = _column(expires, n, np.uint64), _column(stream, n, np.uint32), _column(aux, n, np.uint32)
        _lib.check(self._lib, self._lib.bmpow_invset_add(self._handle(), n, k.ctypes.data, _addr(e), _addr(s), _addr(a),
                                                         state.ctypes.data, first.ctypes.data), 'bmpow_invset_add')
        return state, first

    def contains(self, keys, values=False):
        """A bool array; with ``values`` also the ``VALUE_DTYPE`` records (zeros where absent)."""
        k = _keys(keys)
        n = len(k)
        present = np.zeros(n, dtype=np.uint8)
        vals = np.zeros(n, dtype=VALUE_DTYPE) if values else None
        _lib.check(self._lib, self._lib.bmpow_invset_contains(self._handle(), n, k.ctypes.data, present.ctypes.data,
                                                              _addr(vals)), 'bmpow_invset_contains')
        return (present.astype(bool), vals) if values else present.astype(bool)

    def __contains__(self, key):
        return bool(self.contains([bytes(key)])[0])

    def discard(self, keys):
        """Remove the keys; a bool array of which were in the set."""
        k = _keys(keys)
        present = np.zeros(len(k), dtype=np.uint8)
        _lib.check(self._lib, self._lib.bmpow_invset_remove(self._handle(), len(k), k.ctypes.data, present.ctypes.data),
                   'bmpow_invset_remove')
        return present.astype(bool)

    def sweep(self, min_expires):
        """Drop every entry with ``expires < min_expires``; returns what is left."""
        return int(_lib.check(self._lib, self._lib.bmpow_invset_sweep(self._handle(), int(min_expires)),
                              'bmpow_invset_sweep'))

    def clean(self, now):
        """``Inventory.clean`` (``src/storage/sqlite.py:115-120``): ``expirestime < now - 3 h`` leaves."""
        return self.sweep(max(int(now) - 3 * 3600, 0))

    def unexpired_hashes_by_stream(self, stream, now, cap=None):
        """``unexpired_hashes_by_stream`` (``sqlite.py:92-101``): an ``(m, 32)`` uint8 array in no particular
        order.  With ``cap`` at most that many, and the full count beside them: ``(hashes, count)``."""
        size = len(self) if cap is None else int(cap)
        out = np.zeros((size, 32), dtype=np.uint8)
        got = _lib.check(self._lib, self._lib.bmpow_invset_list(self._handle(), int(stream), int(now), _addr(out) if size
                                                                else None, size), 'bmpow_invset_list')
        return out[:min(got, size)] if cap is None else (out[:min(got, size)], int(got))

    def stats(self):
        s = _lib.BmpowInvStats()
        _lib.check(self._lib, self._lib.bmpow_invset_stats(self._handle(), ctypes.byref(s)), 'bmpow_invset_stats')
        return {f: getattr(s, f) for f, _ in s._fields_}


def walk(payload, kind, dandelion=False):
    """Host only (``bmpow_inv_walk``): one payload as ``decode_payload_content("l32s")`` and the handler's
    first checks read it.  Returns the ``BmpowInvPkt``."""
    payload = bytes(payload)
    out = _lib.BmpowInvPkt()
    lib = _lib.host()
    raw = ctypes.cast(ctypes.c_char_p(payload), ctypes.c_void_p)
    _lib.check(lib, lib.bmpow_inv_walk(raw, len(payload), int(kind), int(bool(dandelion)), ctypes.byref(out)),
               'bmpow_inv_walk')
    return out


class InvResult(object):
    """What :func:`check_invs` found.  Per packet: ``status``, ``count`` (the reference's ``len(items)``),
    ``first_item``, ``n_items``, ``item_offset``, ``kind``.  Per item, in packet order then item order:
    ``item_state`` (``HAVE``, ``KNOWN``, ``NEW``, ``NEW_AGAIN``, ``SHORT``; for a ``getdata`` ``HAVE`` or
    ``NOT_HAVE``), ``item_first`` (for ``NEW_AGAIN`` the first item of this call with the same hash) and
    ``item_packet``."""

    def __init__(self, payload_of, kinds, pkts, item_state, item_first):
        self._payload_of = payload_of
        self.kind = kinds
        self.packets = pkts
        self.status, self.count = pkts['status'], pkts['count']
        self.first_item, self.n_items, self.item_offset = pkts['first_item'], pkts['n_items'], pkts['item_offset']
        self.item_state, self.item_first = item_state, item_first
        self.item_packet = np.repeat(np.arange(len(pkts), dtype=np.uint32), pkts['n_items'])

    def __len__(self):
        return len(self.item_state)

    def item(self, j):
        """Item j's bytes, cut from the caller's buffer (fewer than 32 for a ``SHORT`` one)."""
        p = int(self.item_packet[j])
        at = int(self.item_offset[p]) + 32 * (j - int(self.first_item[p]))
        return bytes(self._payload_of(p)[at:at + 32])

    def new_items(self):
        """Indices of the items now first announced: what the reference would go on to request."""
        return np.flatnonzero(self.item_state == NEW)


def check_invs(payloads, kinds, have, missing, now, dandelion=False, commands=('inv', 'dinv', 'getdata')):
    """``_command_inv`` / ``bm_command_getdata``'s membership work for a list of payloads of ``kinds`` (``INV``,
    ``DINV``, ``GETDATA``; one for all or one each) in one call: a lookup in ``have``, then an add into
    ``missing`` with ``expires = now`` for the announced hashes we do not have.  ``payloads`` may instead be a
    :class:`pybitmessage_amd.packets.PacketResult`: its valid packets whose command is in ``commands`` go in
    where they lie in the connection buffers (``kinds`` is then ignored, and ``InvResult.packet_index`` names
    their records).  The Dandelion exception (``i in Inventory() and not Dandelion().hasHash(i)``) and
    ``skipUntil`` stay with the caller."""
    index = None
    if isinstance(payloads, packets.PacketResult):
        res = payloads
        wanted = [packets.COMMANDS.index(c) for c in commands]
        index = np.flatnonzero(np.isin(res.command, wanted) & (res.status == packets.OK))
        bufs = res._buffers
        conn = res.conn[index].astype(np.int64)
        ptrs = (_pointers(bufs)[conn] + res.offset[index].astype(np.uint64) + np.uint64(packets.HEADER_SIZE)
                if len(index) else np.zeros(0, dtype=np.uint64))
        lens = res.length[index].astype(np.uint64)
        kind = np.array([KIND_OF_COMMAND[packets.COMMANDS[c]] for c in res.command[index]], dtype=np.uint8)
        keep = bufs

        def payload_of(p):
            return res.payload(int(index[p]))
    else:
        keep = packets._as_buffers(payloads)
        ptrs = _pointers(keep) if keep else np.zeros(0, dtype=np.uint64)
        lens = np.fromiter(map(len, keep), dtype=np.uint64, count=len(keep))
        kind = (np.full(len(keep), kinds, dtype=np.uint8) if not np.ndim(kinds)
                else np.ascontiguousarray(list(kinds), dtype=np.uint8))
        if len(kind) != len(keep):
            raise ValueError('one kind per payload')

        def payload_of(p):
            return keep[p]
    n = len(lens)
    pkts = np.zeros(n, dtype=PKT_DTYPE)
    ptrs = np.ascontiguousarray(ptrs, dtype=np.uint64)
    host = _lib.host()
    one = _lib.BmpowInvPkt()
    cap = 0
    for p in range(n):  # the walk alone sizes the item arrays (no device)
        _lib.check(host, host.bmpow_inv_walk(int(ptrs[p]) if lens[p] else None, int(lens[p]), int(kind[p]),
                                             int(bool(dandelion)), ctypes.byref(one)), 'bmpow_inv_walk')
        cap += one.n_items
    state, first = np.zeros(cap, dtype=np.uint8), np.zeros(cap, dtype=np.uint32)
    if n:
        lib = _lib.get()
        got = _lib.check(lib, lib.bmpow_inv_batch(have._handle(), missing._handle() if missing is not None else None, n,
                                                  ptrs.ctypes.data, lens.ctypes.data_as(P64), kind.ctypes.data, int(now),
                                                  int(bool(dandelion)), pkts.ctypes.data, _addr(state) if cap else None,
                                                  _addr(first) if cap else None, cap), 'bmpow_inv_batch')
        assert got == cap
    out = InvResult(payload_of, kind, pkts, state, first)
    out.packet_index = index
    return out


def store_mask(status, acceptmismatch=False):
    """The rows ``bm_command_object`` goes on to store (``Inventory()[hash] = ...``, ``bmproto.py:401-435``)."""
    return np.isin(status, STORED_WITH_MISMATCH if acceptmismatch else STORED)


class AdmitResult(object):
    """What :func:`admit` found, one row per intake record: ``already`` (in ``have`` before the call: the
    reference's ``BMObjectAlreadyHaveError``), ``state`` (``ADDED``: stored by this call; ``DUP``: a later copy
    inside the batch, already had by then; ``PRESENT``; ``ABSENT``: not stored) and ``stored`` (the mask)."""

    def __init__(self, already, state, stored):
        self.already, self.state, self.stored = already, state, stored

    def added(self):
        return np.flatnonzero(self.state == ADDED)


def admit(result, have, missing, acceptmismatch=False):
    """The step behind the intake for an :class:`pybitmessage_amd.intake.IntakeResult` (or a ``PacketResult``,
    whose ``intake`` is taken): ``checkAlreadyHave`` against ``have`` for the rows that reach it, the store of
    the rows :func:`store_mask` names with the record's ``expires`` and ``stream`` (``aux`` = the row), and the
    hash of every looked-up row out of ``missing``."""
    objects = None
    if isinstance(result, packets.PacketResult):  # its other packets carry zeroed records: they take no part
        objects = (result.command == packets.OBJECT) & (result.status == packets.OK)
        result = result.intake
    recs = result.records
    n = len(recs)
    stored = store_mask(recs['status'], acceptmismatch).astype(np.uint8)
    if objects is not None:
        stored[~objects] = 2  # BMPOW_INV_ADMIT_SKIP
    already, state = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
    if n:
        lib = _lib.get()
        stride = recs.strides[0]
        _lib.check(lib, lib.bmpow_inv_admit(have._handle(), missing._handle() if missing is not None else None, n,
                                            recs.ctypes.data, stride, stored.ctypes.data, already.ctypes.data,
                                            state.ctypes.data), 'bmpow_inv_admit')
    return AdmitResult(already.astype(bool), state, stored == 1)
