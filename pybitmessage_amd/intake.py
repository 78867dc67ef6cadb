"""Batched object intake on the GPU: ``network/bmobject.py`` for a whole flood.

The reference's network thread builds a ``BMObject`` for every received object
(``src/network/bmproto.py:377-441``): it decodes the header ``QQIvv``, computes
``calculateInventoryHash(data)`` (``src/addresses.py:137-143``), checks the proof of work and
runs the EOL, stream and per-type checks of ``src/network/bmobject.py:71-163``.  Here
:func:`check_objects` does that for a list of objects with one upload and one launch per shard
(``bmpow_intake_batch``, include/bmpow_intake.h), and :func:`inventory_hashes` gives the hashes
alone.  The already-have lookup (``checkAlreadyHave``) and the store behind it are
:func:`pybitmessage_amd.inventory.admit`, which takes the :class:`IntakeResult` as it is.  No CPU fallback: without the HIP library the calls raise :class:`BmpowUnavailable`.
"""
import ctypes

import numpy as np

from . import _lib
from .verify import P64, _fast, _pointers

#: every check passed: the object goes to the ``objectProcessorQueue``
OK = 0
#: the header does not decode (``struct.error`` / ``addresses.varintDecodeError``)
MALFORMED = 1
#: ``BMProtoExcessiveDataError``: more than 2**18 bytes after the header
TOO_LARGE = 2
#: ``BMObjectInsufficientPOWError``
INSUFFICIENT_POW = 3
#: ``BMObjectExpiredError``: end of life more than 28 days 3 hours ahead
EXPIRED_FUTURE = 4
#: ``BMObjectExpiredError``: end of life more than an hour ago
EXPIRED_PAST = 5
#: ``BMObjectInvalidError`` from ``checkStream``: stream 0 or above 2**63 - 1
INVALID_STREAM = 6
#: ``BMObjectUnwantedStreamError``
UNWANTED_STREAM = 7
#: ``BMObjectInvalidError`` from ``checkObjectByType``
INVALID_FOR_TYPE = 8

STATUS_NAMES = {OK: 'OK', MALFORMED: 'MALFORMED', TOO_LARGE: 'TOO_LARGE', INSUFFICIENT_POW: 'INSUFFICIENT_POW',
                EXPIRED_FUTURE: 'EXPIRED_FUTURE', EXPIRED_PAST: 'EXPIRED_PAST', INVALID_STREAM: 'INVALID_STREAM',
                UNWANTED_STREAM: 'UNWANTED_STREAM', INVALID_FOR_TYPE: 'INVALID_FOR_TYPE'}

#: ``bmpow_intake_rec`` as a numpy record
REC_DTYPE = np.dtype([('nonce', '<u8'), ('expires', '<u8'), ('version', '<u8'), ('stream', '<u8'), ('pow', '<u8'),
                      ('object_type', '<u4'), ('payload_offset', '<u4'), ('status', '<i4'), ('reserved', '<u4'),
                      ('inv', 'u1', (32,))])
assert REC_DTYPE.itemsize == ctypes.sizeof(_lib.BmpowIntakeRec)


def _as_bytes(objects):
    objs = objects if type(objects) is list else list(objects)
    if set(map(type, objs)) - {bytes}:  # bytearray / memoryview: one bytes copy each
        objs = [o if type(o) is bytes else bytes(o) for o in objs]
    return objs


def inventory_hashes(objects):
    """``[calculateInventoryHash(o) for o in objects]`` with one GPU launch per shard.  An object
    shorter than its 8-byte nonce is an argument error (``BmpowError``, code ``E_ARG``)."""
    objs = _as_bytes(objects)
    n = len(objs)
    if n == 0:
        return []
    lib = _lib.get()
    ptrs = _pointers(objs)
    lens = np.fromiter(map(len, objs), dtype=np.uint64, count=n)
    out = np.zeros((n, 32), dtype=np.uint8)
    _lib.check(lib, lib.bmpow_inventory_hashes(n, ptrs.ctypes.data, lens.ctypes.data_as(P64),
                                               out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))),
               'bmpow_inventory_hashes')
    del objs  # the pointers were valid for the call
    raw = out.tobytes()
    return [raw[32 * i:32 * i + 32] for i in range(n)]


class IntakeResult(object):
    """What :func:`check_objects` found, one row per object: numpy columns named as the
    ``BMObject`` attributes they stand for."""

    def __init__(self, objects, recs):
        self._objects = objects
        self.records = recs
        self.inventoryHash = recs['inv']          # (n, 32) uint8
        self.status = recs['status']
        self.expiresTime = recs['expires']
        self.objectType = recs['object_type']
        self.version = recs['version']
        self.streamNumber = recs['stream']
        self.payloadOffset = recs['payload_offset']
        self.pow = recs['pow']

    def __len__(self):
        return len(self.records)

    def inventory_hash(self, i):
        """Object i's inventory hash as 32 bytes."""
        return self.inventoryHash[i].tobytes()

    def tag(self, i):
        """``BMObject.tag``: ``data[payloadOffset:payloadOffset + 32]``."""
        off = int(self.payloadOffset[i])
        return bytes(self._objects[i][off:off + 32])

    def accepted(self):
        """Indices of the objects every check passed."""
        return np.flatnonzero(self.status == OK)


def check_objects(objects, streams=(1,), nonceTrialsPerByte=0, payloadLengthExtraBytes=0, recvTime=0, now=0):
    """``bm_command_object``'s per-object work for a list of objects: header, inventory hash, proof
    of work at (``nonceTrialsPerByte``, ``payloadLengthExtraBytes``, ``recvTime``) and the sanity
    checks against ``streams`` (``state.streamsInWhichIAmParticipating``) and ``now``
    (``int(time.time())``; 0 = the clock).  Returns an :class:`IntakeResult`; ``status`` holds the
    first check that failed, in the reference's order."""
    objs = objects if type(objects) is list else list(objects)
    n = len(objs)
    if n == 0:
        return IntakeResult(objs, np.zeros(0, dtype=REC_DTYPE))
    lib = _lib.get()
    recs = np.empty(n, dtype=REC_DTYPE)  # the library writes every record
    st = np.ascontiguousarray(np.asarray(list(streams), dtype=np.uint64))
    prm = _lib.BmpowIntakeParams(int(now), int(recvTime), int(nonceTrialsPerByte), int(payloadLengthExtraBytes),
                                 st.ctypes.data_as(P64), len(st))
    fast = _fast()
    if fast is not None and hasattr(fast, 'intake_list'):
        # the list walked in C, the call with the GIL released (csrc/bmpow_pyext.c)
        addr = ctypes.cast(lib.bmpow_intake_batch, ctypes.c_void_p).value
        try:
            rc = fast.intake_list(addr, objs, ctypes.addressof(prm), recs.ctypes.data)
        except TypeError:  # bytearray / memoryview items: one bytes copy each
            objs = _as_bytes(objs)
            rc = fast.intake_list(addr, objs, ctypes.addressof(prm), recs.ctypes.data)
        _lib.check(lib, rc, 'bmpow_intake_batch')
        return IntakeResult(objs, recs)
    objs = _as_bytes(objs)
    ptrs = _pointers(objs)
    lens = np.fromiter(map(len, objs), dtype=np.uint64, count=n)
    _lib.check(lib, lib.bmpow_intake_batch(n, ptrs.ctypes.data, lens.ctypes.data_as(P64), ctypes.byref(prm),
                                           recs.ctypes.data), 'bmpow_intake_batch')
    return IntakeResult(objs, recs)


def header(obj):
    """Host only.  The decoded header of one object as a ``BmpowIntakeRec``, or None where the
    reference's ``decode_payload_content("QQIvv")`` raises."""
    obj = bytes(obj)
    rec = _lib.BmpowIntakeRec()
    if _lib.host().bmpow_intake_header(obj, len(obj), ctypes.byref(rec)) != 1:
        return None
    return rec


def status_of(rec, length, pow_ok, now, streams=(1,)):
    """Host only.  ``bmpow_intake_status``: the first failing check for a decoded header."""
    st = (ctypes.c_uint64 * max(len(streams), 1))(*streams)
    return _lib.host().bmpow_intake_status(ctypes.byref(rec), length, int(bool(pow_ok)), int(now), st, len(streams))


def stats():
    s = _lib.BmpowIntakeStats()
    lib = _lib.get()
    _lib.check(lib, lib.bmpow_intake_get_stats(ctypes.byref(s)), 'bmpow_intake_get_stats')
    return {f: getattr(s, f) for f, _ in s._fields_}


def reset_stats():
    _lib.get().bmpow_intake_reset_stats()
