"""Addresses, and who sent an object: the reference's ``src/addresses.py`` with its batch forms on the GPU.

Once a signature has verified, the reference hashes the sender's two public keys into the ripe
(``RIPEMD160(SHA512(pubSigningKey || pubEncryptionKey))``, ``src/class_objectProcessor.py:877-879``,
``src/protocol.py:493-495``) and turns it into the ``BM-`` address it stores (``encodeAddress``,
``src/addresses.py:146-180``), or into the tag it compares (``:889-893``); subscriptions and needed pubkeys
derive their keys from the same bytes (``src/shared.py:162-184``, ``src/class_singleWorker.py:84-90``).
``bmpow_ident_derive`` / ``bmpow_ident_from_ripe`` (``include/bmpow_ident.h``) run all of that for a batch,
one lane per row: :func:`derive_batch`, :func:`encode_batch`, :func:`address_keys`.

The single-value forms are host code restated from the reference (those ``addressgen`` already has are
re-exported).  The batch forms have no CPU fallback: without the HIP library they raise
:class:`BmpowUnavailable`.
"""
import ctypes
import hashlib

import numpy as np

from . import _lib
from .addressgen import ALPHABET, encodeAddress, encodeBase58, encodeVarint  # noqa: F401 -- re-exported
from .ecies import _varint
from .signatures import _key64

_P64 = ctypes.POINTER(ctypes.c_uint64)
U64_MAX = (1 << 64) - 1

#: one ``bmpow_ident_rec`` (include/bmpow_ident.h)
REC = np.dtype([('ripe', np.uint8, 20), ('key_v3', np.uint8, 32), ('tag_key', np.uint8, 32), ('tag', np.uint8, 32),
                ('addr_len', np.uint8), ('addr', 'S63')])
assert REC.itemsize == ctypes.sizeof(_lib.BmpowIdentRec) == 180


class varintDecodeError(Exception):
    """``addresses.varintDecodeError``."""


def decodeVarint(data):
    """``addresses.decodeVarint`` (``src/addresses.py:82-134``): ``(value, length)``; ``(0, 0)`` for empty
    input; raises :class:`varintDecodeError` for a truncated or not minimally encoded varint."""
    res = _varint(bytes(data))
    if res is None:
        raise varintDecodeError('truncated varint, or not encoded with the lowest possible number of bytes')
    return res


def decodeBase58(string):
    """``addresses.decodeBase58`` (``src/addresses.py:36-53``): 0 for a character outside the alphabet."""
    num = 0
    for char in string:
        digit = ALPHABET.find(char)
        if digit < 0:
            return 0
        num = num * 58 + digit
    return num


def calculateInventoryHash(data):
    """``addresses.calculateInventoryHash`` (``src/addresses.py:137-143``)."""
    return hashlib.sha512(hashlib.sha512(data).digest()).digest()[0:32]


def decodeAddress(address):
    """``addresses.decodeAddress`` (``src/addresses.py:183-277``): ``(status, version, stream, ripe)`` with
    every status string of the reference; where the status is not ``'success'`` the rest is ``0, 0, b''``
    (the reference returns ``''`` there)."""
    if isinstance(address, bytes):
        address = address.decode('ascii', 'replace')
    address = str(address).strip()
    integer = decodeBase58(address[3:] if address[:3] == 'BM-' else address)
    if integer == 0:
        return 'invalidcharacters', 0, 0, b''
    data = integer.to_bytes((integer.bit_length() + 7) // 8, 'big')
    if data[-4:] != hashlib.sha512(hashlib.sha512(data[:-4]).digest()).digest()[0:4]:
        return 'checksumfailed', 0, 0, b''
    ver = _varint(data[:9])
    if ver is None:
        return 'varintmalformed', 0, 0, b''
    version, used = ver
    if version > 4 or version == 0:
        return 'versiontoohigh', 0, 0, b''
    st = _varint(data[used:])
    if st is None:
        return 'varintmalformed', 0, 0, b''
    stream, used2 = st
    if version == 1:
        return 'success', version, stream, data[-24:-4]
    ripe = data[used + used2:-4]
    if version in (2, 3):
        if len(ripe) in (18, 19, 20):
            return 'success', version, stream, ripe.rjust(20, b'\x00')
        if len(ripe) < 18:
            return 'ripetooshort', 0, 0, b''
        return 'ripetoolong', 0, 0, b''
    if ripe[0:1] == b'\x00':
        return 'encodingproblem', 0, 0, b''  # non-malleability: the zero bytes must have been removed
    if len(ripe) > 20:
        return 'ripetoolong', 0, 0, b''
    if len(ripe) < 4:
        return 'ripetooshort', 0, 0, b''
    return 'success', version, stream, ripe.rjust(20, b'\x00')


class Identified(object):
    """A batch's records (``bmpow_ident_rec``).  The columns ``ripe``, ``key_v3``, ``tag_key`` and ``tag``
    are ``uint8`` arrays of shape (n, 20) / (n, 32); ``address(i)`` / ``addresses()`` give the ``BM-``
    strings."""

    def __init__(self, recs):
        self.recs = recs
        self.ripe, self.key_v3, self.tag_key, self.tag = recs['ripe'], recs['key_v3'], recs['tag_key'], recs['tag']

    def __len__(self):
        return len(self.recs)

    def address(self, i):
        r = self.recs[i]
        return 'BM-' + bytes(r['addr'])[:int(r['addr_len'])].decode('ascii')

    def addresses(self):
        # numpy drops an 'S' field's trailing zero bytes, which is all that stands behind addr_len characters
        return ['BM-' + a.decode('ascii') for a in self.recs['addr'].tolist()]


def _u64_column(values, n, what):
    if isinstance(values, np.ndarray) and values.dtype == np.uint64:
        arr = np.ascontiguousarray(values)
    else:
        vals = list(values)
        if any(not 0 <= int(v) <= U64_MAX for v in vals):
            raise ValueError('%s must be below 2^64 (encodeVarint raises above)' % what)
        arr = np.array(vals, dtype=np.uint64)
    if arr.shape != (n,):
        raise ValueError('one %s per row' % what)
    return arr


def _rows(data, width, what):
    """(n, width) uint8, from such an array or from a list of byte strings."""
    if isinstance(data, np.ndarray) and data.dtype == np.uint8 and data.ndim == 2 and data.shape[1] == width:
        return np.ascontiguousarray(data)
    items = [bytes(d) for d in data]
    if any(len(d) != width for d in items):
        raise ValueError('%s are %d bytes each' % (what, width))
    return np.frombuffer(b''.join(items), dtype=np.uint8).reshape(len(items), width)


def _keys(keys):
    if isinstance(keys, np.ndarray):
        return _rows(keys, 64, 'public keys')
    out = [_key64(k) for k in keys]
    if any(k is None for k in out):
        raise ValueError('public keys are 64 bytes (X || Y) or 65 (04 || X || Y)')
    return _rows(out, 64, 'public keys')


def _run(name, rows, versions, streams):
    n = len(rows)
    versions, streams = _u64_column(versions, n, 'version'), _u64_column(streams, n, 'stream')
    recs = np.zeros(n, dtype=REC)
    lib = _lib.get()
    _lib.check(lib, getattr(lib, name)(n, rows.ctypes.data, versions.ctypes.data_as(_P64),
                                       streams.ctypes.data_as(_P64), recs.ctypes.data), name)
    return Identified(recs)


def derive_batch(pub_signing, pub_encryption, versions, streams):
    """Per (signing key, encryption key, address version, stream) the sender's ripe, the keys and the tag
    derived from it and the address, on the device (``bmpow_ident_derive``).  Keys are 64 bytes (``X ||
    Y``) or 65 (``04 || X || Y``) as :func:`signatures.verify_batch` takes them, or ``uint8`` arrays of
    shape (n, 64); anything else raises ``ValueError``."""
    ks, ke = _keys(pub_signing), _keys(pub_encryption)
    if len(ks) != len(ke):
        raise ValueError('one encryption key per signing key')
    return _run('bmpow_ident_derive', np.ascontiguousarray(np.concatenate([ks, ke], axis=1)), versions, streams)


def encode_batch(versions, streams, ripes):
    """``encodeAddress`` for a batch (``bmpow_ident_from_ripe``), with the keys and tags of each address in
    the result's other columns.  Ripes are 20 bytes each, whatever the version."""
    return _run('bmpow_ident_from_ripe', _rows(ripes, 20, 'ripes'), versions, streams)


def address_keys(addresses):
    """Per address ``(status, version, stream, ripe, lookup_key, privkey)``: the address decoded on the
    host, and what subscriptions and needed pubkeys are kept under, derived on the device
    (``src/shared.py:162-184``, ``src/class_singleWorker.py:84-90``): ``ripe`` and ``SHA512(data)[:32]`` up
    to version 3, the tag and ``SHA512(SHA512(data))[:32]`` from version 4, with ``data = varint(version)
    || varint(stream) || ripe``.  An address that does not decode gives ``(status, 0, 0, b'', None, None)``."""
    decoded = [decodeAddress(a) for a in addresses]
    live = [i for i, d in enumerate(decoded) if d[0] == 'success']
    out = [d + (None, None) for d in decoded]
    if live:
        res = encode_batch([decoded[i][1] for i in live], [decoded[i][2] for i in live], [decoded[i][3] for i in live])
        for j, i in enumerate(live):
            if decoded[i][1] <= 3:
                out[i] = decoded[i] + (decoded[i][3], res.key_v3[j].tobytes())
            else:
                out[i] = decoded[i] + (res.tag[j].tobytes(), res.tag_key[j].tobytes())
    return out


def stats():
    """The library's identification counters (``bmpow_ident_stats``) as a dict."""
    lib = _lib.get()
    st = _lib.BmpowIdentStats()
    _lib.check(lib, lib.bmpow_ident_get_stats(ctypes.byref(st)), 'bmpow_ident_get_stats')
    return {f: getattr(st, f) for f, _ in st._fields_}


def reset_stats():
    _lib.get().bmpow_ident_reset_stats()
