"""Outgoing msgs, broadcasts and pubkeys from their fields to the finished payload, in one call on the device.

The mirror of :mod:`receive`.  ``class_singleWorker`` signs, encrypts and hashes every object it sends one
at a time: ``sendMsg`` (``src/class_singleWorker.py:1224-1276``), ``sendBroadcast`` (``:641-681``),
``sendOutOrStoreMyV4Pubkey`` (``:420-465``) and ``sendOutOrStoreMyV3Pubkey`` (``:342-378``).  All four have
one shape::

    head = pack('>Q', embeddedTime) + objectType + varint(version) + varint(stream) [+ tag]
    sig  = sign(head + body);   tail = varint(len(sig)) + sig
    payload = head + encrypt(body + tail)      (SEALED: msg, broadcast, v4 pubkey)
    payload = head + body + tail               (CLEAR: v3 pubkey)
    initialHash = sha512(payload)

:func:`build_objects` (``bmpow_tx_objects``, ``include/bmpow_tx.h``) takes heads and bodies and returns the
payloads and their ``initialHash``: the bytes go up once, and the padding, both digests, the signing
equation, DER, the ECIES key agreement, AES-256-CBC, HMAC-SHA256 and the payload's SHA-512 run on the
device.  :func:`build_msgs`, :func:`build_broadcasts` and :func:`build_pubkeys` assemble head and body from
fields.  Nonces, ephemeral keys and IVs come from libcrypto's ``RAND_bytes`` unless the caller supplies
them.  No CPU fallback: without the HIP library the calls raise :class:`BmpowUnavailable`.
"""
import collections
import ctypes
from struct import pack

import numpy as np

from . import _lib, addresses, sender, worker
from .ecies import _key32
from .sender import DIGESTS
from .signatures import _key64
from .worker import _varint

_P64 = ctypes.POINTER(ctypes.c_uint64)

SEALED, CLEAR = 0, 1  # BMPOW_TX_SEALED / BMPOW_TX_CLEAR
OK, BAD_RECIPIENT, NO_SIGNATURE, TOO_LARGE = 0, 1, 2, 3  # BMPOW_TX_*
HEAD_MIN, HEAD_MAX, MAX_BODY = 12, 62, 2 ** 18

REC = np.dtype([('status', np.int32), ('obj_len', np.uint32), ('plain_len', np.uint32), ('sig_len', np.uint8),
                ('kind', np.uint8), ('digest', np.uint8), ('reserved', np.uint8), ('sig', np.uint8, 72),
                ('initial_hash', np.uint8, 64)])
assert REC.itemsize == ctypes.sizeof(_lib.BmpowTxRec) == 152

_NO_POINT = b'\xff' * 64  # a coordinate >= p: what a recipient key of another size is handed on as
_ONE = b'\x00' * 31 + b'\x01'


def obj_cap(head_len, body_len):
    """``BMPOW_TX_OBJ_CAP``: the bound on a payload of either kind."""
    return head_len + sender.blob_cap(body_len + 73)


def layout_row(head_len, body_len):
    """Where a row's pieces lie in its slot of the device pool (``bmpow_tx_layout_row``, host only), as a
    dict: ``slot_bytes``, ``body_at``, ``tail_at``, ``plain_cap``, ``signed_len``, ``hash_blocks``."""
    lib = _lib.host()
    lay = _lib.BmpowTxLayout()
    _lib.check(lib, lib.bmpow_tx_layout_row(int(head_len), int(body_len), ctypes.byref(lay)), 'bmpow_tx_layout_row')
    return {f: getattr(lay, f) for f, _ in lay._fields_ if f != 'reserved'}


class BuiltObjects(object):
    """A batch's records (``bmpow_tx_rec``) beside the payloads.  ``status``, ``kind``, ``digest``, ``obj_len``
    and ``plain_len`` are numpy columns.  ``payload(i)`` and ``initial_hash(i)`` belong to rows whose status is
    ``OK`` (None otherwise); ``signature(i)`` is None only for ``NO_SIGNATURE`` and for rows refused before the
    device."""

    def __init__(self, recs, arena, offs):
        self.recs, self._arena, self._offs = recs, arena, offs
        self.status, self.kind, self.digest = recs['status'], recs['kind'], recs['digest']
        self.obj_len, self.plain_len = recs['obj_len'], recs['plain_len']

    def __len__(self):
        return len(self.recs)

    def payload(self, i):
        if self.recs[i]['status'] != OK:
            return None
        a = int(self._offs[i])
        return self._arena[a:a + int(self.recs[i]['obj_len'])].tobytes()

    def signature(self, i):
        n = int(self.recs[i]['sig_len'])
        return self.recs[i]['sig'][:n].tobytes() if n else None

    def initial_hash(self, i):
        return self.recs[i]['initial_hash'].tobytes() if self.recs[i]['status'] == OK else None

    def accepted(self):
        """The rows that go on to their proof of work."""
        return [int(i) for i in np.flatnonzero(self.status == OK)]


def _as_bytes(items):
    return [x if type(x) is bytes else bytes(x) for x in items]


def build_objects(kinds, heads, bodies, privkeys, pubkeys, digestalg='sha256', nonces=None, ephemeral=None, ivs=None):
    """The raw call (``bmpow_tx_objects``): per row its kind (``SEALED`` / ``CLEAR``), head (12 .. 62 bytes),
    body, the private signing key (32 raw bytes, or fewer as ``BN_bn2bin`` leaves them) and the recipient's
    public encryption key (64 or 65 raw bytes or their hex; ignored, and may be None, for ``CLEAR``), as a
    :class:`BuiltObjects`.  A recipient key of another size, with a coordinate >= p or off the curve gives
    ``BAD_RECIPIENT``; a payload that makes an object above 2^18 bytes ``TOO_LARGE``.  ``nonces``,
    ``ephemeral`` (private keys) and ``ivs`` (16 bytes each) fix the random inputs (tests); by default they are
    drawn.  A signing key or a supplied nonce or ephemeral key that is 0 or >= n raises."""
    if digestalg not in DIGESTS:
        raise ValueError('Unknown digest algorithm %s' % digestalg)
    kinds = [int(k) for k in kinds]
    n = len(kinds)
    if not (n == len(heads) == len(bodies) == len(privkeys) == len(pubkeys)):
        raise ValueError('one kind, head, body, signing key and recipient key per object')
    for opt in (nonces, ephemeral, ivs):
        if opt is not None and len(opt) != n:
            raise ValueError('one nonce, one ephemeral key and one IV per object')
    if any(k not in (SEALED, CLEAR) for k in kinds):
        raise ValueError('a kind is SEALED or CLEAR')
    hs, bs = _as_bytes(heads), _as_bytes(bodies)
    if any(not HEAD_MIN <= len(h) <= HEAD_MAX for h in hs):
        raise ValueError('a head is %d to %d bytes' % (HEAD_MIN, HEAD_MAX))
    priv = b''.join(_key32(k) for k in privkeys)
    pub = b''.join(((None if k is None else _key64(k)) or _NO_POINT) if kind == SEALED else bytes(64)
                   for kind, k in zip(kinds, pubkeys))
    ks = None if nonces is None else b''.join(_key32(k) for k in nonces)
    eph = None if ephemeral is None else b''.join(_key32(e) if kind == SEALED else _ONE for kind, e in zip(kinds, ephemeral))
    iv = None if ivs is None else b''.join(bytes(v) if kind == SEALED else bytes(16) for kind, v in zip(kinds, ivs))
    if iv is not None and len(iv) != 16 * n:
        raise ValueError('IVs are 16 bytes each')
    recs = np.zeros(n, dtype=REC)
    if n == 0:
        return BuiltObjects(recs, np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64))
    hl = np.fromiter(map(len, hs), dtype=np.uint64, count=n)
    bl = np.fromiter(map(len, bs), dtype=np.uint64, count=n)
    caps = np.where(bl > MAX_BODY, 0, hl + 118 + 16 * ((bl + 73) // 16 + 1)).astype(np.uint64)
    offs = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(caps, out=offs[1:])
    arena = np.zeros(max(int(offs[-1]), 1), dtype=np.uint8)
    ptrs = (arena.ctypes.data + offs[:-1]).astype(np.uint64)
    lib = _lib.get()
    hp = (ctypes.c_char_p * n)(*hs)
    bp = (ctypes.c_char_p * n)(*bs)
    _lib.check(lib, lib.bmpow_tx_objects(n, bytes(kinds), ctypes.cast(hp, ctypes.c_void_p), hl.astype(np.uint8).tobytes(),
                                         ctypes.cast(bp, ctypes.c_void_p), bl.ctypes.data_as(_P64), priv, pub,
                                         DIGESTS[digestalg], ks, eph, iv, ptrs.ctypes.data_as(ctypes.c_void_p),
                                         caps.ctypes.data_as(_P64), recs.ctypes.data), 'bmpow_tx_objects')
    return BuiltObjects(recs, arena, offs)


# ---------------------------------------------------------------------------------------------------------
# head and body per kind, from fields
# ---------------------------------------------------------------------------------------------------------
MsgFields = collections.namedtuple('MsgFields', [
    'embeddedTime', 'toStream', 'fromVersion', 'fromStream', 'bitfield', 'pubSigningKey', 'pubEncryptionKey', 'toRipe',
    'encoding', 'message', 'fullAckPayload', 'ntpb', 'extra', 'privSigningKey', 'recipientKey'])
BroadcastFields = collections.namedtuple('BroadcastFields', [
    'embeddedTime', 'version', 'stream', 'ripe', 'bitfield', 'pubSigningKey', 'pubEncryptionKey', 'encoding', 'message',
    'ntpb', 'extra', 'privSigningKey'])
PubkeyFields = collections.namedtuple('PubkeyFields', [
    'embeddedTime', 'version', 'stream', 'ripe', 'bitfield', 'pubSigningKey', 'pubEncryptionKey', 'ntpb', 'extra',
    'privSigningKey'])


def msg_head(embedded_time, stream):
    """A msg object's bytes in front of the encrypted blob (``:1224``, ``:1252-1254``)."""
    return pack('>Q', embedded_time) + b'\x00\x00\x00\x02' + _varint(1) + _varint(stream)


def broadcast_head(embedded_time, version, stream, tag=b''):
    """A broadcast's (``:606-623``): broadcast version 4 for address versions up to 3, 5 with the tag."""
    head = pack('>Q', embedded_time) + b'\x00\x00\x00\x03' + _varint(4 if version <= 3 else 5) + _varint(stream)
    return head + (bytes(tag) if version >= 4 else b'')


def pubkey_head(embedded_time, version, stream, tag=b''):
    """A pubkey's (``:343-346``, ``:418-421`` and ``:456``): with the tag from address version 4."""
    head = pack('>Q', embedded_time) + b'\x00\x00\x00\x01' + _varint(version) + _varint(stream)
    return head + (bytes(tag) if version >= 4 else b'')


def build_msgs(msgs, digestalg='sha256', nonces=None, ephemeral=None, ivs=None):
    """``sendMsg`` from ``:1136`` to ``:1275`` for :class:`MsgFields` rows: the head of :func:`msg_head`, the
    body of :func:`worker.msg_plaintext`, sealed to ``recipientKey``."""
    msgs = list(msgs)
    heads = [msg_head(m.embeddedTime, m.toStream) for m in msgs]
    bodies = [worker.msg_plaintext(m.fromVersion, m.fromStream, m.bitfield, m.pubSigningKey, m.pubEncryptionKey, m.toRipe,
                                   m.encoding, m.message, m.fullAckPayload or b'', m.ntpb, m.extra) for m in msgs]
    return build_objects([SEALED] * len(msgs), heads, bodies, [m.privSigningKey for m in msgs],
                         [m.recipientKey for m in msgs], digestalg, nonces, ephemeral, ivs)


def _address_points(versions, streams, ripes):
    """Per address the tag and the public key its broadcasts and pubkeys are encrypted to: the point of
    ``SHA512(data)[:32]`` up to version 3, of ``SHA512(SHA512(data))[:32]`` from version 4 (``:452-464``,
    ``:655-663``), both derived in batches on the device."""
    if not versions:
        return [], []
    ident = addresses.encode_batch(versions, streams, ripes)
    privs = [(ident.key_v3 if v <= 3 else ident.tag_key)[i].tobytes() for i, v in enumerate(versions)]
    return [ident.tag[i].tobytes() for i in range(len(versions))], sender.priv_to_pub(privs)


def build_broadcasts(broadcasts, digestalg='sha256', nonces=None, ephemeral=None, ivs=None):
    """``sendBroadcast`` from ``:606`` to ``:665`` for :class:`BroadcastFields` rows: the head of
    :func:`broadcast_head`, the body of :func:`worker.broadcast_plaintext`, sealed to the key derived from the
    sender's own address."""
    bcs = list(broadcasts)
    tags, points = _address_points([b.version for b in bcs], [b.stream for b in bcs],
                                   [bytes(b.ripe).rjust(20, b'\x00') for b in bcs])
    heads = [broadcast_head(b.embeddedTime, b.version, b.stream, tag) for b, tag in zip(bcs, tags)]
    bodies = [worker.broadcast_plaintext(b.version, b.stream, b.bitfield, b.pubSigningKey, b.pubEncryptionKey, b.encoding,
                                         b.message, b.ntpb, b.extra) for b in bcs]
    return build_objects([SEALED] * len(bcs), heads, bodies, [b.privSigningKey for b in bcs], points, digestalg, nonces,
                         ephemeral, ivs)


def build_pubkeys(pubkeys, digestalg='sha256', nonces=None, ephemeral=None, ivs=None):
    """``sendOutOrStoreMyV3Pubkey`` (``:343-373``, clear) and ``sendOutOrStoreMyV4Pubkey`` (``:418-466``, sealed
    to the key derived from the address) for :class:`PubkeyFields` rows of address version 3 or 4.  A v2 pubkey
    carries no signature: :func:`worker.pubkey_object` builds it."""
    pks = list(pubkeys)
    if any(p.version not in (3, 4) for p in pks):
        raise ValueError('a signed pubkey is of address version 3 or 4')
    v4 = [i for i, p in enumerate(pks) if p.version == 4]
    tags, points = _address_points([4] * len(v4), [pks[i].stream for i in v4],
                                   [bytes(pks[i].ripe).rjust(20, b'\x00') for i in v4])
    tag_of, point_of = dict(zip(v4, tags)), dict(zip(v4, points))
    heads = [pubkey_head(p.embeddedTime, p.version, p.stream, tag_of.get(i, b'')) for i, p in enumerate(pks)]
    bodies = [worker.pubkey_plaintext(p.bitfield, p.pubSigningKey, p.pubEncryptionKey, p.ntpb, p.extra) for p in pks]
    return build_objects([SEALED if p.version == 4 else CLEAR for p in pks], heads, bodies,
                         [p.privSigningKey for p in pks], [point_of.get(i) for i in range(len(pks))], digestalg, nonces,
                         ephemeral, ivs)


def stats():
    """The counters of ``bmpow_tx_objects`` (``bmpow_tx_stats``) as a dict."""
    lib = _lib.get()
    st = _lib.BmpowTxStats()
    _lib.check(lib, lib.bmpow_tx_get_stats(ctypes.byref(st)), 'bmpow_tx_get_stats')
    return {f: getattr(st, f) for f, _ in st._fields_}


def reset_stats():
    _lib.get().bmpow_tx_reset_stats()
