"""Batched ECDSA signature verification of received objects on the GPU.

The reference checks every v3 / v4 pubkey, every decrypted msg and every broadcast it receives with
``highlevelcrypto.verify`` (``src/highlevelcrypto.py:88-108``): two ``pyelliptic.ECC.verify`` calls
(``src/pyelliptic/ecc.py:387-440``), one under SHA-1 and then, unless that passed, one under SHA-256.
Here ``bmpow_sig_verify`` (``include/bmpow_sig.h``) runs a whole batch on the device: both digests of
every message in one pass, the scalars mod the group order, and one variable-base multiplication per
signature that serves both digests.  No CPU fallback: without the HIP library the calls raise
:class:`BmpowUnavailable`.
"""
import collections
import ctypes

import numpy as np

from . import _lib
from .addressgen import encodeVarint
from .ecies import _varint

_PU8 = ctypes.POINTER(ctypes.c_uint8)
_P64 = ctypes.POINTER(ctypes.c_uint64)

INVALID, SHA1, SHA256 = 0, 1, 2  # BMPOW_SIG_* (include/bmpow_sig.h)


def _key64(key):
    """X || Y of a public key given as 64 raw bytes, 65 raw bytes (``04 || X || Y``) or the hex of
    either (str or bytes); None for anything else."""
    if isinstance(key, str):
        key = key.encode('ascii', 'replace')
    key = bytes(key)
    if len(key) in (128, 130):
        try:
            key = bytes.fromhex(key.decode('ascii'))
        except (ValueError, UnicodeDecodeError):
            return None
    if len(key) == 65:
        key = key[1:]  # hexToPubkey drops the first byte unread
    return key if len(key) == 64 else None


def verify_batch_digest(msgs, sigs, pubkeys):
    """Per (message, DER signature, public key) the reference's verdict as a code: ``SHA1`` (1) where
    the signature is valid under SHA-1, ``SHA256`` (2) where it is valid under SHA-256 only,
    ``INVALID`` (0) otherwise -- also for a signature that is no canonical DER, a key that is not 64 /
    65 bytes, has a coordinate >= p or is off the curve (the reference's ``except:`` returns False)."""
    n = len(msgs)
    if not (n == len(sigs) == len(pubkeys)):
        raise ValueError('one signature and one key per message')
    if n == 0:
        return []
    ms = [m if type(m) is bytes else bytes(m) for m in msgs]
    ss = [s if type(s) is bytes else bytes(s) for s in sigs]
    keys = [_key64(k) for k in pubkeys]
    live = [i for i, k in enumerate(keys) if k is not None]
    out = [INVALID] * n
    if not live:
        return out
    m = len(live)
    lib = _lib.get()
    mp = (ctypes.c_char_p * m)(*[ms[i] for i in live])
    sp = (ctypes.c_char_p * m)(*[ss[i] for i in live])
    ml = np.fromiter((len(ms[i]) for i in live), dtype=np.uint64, count=m)
    sl = np.fromiter((len(ss[i]) for i in live), dtype=np.uint64, count=m)
    verdict = np.zeros(m, dtype=np.uint8)
    _lib.check(lib, lib.bmpow_sig_verify(m, ctypes.cast(mp, ctypes.c_void_p), ml.ctypes.data_as(_P64),
                                         ctypes.cast(sp, ctypes.c_void_p), sl.ctypes.data_as(_P64),
                                         b''.join(keys[i] for i in live), verdict.ctypes.data_as(_PU8)),
               'bmpow_sig_verify')
    for i, v in zip(live, verdict):
        out[i] = int(v)
    return out


def verify_batch(msgs, sigs, pubkeys):
    """``highlevelcrypto.verify`` for a batch: one bool per (message, signature, public key)."""
    return [v != INVALID for v in verify_batch_digest(msgs, sigs, pubkeys)]


def verify(msg, sig, hexPubkey):
    """``highlevelcrypto.verify(msg, sig, hexPubkey)`` (``src/highlevelcrypto.py:88-108``): ``hexPubkey``
    is the hex of ``04 || X || Y``, str or bytes."""
    return verify_batch([msg], [sig], [hexPubkey])[0]


def ecdsa_verify_digest(pubkeys, rs, digests):
    """The raw equation (``bmpow_ecdsa_verify_digest``): per (X || Y, r || s, 32-byte big-endian digest)
    whether the signature verifies; strict about ranges (coordinate >= p, point off the curve, r or s
    equal to 0 or >= n give False)."""
    n = len(pubkeys)
    if not (n == len(rs) == len(digests)):
        raise ValueError('one r || s and one digest per key')
    if n == 0:
        return []
    pub, sig, e = b''.join(map(bytes, pubkeys)), b''.join(map(bytes, rs)), b''.join(map(bytes, digests))
    if len(pub) != 64 * n or len(sig) != 64 * n or len(e) != 32 * n:
        raise ValueError('keys and r || s are 64 bytes each, digests 32')
    lib = _lib.get()
    ok = ctypes.create_string_buffer(n)
    _lib.check(lib, lib.bmpow_ecdsa_verify_digest(n, pub, sig, e, ctypes.cast(ok, _PU8)), 'bmpow_ecdsa_verify_digest')
    return [bool(b) for b in ok.raw]


def parse(sig):
    """``(r, s)`` as 32 big-endian bytes each for a canonical DER signature with 1 <= r, s < n (host
    only), else None."""
    lib = _lib.host()
    sig = bytes(sig)
    rs = ctypes.create_string_buffer(64)
    rc = _lib.check(lib, lib.bmpow_sig_parse(sig, len(sig), ctypes.cast(rs, _PU8)), 'bmpow_sig_parse')
    return (rs.raw[:32], rs.raw[32:]) if rc == 1 else None


def stats():
    """The library's signature counters (``bmpow_sig_stats``) as a dict."""
    lib = _lib.get()
    st = _lib.BmpowSigStats()
    _lib.check(lib, lib.bmpow_sig_get_stats(ctypes.byref(st)), 'bmpow_sig_get_stats')
    return {f: getattr(st, f) for f, _ in st._fields_}


def reset_stats():
    _lib.get().bmpow_sig_reset_stats()


def pubkey_v3_signed_parts(obj):
    """``(signedData, signature, pubSigningKey64)`` of a v3 pubkey object as ``processpubkey`` takes
    them (``src/class_objectProcessor.py:345-371``; the header walk ``:276-282``): ``signedData`` is
    ``obj[8:endOfSignedData]``, the signing key the 64 bytes after the 4 behaviour bytes.  None where
    the reference returns before ``verify``: an address version other than 3 (this extractor's scope),
    ``len(obj) < 170``, or a varint that does not decode (the reference raises).  A signature cut short
    by the end of the object is returned as it is sliced there; ``verify`` then says False."""
    obj = bytes(obj)
    pos = 20
    ver = _varint(obj[pos:pos + 10])
    if ver is None:
        return None
    pos += ver[1]
    stream = _varint(obj[pos:pos + 10])
    if stream is None:
        return None
    pos += stream[1]
    if ver[0] != 3 or len(obj) < 170:
        return None
    pos += 4
    key = obj[pos:pos + 64]
    pos += 128
    for _ in range(2):  # nonceTrialsPerByte, payloadLengthExtraBytes
        v = _varint(obj[pos:pos + 10])
        if v is None:
            return None
        pos += v[1]
    end = pos
    siglen = _varint(obj[pos:pos + 10])
    if siglen is None:
        return None
    pos += siglen[1]
    return obj[8:end], obj[pos:pos + siglen[0]], key


def msg_signed_parts(obj, plaintext):
    """``(signedData, signature, pubSigningKey64)`` of a decrypted msg as ``processmsg`` takes them
    (``src/class_objectProcessor.py:479-564``; the object's msg version and stream ``:441-452``):
    ``signedData`` is ``obj[8:20] + varint(1) + varint(stream) + plaintext[:bottomOfAckData]``.  None
    where the reference returns before ``verify``: a msg version other than 1, sender version 0 or
    > 4, ``len(plaintext) < 170``, sender stream 0, or a varint that does not decode.  The ``toRipe``
    comparison (``:531``) stays with the caller; nothing past the signature is read."""
    obj, data = bytes(obj), bytes(plaintext)
    mv = _varint(obj[20:29])
    if mv is None or mv[0] != 1:
        return None
    claimed = _varint(obj[20 + mv[1]:29 + mv[1]])
    if claimed is None:
        return None
    pos = 0
    ver = _varint(data[pos:pos + 10])
    if ver is None:
        return None
    pos += ver[1]
    if ver[0] == 0 or ver[0] > 4 or len(data) < 170:
        return None
    stream = _varint(data[pos:pos + 10])
    if stream is None or stream[0] == 0:
        return None
    pos += stream[1] + 4
    key = data[pos:pos + 64]
    pos += 128
    if ver[0] >= 3:
        for _ in range(2):  # requiredAverageProofOfWorkNonceTrialsPerByte, requiredPayloadLengthExtraBytes
            v = _varint(data[pos:pos + 10])
            if v is None:
                return None
            pos += v[1]
    pos += 20  # toRipe
    enc = _varint(data[pos:pos + 10])  # messageEncodingType
    if enc is None:
        return None
    pos += enc[1]
    for _ in range(2):  # message, ackData
        ln = _varint(data[pos:pos + 10])
        if ln is None:
            return None
        pos += ln[1] + ln[0]
    bottom = pos
    siglen = _varint(data[pos:pos + 10])
    if siglen is None:
        return None
    pos += siglen[1]
    signed = obj[8:20] + encodeVarint(1) + encodeVarint(claimed[0]) + data[:bottom]
    return signed, data[pos:pos + siglen[0]], key


BroadcastParts = collections.namedtuple('BroadcastParts', [
    'signedData', 'signature', 'pubSigningKey64', 'pubEncryptionKey64', 'senderVersion', 'senderStream', 'encoding',
    'message', 'pubkeyData'])
PubkeyV4Parts = collections.namedtuple('PubkeyV4Parts', [
    'signedData', 'signature', 'pubSigningKey64', 'pubEncryptionKey64', 'storedData', 'addressVersion', 'stream', 'tag'])


def broadcast_header(obj):
    """``(broadcastVersion, stream, tag, payloadOffset)`` of a broadcast object as ``processbroadcast``
    walks it (``src/class_objectProcessor.py:756-769``, ``:808-809``): ``tag`` is the 32 bytes behind the
    stream number of a v5 broadcast (fewer where the object ends there) and None for v4; the encrypted
    part is ``obj[payloadOffset:]`` and the signed data starts with ``obj[8:payloadOffset]``.  None where
    the reference returns at ``:760`` (a broadcast version other than 4 or 5) or a varint raises."""
    obj = bytes(obj)
    pos = 20
    bv = _varint(obj[pos:pos + 9])
    if bv is None or bv[0] < 4 or bv[0] > 5:
        return None
    pos += bv[1]
    stream = _varint(obj[pos:pos + 10])
    if stream is None:
        return None
    pos += stream[1]
    if bv[0] == 4:
        return 4, stream[0], None, pos
    return 5, stream[0], obj[pos:pos + 32], pos + 32


def broadcast_signed_parts(obj, plaintext):
    """What ``processbroadcast`` reads out of a decrypted broadcast (``src/class_objectProcessor.py:
    826-915``) as a :class:`BroadcastParts`: ``signedData`` is ``obj[8:payloadOffset] +
    plaintext[:readPositionAtBottomOfMessage]``, ``pubkeyData`` is ``plaintext[:endOfPubkeyPosition]``
    (what the pubkeys table stores), the keys are the 64 bytes the reference puts ``04`` in front of.  None
    where the reference returns before ``verify`` for a reason the plaintext alone decides: a sender
    version outside 2..3 for a v4 broadcast (``:830``) or below 4 for a v5 one (``:838``), a sender stream
    other than the object's (``:848``), encoding type 0 (``:901``), or a varint that raises.  The ripe
    (``:882``) and tag (``:893``) comparisons stay with the caller (:func:`receive.process_broadcasts`).
    Slices cut short by the end of the plaintext are returned as they are sliced there."""
    head = broadcast_header(obj)
    if head is None:
        return None
    obj, data = bytes(obj), bytes(plaintext)
    bv, cleartext_stream = head[0], head[1]
    pos = 0
    ver = _varint(data[pos:pos + 9])
    if ver is None:
        return None
    if (bv == 4 and (ver[0] < 2 or ver[0] > 3)) or (bv == 5 and ver[0] < 4):
        return None
    pos += ver[1]
    stream = _varint(data[pos:pos + 9])
    if stream is None or stream[0] != cleartext_stream:
        return None
    pos += stream[1] + 4
    key_s = data[pos:pos + 64]
    pos += 64
    key_e = data[pos:pos + 64]
    pos += 64
    if ver[0] >= 3:
        for _ in range(2):  # requiredAverageProofOfWorkNonceTrialsPerByte, requiredPayloadLengthExtraBytes
            v = _varint(data[pos:pos + 10])
            if v is None:
                return None
            pos += v[1]
    end_of_pubkey = pos
    enc = _varint(data[pos:pos + 9])
    if enc is None or enc[0] == 0:
        return None
    pos += enc[1]
    mlen = _varint(data[pos:pos + 9])
    if mlen is None:
        return None
    pos += mlen[1]
    message = data[pos:pos + mlen[0]]
    pos += mlen[0]
    bottom = pos
    siglen = _varint(data[pos:pos + 9])
    if siglen is None:
        return None
    pos += siglen[1]
    return BroadcastParts(obj[8:head[3]] + data[:bottom], data[pos:pos + siglen[0]], key_s, key_e, ver[0], stream[0],
                          enc[0], message, data[:end_of_pubkey])


def pubkey_v4_header(obj):
    """``(addressVersion, stream, tag, payloadOffset)`` of an encrypted pubkey object as
    ``decryptAndCheckPubkeyPayload`` walks it (``src/protocol.py:412-439``); None where a varint raises."""
    obj = bytes(obj)
    pos = 20
    ver = _varint(obj[pos:pos + 10])
    if ver is None:
        return None
    pos += ver[1]
    stream = _varint(obj[pos:pos + 10])
    if stream is None:
        return None
    pos += stream[1]
    return ver[0], stream[0], obj[pos:pos + 32], pos + 32


def pubkey_v4_signed_parts(obj, plaintext):
    """What ``decryptAndCheckPubkeyPayload`` reads out of a decrypted v4 pubkey (``src/protocol.py:
    412-482``) as a :class:`PubkeyV4Parts`: ``signedData`` is ``obj[8:payloadOffset] +
    plaintext[:endOfKeys]``, ``storedData`` ``obj[20:tagOffset] + plaintext[:endOfKeys]`` (what the pubkeys
    table stores, ``:421``, ``:477``).  None where a varint raises
    (the reference's ``except varintDecodeError`` returns ``'failed'``).  The version, stream and ripe
    comparisons stay with the caller (:func:`receive.check_pubkeys_v4`)."""
    head = pubkey_v4_header(obj)
    if head is None:
        return None
    obj = bytes(obj)
    ver, stream, tag, off = head
    data = bytes(plaintext)
    pos = 4
    key_s = data[pos:pos + 64]
    pos += 64
    key_e = data[pos:pos + 64]
    pos += 64
    for _ in range(2):  # specifiedNonceTrialsPerByte, specifiedPayloadLengthExtraBytes
        v = _varint(data[pos:pos + 10])
        if v is None:
            return None
        pos += v[1]
    end = pos
    siglen = _varint(data[pos:pos + 10])
    if siglen is None:
        return None
    pos += siglen[1]
    return PubkeyV4Parts(obj[8:off] + data[:end], data[pos:pos + siglen[0]], key_s, key_e, obj[20:off - 32] + data[:end],
                         ver, stream, tag)
