"""Batched ECIES trial decryption of received msgs and broadcasts on the GPU.

The reference tries every msg that passed the PoW check against every private key the user holds
(``class_objectProcessor.processmsg``, ``src/class_objectProcessor.py:459-477``; broadcasts
``:779-790``), one ``pyelliptic.ECC.decrypt`` (``src/pyelliptic/ecc.py:484-501``) per try: an ECDH on
secp256k1 with the message's ephemeral key, a SHA-512 of the shared x and an HMAC-SHA256 over the
whole blob -- and almost every try fails.  Here ``bmpow_ecies_match`` (``include/bmpow_ecies.h``)
runs all tries of a batch on the device and reports, per payload, the key whose MAC verifies; the
AES pass of the few matches runs on the host (``bmpow_ecies_decrypt``, libcrypto).  Every key is
tried against every payload whatever the outcome, so a call's duration says nothing about which
payload matched.  No CPU fallback: without the HIP library the calls raise
:class:`BmpowUnavailable`.
"""
import ctypes

import numpy as np

from . import _lib

_PU8 = ctypes.POINTER(ctypes.c_uint8)


def _key32(key):
    """pyelliptic keeps private keys as ``BN_bn2bin`` leaves them, leading zero bytes stripped."""
    key = bytes(key)
    if len(key) > 32:
        raise ValueError('private key longer than 32 bytes')
    return key.rjust(32, b'\x00')


def _match(payloads, privkeys, want_key_e):
    objs = [p if type(p) is bytes else bytes(p) for p in payloads]
    keys = b''.join(_key32(k) for k in privkeys)
    n, nk = len(objs), len(keys) // 32
    if n == 0:
        return [], None, objs
    lib = _lib.get()
    ptrs = (ctypes.c_char_p * n)(*objs)
    lens = np.fromiter(map(len, objs), dtype=np.uint64, count=n)
    match = np.zeros(n, dtype=np.int32)
    key_e = np.zeros((n, 32), dtype=np.uint8) if want_key_e else None
    _lib.check(lib, lib.bmpow_ecies_match(n, ctypes.cast(ptrs, ctypes.c_void_p),
                                          lens.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), nk, keys,
                                          match.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                          key_e.ctypes.data_as(_PU8) if want_key_e else None),
               'bmpow_ecies_match')
    return [int(m) if m >= 0 else None for m in match], key_e, objs


def match_keys(payloads, privkeys):
    """Per payload, the lowest index into ``privkeys`` of a key whose MAC verifies, or None
    (also for a malformed payload or an ephemeral point off the curve)."""
    return _match(payloads, privkeys, False)[0]


def decrypt(payload, key_e):
    """AES-256-CBC of the payload's ciphertext with ``key_e`` (host, libcrypto); None where the
    reference's ``decrypt`` raises: bad padding, or a ciphertext that is empty or no multiple of
    16 bytes."""
    lib = _lib.host()
    payload, key_e = bytes(payload), bytes(key_e)
    out = ctypes.create_string_buffer(max(len(payload), 1))
    n = lib.bmpow_ecies_decrypt(payload, len(payload), key_e, ctypes.cast(out, _PU8), len(payload))
    return out.raw[:n] if n >= 0 else None


def decrypt_batch(payloads, privkeys):
    """Per payload ``(index, plaintext)`` of the matching key, or None where no key matches or the
    matching key's plaintext has bad padding (the reference's ``decrypt`` raises there and
    ``processmsg`` goes on as if the key did not match)."""
    match, key_e, objs = _match(payloads, privkeys, True)
    out = []
    for i, m in enumerate(match):
        plain = decrypt(objs[i], key_e[i].tobytes()) if m is not None else None
        out.append((m, plain) if plain is not None else None)
    return out


def _varint(data):
    """``addresses.decodeVarint``: (value, length), or None where the reference raises (truncated or
    not minimally encoded); empty input gives (0, 0) as there."""
    if not data:
        return 0, 0
    first = data[0]
    if first < 253:
        return first, 1
    size, floor = {253: (2, 253), 254: (4, 65536), 255: (8, 4294967296)}[first]
    if len(data) < 1 + size:
        return None
    value = int.from_bytes(data[1:1 + size], 'big')
    return (value, 1 + size) if value >= floor else None


def msg_payload(obj):
    """The encrypted part of a msg object, ``data[readPosition:]`` of ``processmsg`` (:441-452): past
    the 20-byte header (nonce, time, object type), the msg version and the stream number.  None unless
    the version is 1 (or where a varint does not decode)."""
    obj = bytes(obj)
    pos = 20
    ver = _varint(obj[pos:pos + 9])
    if ver is None or ver[0] != 1:
        return None
    pos += ver[1]
    stream = _varint(obj[pos:pos + 9])
    if stream is None:
        return None
    return obj[pos + stream[1]:]


def process_msgs(objects, keys_by_ripe):
    """The decryption loop of ``processmsg`` for a batch of msg objects: per object ``(ripe,
    plaintext)`` for the key that decrypts it, or None.  ``keys_by_ripe`` maps the ripe of each of the
    user's addresses to its private encryption key (``shared.myECCryptorObjects``'s keys and the
    ``privkey`` of its values)."""
    ripes = list(keys_by_ripe)
    payloads = [msg_payload(o) for o in objects]
    live = [i for i, p in enumerate(payloads) if p is not None]
    res = decrypt_batch([payloads[i] for i in live], [keys_by_ripe[r] for r in ripes])
    out = [None] * len(payloads)
    for i, r in zip(live, res):
        if r is not None:
            out[i] = (ripes[r[0]], r[1])
    return out


def ecdh(privkeys, points):
    """Raw shared x of each (key, (X, Y)) pair as 32 big-endian bytes, or None for a refused pair
    (``bmpow_ecdh``: coordinate >= p, point off the curve, key 0 or >= n)."""
    n = len(privkeys)
    if n != len(points):
        raise ValueError('one point per key')
    if n == 0:
        return []
    priv = b''.join(_key32(k) for k in privkeys)
    pub = b''.join(bytes(x).rjust(32, b'\x00') + bytes(y).rjust(32, b'\x00') for x, y in points)
    if len(pub) != 64 * n:
        raise ValueError('coordinate longer than 32 bytes')
    lib = _lib.get()
    out = ctypes.create_string_buffer(32 * n)
    ok = ctypes.create_string_buffer(n)
    _lib.check(lib, lib.bmpow_ecdh(n, priv, pub, ctypes.cast(out, _PU8), ctypes.cast(ok, _PU8)), 'bmpow_ecdh')
    return [out.raw[32 * i:32 * i + 32] if ok.raw[i] else None for i in range(n)]


def parse(payload):
    """``(X mod p, Y mod p, body_off)`` of a well-formed payload (host only), else None."""
    lib = _lib.host()
    payload = bytes(payload)
    xy = ctypes.create_string_buffer(64)
    off = ctypes.c_size_t(0)
    rc = _lib.check(lib, lib.bmpow_ecies_parse(payload, len(payload), ctypes.cast(xy, _PU8), ctypes.byref(off)),
                    'bmpow_ecies_parse')
    return (xy.raw[:32], xy.raw[32:], off.value) if rc == 1 else None
