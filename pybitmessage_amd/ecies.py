"""Batched ECIES trial decryption of received msgs and broadcasts on the GPU.

The reference tries every msg that passed the PoW check against every private key the user holds
(``class_objectProcessor.processmsg``, ``src/class_objectProcessor.py:459-477``; broadcasts
``:779-790``), one ``pyelliptic.ECC.decrypt`` (``src/pyelliptic/ecc.py:484-501``) per try: an ECDH on
secp256k1 with the message's ephemeral key, a SHA-512 of the shared x and an HMAC-SHA256 over the
whole blob -- and almost every try fails.  Here ``bmpow_ecies_match`` (``include/bmpow_ecies.h``)
runs all tries of a batch on the device and reports, per payload, the key whose MAC verifies; the
AES pass of the matches is one more call on the device (``bmpow_aes256_cbc``; a single payload can
still be opened on the host with ``bmpow_ecies_decrypt``, libcrypto).  Every key is
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


def aes_cbc_batch(keys, ivs, data, decrypt=False):
    """Raw AES-256-CBC with PKCS#7 padding on the device (``bmpow_aes256_cbc``), one 32-byte key and one
    16-byte IV per message.  Encrypting gives the padded ciphertexts.  Decrypting gives the plaintexts,
    None where the reference's ``decrypt`` raises: an input that is empty or no multiple of 16 bytes, or
    bad padding."""
    n = len(data)
    if not (n == len(keys) == len(ivs)):
        raise ValueError('one key and one IV per message')
    if n == 0:
        return []
    ks, vs = [bytes(k) for k in keys], [bytes(v) for v in ivs]
    if any(len(k) != 32 for k in ks) or any(len(v) != 16 for v in vs):
        raise ValueError('keys are 32 bytes, IVs 16 each')
    msgs = [d if type(d) is bytes else bytes(d) for d in data]
    lib = _lib.get()
    ptrs = (ctypes.c_char_p * n)(*msgs)
    lens = np.fromiter(map(len, msgs), dtype=np.uint64, count=n)
    caps = lens.copy() if decrypt else 16 * (lens // 16 + 1)
    offs = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(caps, out=offs[1:])
    arena = np.zeros(max(int(offs[-1]), 1), dtype=np.uint8)
    outs = (arena.ctypes.data + offs[:-1]).astype(np.uint64)
    got = np.zeros(n, dtype=np.int64)
    p64 = ctypes.POINTER(ctypes.c_uint64)
    _lib.check(lib, lib.bmpow_aes256_cbc(n, 1 if decrypt else 0, b''.join(ks), b''.join(vs),
                                         ctypes.cast(ptrs, ctypes.c_void_p), lens.ctypes.data_as(p64),
                                         outs.ctypes.data_as(ctypes.c_void_p), caps.ctypes.data_as(p64),
                                         got.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))),
               'bmpow_aes256_cbc')
    return [arena[int(offs[i]):int(offs[i]) + int(got[i])].tobytes() if got[i] >= 0 else None for i in range(n)]


def decrypt_batch(payloads, privkeys):
    """Per payload ``(index, plaintext)`` of the matching key, or None where no key matches or the
    matching key's plaintext has bad padding (the reference's ``decrypt`` raises there and
    ``processmsg`` goes on as if the key did not match).  The matches' ciphertexts are opened in one
    ``bmpow_aes256_cbc`` call on the device."""
    match, key_e, objs = _match(payloads, privkeys, True)
    hit = [i for i, m in enumerate(match) if m is not None]
    out = [None] * len(match)
    if not hit:
        return out
    # a match is well-formed: its header lies inside data[:-32] (ecies_parse), the ciphertext behind it
    bodies = []
    for i in hit:
        p = objs[i]
        xl = int.from_bytes(p[18:20], 'big')
        bodies.append(p[22 + xl + int.from_bytes(p[20 + xl:22 + xl], 'big'):-32])
    plains = aes_cbc_batch([key_e[i].tobytes() for i in hit], [objs[i][:16] for i in hit], bodies, decrypt=True)
    for i, plain in zip(hit, plains):
        if plain is not None:
            out[i] = (match[i], plain)
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
