"""Batched ECDSA signing, ECIES encryption and public-key derivation of outgoing objects on the GPU.

The reference signs and encrypts every object it sends with ``highlevelcrypto.sign`` / ``encrypt``
(``src/highlevelcrypto.py:54-85``; ``sendMsg``, ``src/class_singleWorker.py:1224-1234``) and derives
its addresses' public keys with ``pointMult`` / ``privToPub`` (``:47-51``, ``:111-146``): one
``pyelliptic`` call per object.  Here ``bmpow_sig_sign``, ``bmpow_ecies_encrypt`` and
``bmpow_ec_pubkeys`` (``include/bmpow_send.h``) take a whole batch: the curve and scalar arithmetic run
on the device, the AES-256-CBC and HMAC-SHA256 pass of the blobs on the host's threads (libcrypto) or,
with :func:`set_seal` (``BMPOW_SEAL=device``), on the device behind the ladder (``sl_seal_kernel``),
where the derived keys never reach host memory; the blobs are the same bytes either way.
Nonces, ephemeral keys and IVs come from libcrypto's ``RAND_bytes`` unless the caller supplies them.  No
CPU fallback: without the HIP library the calls raise :class:`BmpowUnavailable`.
"""
import ctypes

import numpy as np

from . import _lib
from .ecies import _key32
from .signatures import _key64

_PU8 = ctypes.POINTER(ctypes.c_uint8)
_P64 = ctypes.POINTER(ctypes.c_uint64)

DIGESTS = {'sha1': 1, 'sha256': 2}  # BMPOW_SIG_SHA1 / BMPOW_SIG_SHA256 (include/bmpow_sig.h)


def blob_cap(length):
    """``BMPOW_ECIES_BLOB_CAP``: the bound on the blob of a ``length``-byte plaintext."""
    return 118 + 16 * (length // 16 + 1)


def _as_bytes(items):
    return [x if type(x) is bytes else bytes(x) for x in items]


def priv_to_pub(privkeys):
    """``highlevelcrypto.pointMult`` for a batch: the 65 bytes ``04 || X || Y`` per private key, None
    for a key that is 0 or not below the group order."""
    n = len(privkeys)
    if n == 0:
        return []
    priv = b''.join(_key32(k) for k in privkeys)
    lib = _lib.get()
    pub = np.zeros((n, 64), dtype=np.uint8)
    ok = np.zeros(n, dtype=np.uint8)
    _lib.check(lib, lib.bmpow_ec_pubkeys(n, priv, pub.ctypes.data_as(_PU8), ok.ctypes.data_as(_PU8)), 'bmpow_ec_pubkeys')
    raw = pub.tobytes()
    return [b'\x04' + raw[64 * i:64 * i + 64] if ok[i] else None for i in range(n)]


def sign_digest(privkeys, nonces, digests):
    """The raw equation (``bmpow_ecdsa_sign_digest``): per (key, nonce, 32-byte big-endian digest) the
    64 bytes ``r || s``, or None for a key or nonce that is 0 or >= n and for ``r == 0`` or ``s == 0``."""
    n = len(privkeys)
    if not (n == len(nonces) == len(digests)):
        raise ValueError('one nonce and one digest per key')
    if n == 0:
        return []
    d, k = b''.join(_key32(x) for x in privkeys), b''.join(_key32(x) for x in nonces)
    e = b''.join(_as_bytes(digests))
    if len(e) != 32 * n:
        raise ValueError('digests are 32 bytes each')
    lib = _lib.get()
    rs = np.zeros((n, 64), dtype=np.uint8)
    ok = np.zeros(n, dtype=np.uint8)
    _lib.check(lib, lib.bmpow_ecdsa_sign_digest(n, d, k, e, rs.ctypes.data_as(_PU8), ok.ctypes.data_as(_PU8)),
               'bmpow_ecdsa_sign_digest')
    raw = rs.tobytes()
    return [raw[64 * i:64 * i + 64] if ok[i] else None for i in range(n)]


def der(rs):
    """The canonical DER signature of the 64 bytes ``r || s`` (host only)."""
    lib = _lib.host()
    out = ctypes.create_string_buffer(72)
    ln = ctypes.c_size_t(0)
    _lib.check(lib, lib.bmpow_sig_der(bytes(rs), ctypes.cast(out, _PU8), ctypes.byref(ln)), 'bmpow_sig_der')
    return out.raw[:ln.value]


def sign_batch(msgs, privkeys, digestalg='sha256', nonces=None):
    """``highlevelcrypto.sign`` for a batch: the DER signature of each message by its private key (32
    raw bytes, or fewer as ``BN_bn2bin`` leaves them) under ``digestalg`` ('sha256', the reference's
    default, or 'sha1').  ``nonces`` fixes each signature's k (tests); by default they are drawn.  None
    for a row whose r or s came out zero.  A key or supplied nonce that is 0 or >= n raises."""
    if digestalg not in DIGESTS:
        raise ValueError('Unknown digest algorithm %s' % digestalg)
    n = len(msgs)
    if n != len(privkeys) or (nonces is not None and n != len(nonces)):
        raise ValueError('one key (and one nonce) per message')
    if n == 0:
        return []
    ms = _as_bytes(msgs)
    priv = b''.join(_key32(k) for k in privkeys)
    ks = None if nonces is None else b''.join(_key32(k) for k in nonces)
    lib = _lib.get()
    mp = (ctypes.c_char_p * n)(*ms)
    ml = np.fromiter(map(len, ms), dtype=np.uint64, count=n)
    sig = np.zeros((n, 72), dtype=np.uint8)
    ln = np.zeros(n, dtype=np.uint8)
    _lib.check(lib, lib.bmpow_sig_sign(n, ctypes.cast(mp, ctypes.c_void_p), ml.ctypes.data_as(_P64), priv,
                                       DIGESTS[digestalg], ks, sig.ctypes.data_as(_PU8), ln.ctypes.data_as(_PU8)),
               'bmpow_sig_sign')
    raw = sig.tobytes()
    return [raw[72 * i:72 * i + int(ln[i])] if ln[i] else None for i in range(n)]


def sign(msg, hexPrivkey, digestalg='sha256'):
    """``highlevelcrypto.sign(msg, hexPrivkey)`` (``src/highlevelcrypto.py:70-85``); ``digestalg`` stands
    for the reference's ``bitmessagesettings.digestalg``."""
    if isinstance(hexPrivkey, bytes):
        hexPrivkey = hexPrivkey.decode('ascii')
    return sign_batch([msg], [bytes.fromhex(hexPrivkey)], digestalg)[0]


def seal(plaintext, iv, R_xy, key):
    """Everything of ``ECC.raw_encrypt`` after the key derivation (``bmpow_ecies_seal``, host only): the
    blob for the 16-byte IV, the ephemeral public key ``X || Y`` and ``key = key_e || key_m``."""
    lib = _lib.host()
    plaintext, iv, R_xy, key = bytes(plaintext), bytes(iv), bytes(R_xy), bytes(key)
    if len(iv) != 16 or len(R_xy) != 64 or len(key) != 64:
        raise ValueError('the IV is 16 bytes, the point and the key 64 each')
    cap = blob_cap(len(plaintext))
    out = ctypes.create_string_buffer(cap)
    n = _lib.check(lib, lib.bmpow_ecies_seal(plaintext, len(plaintext), iv, R_xy, key, ctypes.cast(out, _PU8), cap),
                   'bmpow_ecies_seal')
    return out.raw[:n]


def _arena(lens):
    """One output buffer for blobs of ``lens``-byte plaintexts: (arena, offsets, pointers, capacities)."""
    m = len(lens)
    caps = 118 + 16 * (lens // 16 + 1)
    offs = np.zeros(m + 1, dtype=np.uint64)
    np.cumsum(caps, out=offs[1:])
    arena = np.zeros(int(offs[-1]), dtype=np.uint8)
    ptrs = (arena.ctypes.data + offs[:-1]).astype(np.uint64)
    return arena, offs, ptrs, caps


def seal_batch(plaintexts, ivs, R_xys, keys):
    """:func:`seal` for a batch on the device (``bmpow_ecies_seal_batch``): per row the blob for its
    16-byte IV, ephemeral public key ``X || Y`` (64 bytes, taken as they are) and ``key_e || key_m``
    (64 bytes) -- the bytes :func:`seal` gives."""
    n = len(plaintexts)
    if not (n == len(ivs) == len(R_xys) == len(keys)):
        raise ValueError('one IV, one point and one key per plaintext')
    if n == 0:
        return []
    pts = _as_bytes(plaintexts)
    iv, pub, key = b''.join(_as_bytes(ivs)), b''.join(_as_bytes(R_xys)), b''.join(_as_bytes(keys))
    if len(iv) != 16 * n or len(pub) != 64 * n or len(key) != 64 * n or any(len(k) != 64 for k in keys) \
            or any(len(v) != 16 for v in ivs) or any(len(r) != 64 for r in R_xys):
        raise ValueError('the IV is 16 bytes, the point and the key 64 each')
    lib = _lib.get()
    pp = (ctypes.c_char_p * n)(*pts)
    lens = np.fromiter(map(len, pts), dtype=np.uint64, count=n)
    arena, offs, ptrs, caps = _arena(lens)
    got = np.zeros(n, dtype=np.uint64)
    _lib.check(lib, lib.bmpow_ecies_seal_batch(n, ctypes.cast(pp, ctypes.c_void_p), lens.ctypes.data_as(_P64), iv, pub, key,
                                               ptrs.ctypes.data_as(ctypes.c_void_p), caps.ctypes.data_as(_P64),
                                               got.ctypes.data_as(_P64)),
               'bmpow_ecies_seal_batch')
    return [arena[int(offs[j]):int(offs[j]) + int(got[j])].tobytes() for j in range(n)]


def set_seal(mode):
    """Where :func:`encrypt_batch` seals its blobs (``bmpow_send_set_seal``): 0 on the host's threads, 1 on
    the device, -1 only asks.  Returns the previous mode.  No device is touched."""
    return _lib.host().bmpow_send_set_seal(int(mode))


def seal_stats():
    """The device seal's counters (``bmpow_seal_stats``) as a dict."""
    lib = _lib.host()
    st = _lib.BmpowSealStats()
    _lib.check(lib, lib.bmpow_seal_get_stats(ctypes.byref(st)), 'bmpow_seal_get_stats')
    return {f: getattr(st, f) for f, _ in st._fields_}


def reset_seal_stats():
    _lib.host().bmpow_seal_reset_stats()


def encrypt_batch(plaintexts, pubkeys, ephemeral=None, ivs=None):
    """``highlevelcrypto.encrypt`` for a batch: the ECIES blob of each plaintext to its recipient key
    (64 or 65 raw bytes or their hex, as ``signatures.verify_batch`` takes keys).  None where the
    reference raises: a key of another size, with a coordinate >= p or off the curve.  ``ephemeral``
    (private keys) and ``ivs`` (16 bytes each) fix the random inputs (tests); by default they are drawn."""
    n = len(plaintexts)
    if n != len(pubkeys) or (ephemeral is not None and n != len(ephemeral)) or (ivs is not None and n != len(ivs)):
        raise ValueError('one key (and one ephemeral key, one IV) per plaintext')
    pts = _as_bytes(plaintexts)
    keys = [_key64(k) for k in pubkeys]
    live = [i for i, k in enumerate(keys) if k is not None]
    out = [None] * n
    if not live:
        return out
    m = len(live)
    eph = None if ephemeral is None else b''.join(_key32(ephemeral[i]) for i in live)
    iv = None if ivs is None else b''.join(bytes(ivs[i]) for i in live)
    if iv is not None and len(iv) != 16 * m:
        raise ValueError('IVs are 16 bytes each')
    lib = _lib.get()
    pp = (ctypes.c_char_p * m)(*[pts[i] for i in live])
    lens = np.fromiter((len(pts[i]) for i in live), dtype=np.uint64, count=m)
    arena, offs, ptrs, caps = _arena(lens)
    got = np.zeros(m, dtype=np.uint64)
    _lib.check(lib, lib.bmpow_ecies_encrypt(m, ctypes.cast(pp, ctypes.c_void_p), lens.ctypes.data_as(_P64),
                                            b''.join(keys[i] for i in live), eph, iv,
                                            ptrs.ctypes.data_as(ctypes.c_void_p), caps.ctypes.data_as(_P64),
                                            got.ctypes.data_as(_P64)),
               'bmpow_ecies_encrypt')
    for j, i in enumerate(live):
        if got[j]:
            a = int(offs[j])
            out[i] = arena[a:a + int(got[j])].tobytes()
    return out


def encrypt(msg, hexPubkey):
    """``highlevelcrypto.encrypt(msg, hexPubkey)`` (``src/highlevelcrypto.py:54-57``); raises where the
    reference does (the recipient's key is no good)."""
    blob = encrypt_batch([msg], [hexPubkey])[0]
    if blob is None:
        raise ValueError('the recipient key is not a point of secp256k1')
    return blob


def stats():
    """The library's send-side counters (``bmpow_send_stats``) as a dict."""
    lib = _lib.get()
    st = _lib.BmpowSendStats()
    _lib.check(lib, lib.bmpow_send_get_stats(ctypes.byref(st)), 'bmpow_send_get_stats')
    return {f: getattr(st, f) for f, _ in st._fields_}


def reset_stats():
    _lib.get().bmpow_send_reset_stats()
