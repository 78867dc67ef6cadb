#!/usr/bin/env python3
"""Generate tests/golden/point_kats.json -- what the REFERENCE's own ``pyelliptic.ECC`` over OpenSSL says
about points chosen by their coordinates (``oracle/ecdsa_oracle.py``: ``coordinate_points``, ``rn_msg_cases``,
``ecdh_cases``, ``shared_cases``); build container only, needs /root/reference, read-only:

    BITMESSAGE_HOME=$(mktemp -d) PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_point_golden.py

Everything is seeded: a re-run gives the same bytes.

* ``verify``: ``ECC.verify`` (src/pyelliptic/ecc.py:387-440) under SHA-1 and under SHA-256 for every
  message-level row of ``rn_cases`` (x(R) in [n, p) with r = x - n; r + n reaching p; r + n carrying out of
  256 bits; the honest siblings).  No row of ``key_cases`` is here: a signature over a given message under
  a key chosen by its coordinates needs that key's discrete logarithm.
* ``ecdh``: ``ECC.raw_get_ecdh_key`` (:203-257) for the first key of every point of ``ecdh_cases`` and
  ``shared_cases``, X and Y handed over as ``BN_bn2bin`` leaves them (leading zero bytes stripped).
* ``blobs``: 16 ECIES payloads whose ephemeral point is chosen by its coordinates, built from the oracle's
  shared x with the reference's ``Cipher`` and ``hmac_sha256`` and opened again with ``ECC.decrypt``
  (:484-501): short X or Y, a shared x with 8 or more leading zero bytes, and four spoiled ones (the MAC
  under x ^ 1; X replaced by x + p in 33 bytes).  ``match`` says whether the reference's own ECDH
  succeeded and its HMAC equalled the trailing 32 bytes, ``outcome`` what ``decrypt`` did.
"""
import hashlib
import json
import os
import random
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REF_SRC = '/root/reference/src'
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import ecdsa_oracle as eo  # noqa: E402

P, N = eo.P, eo.N
CURVE = 714  # secp256k1 (pyelliptic/openssl.py)
# (X, Y) lengths wanted among the blobs; (1, 1) stands for the shortest pair there is
COORD_LENS = ((1, 32), (2, 32), (17, 32), (31, 32), (32, 1), (32, 16), (1, 1))


def strip(v):
    """As ``BN_bn2bin`` leaves a number: no leading zero bytes."""
    return v.to_bytes(32, 'big').lstrip(b'\x00')


def lens(pt):
    return len(strip(pt[0])), len(strip(pt[1]))


def main():
    sys.path.insert(0, REF_SRC)
    from pyelliptic.cipher import Cipher
    from pyelliptic.ecc import ECC
    from pyelliptic.hash import hmac_sha256
    from pyelliptic.openssl import OpenSSL

    def with_pub(key64):
        e = ECC(curve='secp256k1')
        e.pubkey_x, e.pubkey_y = key64[:32], key64[32:]
        return e

    def with_priv(k):
        e = ECC(curve='secp256k1')
        e.privkey = strip(k)
        return e

    # ---- verify ----
    verify = []
    for c in eo.rn_msg_cases():
        e = with_pub(c.key)
        verify.append({'name': c.name, 'family': c.family, 'msg': c.msg.hex(), 'sig': c.sig.hex(), 'key': c.key.hex(),
                       'sha1': bool(e.verify(c.sig, c.msg, digest_alg=OpenSSL.digest_ecdsa_sha1)),
                       'sha256': bool(e.verify(c.sig, c.msg, digest_alg=OpenSSL.EVP_sha256))})
    print('verify:', len(verify), sum(v['sha1'] or v['sha256'] for v in verify), 'valid')

    # ---- ecdh ----
    ecdh = []
    for family, cases in (('ecdh', eo.ecdh_cases()), ('shared', eo.shared_cases())):
        for c in cases[::eo.ECDH_KEYS]:
            got = with_priv(c.k).raw_get_ecdh_key(strip(c.R[0]), strip(c.R[1]))
            ecdh.append({'name': c.name, 'family': family, 'key': strip(c.k).hex(), 'x': strip(c.R[0]).hex(),
                         'y': strip(c.R[1]).hex(), 'shared_x': got.hex()})
    print('ecdh:', len(ecdh))

    # ---- blobs ----
    rng = random.Random(1707)
    V = eo.scalar_set()
    recips = [V[-1], V[-2], V[-3]]  # three of V's random scalars
    points = dict(eo.coordinate_points())
    points['x_two_bytes'] = eo.nearest(2 ** 8)  # no point of the list has a 2-byte X
    by_lens = {}
    for name, pt in points.items():
        by_lens.setdefault(lens(pt), []).append(name)
    shortest = min(by_lens, key=lambda xy: (sum(xy), xy))
    chosen = []
    for want in COORD_LENS:
        names = by_lens[want if want in by_lens else shortest]
        chosen.append(next(name for name in names if name not in chosen))
    eph = [(name, points[name], None) for name in chosen]
    # a shared x with 8 or more leading zero bytes: the shared point itself is chosen, R = S / k
    shared = {c.name: c for c in eo.shared_cases()}
    for name in ('x_small_0_k0', 'x_zero_bytes_8_0_k0', 'x_zero_bytes_16_0_k0', 'x_zero_bytes_31_0_k0'):
        eph.append((name, None, shared[name]))
    eph.append(('x_from_n_0', points['x_from_n_0'], None))  # an ephemeral X in [n, p)

    def build(name, R, k, xb, yb, plain, iv, mac_x=None):
        """A payload to the key k with the point R written as xb, yb; the oracle's shared x keys it."""
        sx = eo.mult(k, R)[0]
        key = hashlib.sha512(sx.to_bytes(32, 'big')).digest()
        body = iv + struct.pack('!HH', CURVE, len(xb)) + xb + struct.pack('!H', len(yb)) + yb
        body += Cipher(key[:32], iv, 1, 'aes-256-cbc').ciphering(plain)
        key_m = key[32:] if mac_x is None else hashlib.sha512(mac_x.to_bytes(32, 'big')).digest()[32:]
        return sx, body + hmac_sha256(key_m, body)

    blobs = []

    def record(name, ri, sx, blob, plain, spoiled):
        r = with_priv(recips[ri])
        xl = struct.unpack('!H', blob[18:20])[0]
        yl = struct.unpack('!H', blob[20 + xl:22 + xl])[0]
        off = 22 + xl + yl
        try:
            got = r.raw_get_ecdh_key(blob[20:20 + xl], blob[22 + xl:off])
            match = hmac_sha256(hashlib.sha512(got).digest()[32:], blob[:-32]) == blob[-32:]
        except Exception:  # noqa: BLE001 -- the reference's own refusal of the point
            match = False
        entry = {'name': name, 'recipient': ri, 'coord_lens': [xl, yl], 'shared_x': sx.to_bytes(32, 'big').hex(),
                 'spoiled': spoiled, 'blob': blob.hex(), 'sent': plain.hex(), 'match': bool(match)}
        try:
            entry['plaintext'] = r.decrypt(blob).hex()
            entry['outcome'] = 'decrypted'
        except Exception as exc:  # noqa: BLE001 -- recorded, whatever it is
            entry['outcome'] = type(exc).__name__
        print('  %-28s lens=%s match=%d %s' % (name, entry['coord_lens'], match, entry['outcome']))
        blobs.append(entry)

    for j, (name, R, sc) in enumerate(eph):
        ri = j % 3
        if sc is not None:  # the case's own key instead of a recipient's
            k, R = sc.k, sc.R
            recips.append(k)
            ri = len(recips) - 1
        else:
            k = recips[ri]
        plain = bytes(rng.getrandbits(8) for _ in range((0, 1, 15, 16, 17, 40, 100)[j % 7]))
        iv = bytes(rng.getrandbits(8) for _ in range(16))
        sx, blob = build(name, R, k, strip(R[0]), strip(R[1]), plain, iv)
        assert sc is None or sx == sc.x < 2 ** 192
        record(name, ri, sx, blob, plain, None)
    for j, (name, R, _) in enumerate(eph[:4]):
        ri = j % 3
        plain = b'spoiled %d' % j
        iv = bytes(rng.getrandbits(8) for _ in range(16))
        if j < 2:
            sx = eo.mult(recips[ri], R)[0]
            _, blob = build(name, R, recips[ri], strip(R[0]), strip(R[1]), plain, iv, mac_x=sx ^ 1)
            record(name + '_mac_under_x_xor_1', ri, sx, blob, plain, 'mac')
        else:
            sx, blob = build(name, R, recips[ri], (R[0] + P).to_bytes(33, 'big'), strip(R[1]), plain, iv)
            record(name + '_x_plus_p', ri, sx, blob, plain, 'x_plus_p')
    assert len(blobs) == 16

    import ssl
    with open(os.path.join(HERE, 'point_kats.json'), 'w') as f:
        json.dump({'source': 'reference pyelliptic.ECC verify / raw_get_ecdh_key / decrypt over ' + ssl.OPENSSL_VERSION,
                   'verify': verify, 'ecdh': ecdh, 'recipient_keys': [k.to_bytes(32, 'big').hex() for k in recips],
                   'blobs': blobs}, f, indent=1)
        f.write('\n')
    print('wrote point_kats.json')


if __name__ == '__main__':
    main()
