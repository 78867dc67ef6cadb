#!/usr/bin/env python3
"""Generate tests/golden/ecies_kats.json -- ECIES trial-decryption fixtures from the REFERENCE's own
``pyelliptic.ECC`` over OpenSSL (build container only; needs /root/reference, read-only):

    BITMESSAGE_HOME=$(mktemp -d) PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_ecies_golden.py

``ECC.encrypt`` draws a random ephemeral key and IV for every blob and the recipient keys are random
too, so a re-run gives a different but equally valid file; the scalar list of ``ecdh_kats`` is seeded.

* ``ecdh_kats``: ``ECC.raw_get_ecdh_key`` (src/pyelliptic/ecc.py:203-257) for edge and random private
  keys against 3 points, one of them with a 31-byte X as ``BN_bn2bin`` leaves it.
* ``msg_kats``: ``ECC.encrypt`` (:452-482) of plaintexts of 0..1000 bytes to three recipient keys, plus
  blobs whose ephemeral key has a short coordinate; each blob is decrypted again by the reference.
* ``verdict_kats``: hand-built payloads run through ``ECC.decrypt`` (:484-501): what the reference
  accepts (``outcome`` = 'decrypted') and what it raises (the exception's class name).  ``wellformed``
  states the structural rule (the key header lies inside ``data[:-32]``), ``match`` whether the
  reference's own ECDH succeeded and its HMAC equalled the trailing 32 bytes.
"""
import hashlib
import hmac
import json
import os
import random
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REF_SRC = '/root/reference/src'

P = 2 ** 256 - 2 ** 32 - 977
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
CURVE = 714  # secp256k1 (pyelliptic/openssl.py)


def main():
    sys.path.insert(0, REF_SRC)
    from pyelliptic.cipher import Cipher
    from pyelliptic.ecc import ECC

    def be(v, n=32):
        return v.to_bytes(n, 'big')

    def with_priv(k):
        e = ECC(curve='secp256k1')
        e.privkey = be(k).lstrip(b'\x00')  # as BN_bn2bin leaves it
        return e

    # ---- ecdh_kats ----
    rng = random.Random(20250216 + 7)
    keys = [1, 2, 3, 15, 16, 17]
    for j in (4, 8, 128, 255):
        keys += [2 ** j - 1, 2 ** j + 1]
    keys += [N - 1, N - 2, (N - 1) // 2, int('aa' * 32, 16), int('55' * 32, 16)]
    keys += [rng.randrange(1, N) for _ in range(40)]
    points = []
    while len(points) < 3:
        e = ECC(curve='secp256k1')
        short = len(e.pubkey_x) == 31
        if (len(points) == 2) != short or len(e.pubkey_y) != 32:
            continue  # two full-width points, then one with a 31-byte X
        points.append(e)
    ecdh = {'keys': [be(k).hex() for k in keys],
            'points': [{'x': p.pubkey_x.hex(), 'y': p.pubkey_y.hex()} for p in points],
            'shared_x': [[with_priv(k).raw_get_ecdh_key(p.pubkey_x, p.pubkey_y).hex() for k in keys] for p in points]}
    print('ecdh kats: %d keys x %d points' % (len(keys), len(points)))

    # ---- msg_kats ----
    recips = [ECC(curve='secp256k1') for _ in range(3)]
    rkeys = [r.privkey.rjust(32, b'\x00').hex() for r in recips]
    msgs = []

    def coord_lens(blob):
        xl = struct.unpack('!H', blob[18:20])[0]
        yl = struct.unpack('!H', blob[20 + xl:22 + xl])[0]
        return xl, yl

    for ri, r in enumerate(recips):
        for n in (0, 1, 15, 16, 17, 100, 1000):
            pt = bytes(rng.randrange(256) for _ in range(n))
            blob = ECC.encrypt(pt, r.get_pubkey())
            assert r.decrypt(blob) == pt
            msgs.append({'recipient': ri, 'plaintext': pt.hex(), 'blob': blob.hex()})
    nshort = 0
    while nshort < 2:
        pt = b'short coordinate %d' % nshort
        blob = ECC.encrypt(pt, recips[nshort].get_pubkey())
        if coord_lens(blob) == (32, 32):
            continue
        assert recips[nshort].decrypt(blob) == pt
        msgs.append({'recipient': nshort, 'plaintext': pt.hex(), 'blob': blob.hex(), 'coord_lens': list(coord_lens(blob))})
        nshort += 1
    print('msg kats:', len(msgs))

    # ---- verdict_kats ----
    r0 = recips[0]
    eph = points[0]
    X, Y = int.from_bytes(eph.pubkey_x, 'big'), int.from_bytes(eph.pubkey_y, 'big')
    shared = r0.raw_get_ecdh_key(eph.pubkey_x, eph.pubkey_y)
    key = hashlib.sha512(shared).digest()
    key_e, key_m = key[:32], key[32:]
    iv = bytes(range(16))
    plain = b'A' * 40

    def enc(pt):
        return Cipher(key_e, iv, 1, 'aes-256-cbc').ciphering(pt)

    def forge(xb, yb, ct, curve=CURVE, mac=True, tamper=False):
        body = iv + struct.pack('!H', curve) + struct.pack('!H', len(xb)) + xb + struct.pack('!H', len(yb)) + yb + ct
        tag = hmac.new(key_m, body, hashlib.sha256).digest() if mac else b'\x5a' * 32
        if tamper:
            tag = tag[:-1] + bytes([tag[-1] ^ 1])
        return body + tag

    ct = enc(plain)
    xb, yb = be(X), be(Y)
    hdr = iv + struct.pack('!HH', CURVE, 32) + xb + struct.pack('!H', 32) + yb  # 86 bytes
    cases = [
        ('plain', forge(xb, yb, ct)),
        ('curve_zero', forge(xb, yb, ct, curve=0)),
        ('curve_other', forge(xb, yb, ct, curve=415)),
        ('x_33_leading_zero', forge(b'\x00' + xb, yb, ct)),
        ('y_34_leading_zeros', forge(xb, b'\x00\x00' + yb, ct)),
        ('x_plus_p', forge(be(X + P, 33), yb, ct)),
        ('y_plus_p', forge(xb, be(Y + P, 33), ct)),
        ('neg_y', forge(xb, be(P - Y), ct)),
        ('off_curve', forge(xb, be((Y + 1) % P), ct)),
        ('x_zero_len', forge(b'', yb, ct)),
        ('bad_mac', forge(xb, yb, ct, tamper=True)),
        ('empty', b''),
        ('short_10', hdr[:10]),
        ('short_17', hdr[:17]),
        ('short_19', hdr[:19]),
        ('short_21', hdr[:21]),
        ('cut_in_x', hdr[:40]),
        ('cut_in_ylen', hdr[:53]),
        ('cut_in_y', hdr[:70]),
        ('tail_0', hdr),
        ('tail_1', hdr + b'\x01'),
        ('tail_31', hdr + b'\x02' * 31),
        ('tail_32_bad_mac', hdr + b'\x03' * 32),
        ('tail_33_bad_mac', hdr + b'\x04' * 33),
        ('tail_32_valid_mac', forge(xb, yb, b'')),
        ('tail_33_valid_mac', forge(xb, yb, b'\x07')),
        ('ct_17_valid_mac', forge(xb, yb, ct[:17])),
        ('bad_padding_valid_mac', forge(xb, yb, ct[:32])),  # 'A' * 32: the last byte 0x41 is no PKCS#7 pad
        ('xlen_claims_too_much', forge(xb, yb, ct)[:18] + struct.pack('!H', 4000) + forge(xb, yb, ct)[20:]),
    ]
    verdicts = []
    for name, blob in cases:
        wellformed, match = False, False
        if len(blob) >= 20:
            xl = struct.unpack('!H', blob[18:20])[0]
            if len(blob) >= 22 + xl:
                yl = struct.unpack('!H', blob[20 + xl:22 + xl])[0]
                off = 22 + xl + yl
                wellformed = off + 32 <= len(blob)
                if wellformed:
                    try:
                        sx = r0.raw_get_ecdh_key(blob[20:20 + xl], blob[22 + xl:off])
                        km = hashlib.sha512(sx).digest()[32:]
                        match = hmac.new(km, blob[:-32], hashlib.sha256).digest() == blob[-32:]
                    except Exception:  # noqa: BLE001 -- the reference's own refusal of the point
                        match = False
        entry = {'name': name, 'blob': blob.hex(), 'wellformed': wellformed, 'match': match}
        try:
            out = r0.decrypt(blob)
            entry['outcome'] = 'decrypted'
            entry['plaintext'] = out.hex()
        except Exception as exc:  # noqa: BLE001 -- recorded, whatever it is
            entry['outcome'] = type(exc).__name__
            entry['message'] = str(exc)[:80]
        print('  %-24s wellformed=%d match=%d %s' % (name, wellformed, match, entry['outcome']))
        verdicts.append(entry)

    import ssl
    with open(os.path.join(HERE, 'ecies_kats.json'), 'w') as f:
        json.dump({'source': 'reference pyelliptic.ECC raw_get_ecdh_key / encrypt / decrypt over ' + ssl.OPENSSL_VERSION,
                   'ecdh_kats': ecdh, 'recipient_keys': rkeys, 'msg_kats': msgs,
                   'verdict_key': rkeys[0], 'verdict_shared_x': shared.hex(),
                   'verdict_point': {'x': xb.hex(), 'y': yb.hex()}, 'verdict_kats': verdicts}, f, indent=1)
    print('wrote ecies_kats.json')


if __name__ == '__main__':
    main()
