#!/usr/bin/env python3
"""Generate tests/golden/send_kats.json -- send-side fixtures from the REFERENCE's own
``highlevelcrypto`` / ``pyelliptic.ECC`` over OpenSSL (build container only; needs /root/reference,
read-only):

    BITMESSAGE_HOME=$(mktemp -d) PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_send_golden.py

``ECC.encrypt`` draws a random ephemeral key and IV for every blob and the recipient keys are random too,
so a re-run gives a different but equally valid file; the scalars, the messages and the signing inputs
are seeded.

* ``encrypt_kats``: ``ECC.encrypt`` (src/pyelliptic/ecc.py:452-482) of plaintexts of 0, 1, 15, 16, 17, 100
  and 1000 bytes to three recipient keys, plus blobs whose ephemeral key has a 31-byte coordinate (drawn
  until two occur).  Each entry records the ephemeral private key -- ``raw_encrypt`` builds its key pair
  through the module's ``ECC`` name, which is a recording subclass while the blobs are made -- and the
  IV, the blob's first 16 bytes; every blob is decrypted again by the reference.
* ``pointmult_kats``: ``highlevelcrypto.pointMult`` (src/highlevelcrypto.py:111-146) of edge and seeded
  scalars.
* ``sign_kats``: for seeded (key d, nonce k, message) and both digests the DER signature of
  ``oracle/ecdsa_oracle.py`` (``sign`` + ``der_encode``: OpenSSL's ``ECDSA_sign`` with the nonce fixed)
  and the reference's ``highlevelcrypto.verify`` verdict on it, which must be True; with rows whose r is
  below 2^248 (found by scanning k) and s on either side of 2^255.
"""
import hashlib
import json
import os
import random
import struct
import sys
from binascii import hexlify

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF_SRC = '/root/reference/src'

N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141


def be(v, n=32):
    return v.to_bytes(n, 'big')


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(1, REF_SRC)
    from oracle import ecdsa_oracle as eo
    import highlevelcrypto
    import pyelliptic.ecc as eccmod

    rng = random.Random(20251019 + 11)
    RefECC = eccmod.ECC

    # ---- encrypt_kats ----
    recips = [RefECC(curve='secp256k1') for _ in range(3)]
    made = []  # private keys of the key pairs generated while the recorder is in place

    class Recorder(RefECC):
        def __init__(self, *args, **kwargs):
            RefECC.__init__(self, *args, **kwargs)
            if not args and set(kwargs) <= {'curve'}:
                made.append(self.privkey)

    def coord_lens(blob):
        xl = struct.unpack('!H', blob[18:20])[0]
        yl = struct.unpack('!H', blob[20 + xl:22 + xl])[0]
        return xl, yl

    def one(ri, pt):
        del made[:]
        eccmod.ECC = Recorder
        try:
            blob = RefECC.encrypt(pt, recips[ri].get_pubkey())
        finally:
            eccmod.ECC = RefECC
        assert len(made) == 1 and recips[ri].decrypt(blob) == pt
        eph = made[0].rjust(32, b'\x00')
        R = eo.mult_g(int.from_bytes(eph, 'big'))  # the recorded key is the blob's
        xl, yl = coord_lens(blob)
        assert blob[20:20 + xl].rjust(32, b'\x00') + blob[22 + xl:22 + xl + yl].rjust(32, b'\x00') == eo.xy_key(R)
        return {'recipient': ri, 'plaintext': pt.hex(), 'ephemeral': eph.hex(), 'iv': blob[:16].hex(),
                'coord_lens': [xl, yl], 'blob': blob.hex()}

    encrypt_kats = []
    for ri in range(3):
        for n in (0, 1, 15, 16, 17, 100, 1000):
            encrypt_kats.append(one(ri, bytes(rng.randrange(256) for _ in range(n))))
    nshort = sum(e['coord_lens'] != [32, 32] for e in encrypt_kats)
    tries = 0
    while nshort < 2:
        tries += 1
        e = one(nshort % 3, b'short coordinate %d' % nshort)
        if e['coord_lens'] == [32, 32]:
            continue
        encrypt_kats.append(e)
        nshort += 1
    print('encrypt kats: %d (%d with a short coordinate, %d extra draws)' % (len(encrypt_kats), nshort, tries))

    # ---- pointmult_kats ----
    scalars = [1, 2, 3, N - 1, N - 2, (N - 1) // 2]
    for j in (1, 8, 15, 16, 17, 32, 64, 128, 192, 240, 255):
        scalars += [2 ** j - 1, 2 ** j + 1]
    scalars += [rng.randrange(1, N) for _ in range(20)]
    pointmult_kats = []
    for k in scalars:
        pub = highlevelcrypto.pointMult(be(k))
        assert len(pub) == 65 and pub[:1] == b'\x04'
        pointmult_kats.append({'priv': be(k).hex(), 'pub': pub.hex()})
    print('pointmult kats:', len(pointmult_kats))

    # ---- sign_kats ----
    sign_kats = []

    def add_sign(name, d, k, msg, alg):
        e = int.from_bytes(hashlib.new(alg, msg).digest(), 'big')
        r, s = eo.sign(d, k, e)
        sig = eo.der_encode(r, s)
        key = eo.xy_key(eo.mult_g(d))
        verdict = bool(highlevelcrypto.verify(msg, sig, hexlify(b'\x04' + key)))
        assert verdict is True, name
        sign_kats.append({'name': name, 'digest': alg, 'priv': be(d).hex(), 'nonce': be(k).hex(), 'msg': msg.hex(),
                          'r': be(r).hex(), 's': be(s).hex(), 'sig': sig.hex(), 'pub': key.hex(), 'verdict': verdict})
        return r, s

    for alg in ('sha1', 'sha256'):
        for i, ln in enumerate((0, 1, 55, 56, 64, 100, 119, 120, 300, 1000)):
            msg = bytes(rng.randrange(256) for _ in range(ln))
            add_sign('%s_len%d' % (alg, ln), rng.randrange(1, N), rng.randrange(1, N), msg, alg)
        for i in range(2):  # a short r: its DER integer has fewer than 32 bytes
            k = rng.randrange(1, N)
            while eo.mult_g(k)[0] % N >= 2 ** 248:
                k += 1
            r, _ = add_sign('%s_short_r_%d' % (alg, i), rng.randrange(1, N), k, b'short r %d' % i, alg)
            assert r < 2 ** 248
        for want_high in (True, False):  # s on either side of 2^255: with and without the DER pad byte
            while True:
                d, k, msg = rng.randrange(1, N), rng.randrange(1, N), bytes(rng.randrange(256) for _ in range(40))
                e = int.from_bytes(hashlib.new(alg, msg).digest(), 'big')
                if (eo.sign(d, k, e)[1] >= 2 ** 255) == want_high:
                    break
            add_sign('%s_s_%s' % (alg, 'high' if want_high else 'low'), d, k, msg, alg)
    print('sign kats:', len(sign_kats))

    import ssl
    with open(os.path.join(HERE, 'send_kats.json'), 'w') as f:
        json.dump({'source': 'reference pyelliptic.ECC encrypt, highlevelcrypto.pointMult / verify over ' + ssl.OPENSSL_VERSION,
                   'recipient_keys': [r.privkey.rjust(32, b'\x00').hex() for r in recips],
                   'recipient_pubs': [(r.pubkey_x.rjust(32, b'\x00') + r.pubkey_y.rjust(32, b'\x00')).hex() for r in recips],
                   'encrypt_kats': encrypt_kats, 'pointmult_kats': pointmult_kats, 'sign_kats': sign_kats}, f, indent=1)
    print('wrote send_kats.json')


if __name__ == '__main__':
    main()
