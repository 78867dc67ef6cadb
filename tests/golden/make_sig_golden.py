#!/usr/bin/env python3
"""Generate tests/golden/sig_kats.json -- signature-verification fixtures from the REFERENCE's own
``pyelliptic.ECC`` and ``highlevelcrypto.verify`` over OpenSSL (build container only; needs
/root/reference, read-only):

    BITMESSAGE_HOME=$(mktemp -d) PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_sig_golden.py

``ECC.sign`` draws a random nonce and the keys are random too, so a re-run gives a different but equally
valid file; the messages and the constructed cases are seeded.

* ``cases``: (message, DER signature, key) triples with, from the reference, ``ECC(pubkey).verify(sig,
  msg, digest_alg)`` under SHA-1 and SHA-256 (``sha1`` / ``sha256``: true, false, or the string
  'raises' where building the key object or verifying raised) and the verdict of
  ``highlevelcrypto.verify`` (``verdict``).  ``code`` composes them as the library reports it (1 valid
  under SHA-1, 2 under SHA-256 only, 0 invalid); ``der_ok`` says whether the signature is a canonical DER
  pair with 1 <= r, s < n, i.e. whether a False is anything but structural.
* ``digest_cases``: (key, r, s, 32-byte digest) with the binding's ``ECDSA_verify`` on that digest.
* ``pubkey_objects`` / ``msg_objects``: whole v3 pubkey objects, and msg plaintexts with the head of
  their objects, signed by the reference over the ``signedData`` composed here, with truncated variants;
  ``parts`` is what ``processpubkey`` / ``processmsg`` hand to ``verify`` (null where they return before
  it), ``verdict`` what ``highlevelcrypto.verify`` says to that.
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

P = 2 ** 256 - 2 ** 32 - 977
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141


def be(v, n=32):
    return v.to_bytes(n, 'big')


def varint(v):
    if v < 253:
        return struct.pack('>B', v)
    if v < 65536:
        return b'\xfd' + struct.pack('>H', v)
    if v < 4294967296:
        return b'\xfe' + struct.pack('>I', v)
    return b'\xff' + struct.pack('>Q', v)


def der_int(v):
    b = be(v, max(1, (v.bit_length() + 7) // 8))
    if b[0] & 0x80:
        b = b'\x00' + b
    return b'\x02' + bytes([len(b)]) + b


def der_sig(r, s):
    body = der_int(r) + der_int(s)
    return b'\x30' + bytes([len(body)]) + body


def der_decode(sig):
    """(r, s) of a signature made by der_sig (the script's own, well-formed ones only)."""
    assert sig[0] == 0x30 and sig[1] == len(sig) - 2 and sig[2] == 2
    lr = sig[3]
    r = int.from_bytes(sig[4:4 + lr], 'big')
    assert sig[4 + lr] == 2 and sig[5 + lr] == len(sig) - 6 - lr
    return r, int.from_bytes(sig[6 + lr:], 'big')


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(1, REF_SRC)
    from oracle.addrgen_oracle import GX, GY, _add
    import highlevelcrypto
    from pyelliptic.ecc import ECC
    from pyelliptic.openssl import OpenSSL

    G = (GX, GY)
    ALG = {'sha1': OpenSSL.digest_ecdsa_sha1, 'sha256': OpenSSL.EVP_sha256}
    rng = random.Random(20251019)

    def mult(k, pt):
        acc = None
        k %= N
        while k:
            if k & 1:
                acc = _add(acc, pt)
            pt = _add(pt, pt)
            k >>= 1
        return acc

    def neg(pt):
        return None if pt is None else (pt[0], (P - pt[1]) % P)

    def lift(x):
        """(x, y) with the even y, or None when x^3 + 7 is no square."""
        y = pow((x * x * x + 7) % P, (P + 1) // 4, P)
        if y * y % P != (x * x * x + 7) % P:
            return None
        return (x, y if y % 2 == 0 else P - y)

    def digest_int(alg, msg):
        return int.from_bytes(hashlib.new(alg, msg).digest(), 'big')

    def pub64(e):
        return e.pubkey_x.rjust(32, b'\x00') + e.pubkey_y.rjust(32, b'\x00')

    def xy64(pt):
        return be(pt[0]) + be(pt[1])

    def ref_one(msg, sig, key64, alg):
        try:
            return bool(ECC(curve='secp256k1', pubkey=highlevelcrypto.hexToPubkey(hexlify(b'\x04' + key64)))
                        .verify(sig, msg, digest_alg=ALG[alg]))
        except Exception:  # noqa: BLE001 -- recorded: highlevelcrypto.verify's bare except turns it into False
            return 'raises'

    cases = []

    def add_case(name, msg, sig, key64, der_ok, expect=None):
        one, two = ref_one(msg, sig, key64, 'sha1'), ref_one(msg, sig, key64, 'sha256')
        verdict = bool(highlevelcrypto.verify(msg, sig, hexlify(b'\x04' + key64)))
        code = 1 if one is True else 2 if two is True else 0
        assert verdict == (code != 0), name
        assert der_ok or not verdict, name  # a structural refusal here is one in the reference too
        if expect is not None:
            assert code == expect, (name, code, expect)
        cases.append({'name': name, 'msg': msg.hex(), 'sig': sig.hex(), 'key': key64.hex(), 'sha1': one, 'sha256': two,
                      'verdict': verdict, 'code': code, 'der_ok': der_ok})
        print('  %-34s sha1=%-6s sha256=%-6s code=%d' % (name, one, two, code))

    # ---- keys: three full-width ones and one whose X has a leading zero byte ----
    keys = []
    while len(keys) < 4:
        e = ECC(curve='secp256k1')
        short = len(e.pubkey_x) == 31
        if (len(keys) == 3) != short or len(e.pubkey_y) != 32:
            continue
        keys.append(e)

    # ---- valid signatures under each digest, every padding edge ----
    lens = [0, 1, 55, 56, 63, 64, 65, 119, 120, 127, 128, 3001]
    for alg in ('sha1', 'sha256'):
        for i, ln in enumerate(lens):
            e = keys[i % len(keys)]
            msg = bytes(rng.randrange(256) for _ in range(ln))
            add_case('valid_%s_len%d' % (alg, ln), msg, e.sign(msg, digest_alg=ALG[alg]), pub64(e), True,
                     1 if alg == 'sha1' else 2)

    # ---- wrong message, wrong key, the negated key ----
    e0, e1 = keys[0], keys[1]
    msg0 = b'the quick brown fox jumps over the lazy dog' * 3
    sig0 = e0.sign(msg0, digest_alg=ALG['sha256'])
    while der_decode(sig0)[0] < 2 ** 255:  # an r whose DER integer carries a zero pad byte
        sig0 = e0.sign(msg0, digest_alg=ALG['sha256'])
    r0, s0 = der_decode(sig0)
    x0, y0 = int.from_bytes(e0.pubkey_x, 'big'), int.from_bytes(e0.pubkey_y, 'big')
    add_case('base_valid', msg0, sig0, pub64(e0), True, 2)
    add_case('wrong_message', msg0 + b'!', sig0, pub64(e0), True, 0)
    add_case('wrong_key', msg0, sig0, pub64(e1), True, 0)
    add_case('negated_key', msg0, sig0, be(x0) + be(P - y0), True, 0)

    # ---- refused keys ----
    small = next(lift(x) for x in range(1, 50) if lift(x))
    add_case('key_off_curve', msg0, sig0, be(x0) + be((y0 + 1) % P), True, 0)
    add_case('key_zero', msg0, sig0, bytes(64), True, 0)
    add_case('key_x_is_p', msg0, sig0, be(P) + be(y0), True, 0)
    add_case('key_y_is_p', msg0, sig0, be(x0) + be(P), True, 0)
    add_case('key_x_all_ones', msg0, sig0, b'\xff' * 32 + be(y0), True, 0)
    add_case('key_y_all_ones', msg0, sig0, be(x0) + b'\xff' * 32, True, 0)
    add_case('key_small_x', msg0, sig0, xy64(small), True, 0)
    add_case('key_small_x_plus_p', msg0, sig0, be(small[0] + P) + be(small[1]), True, 0)

    # ---- DER variants of one valid signature ----
    ri, si = der_int(r0), der_int(s0)
    assert ri[2] == 0  # the pad byte
    body = ri + si

    def seq(b):
        return b'\x30' + bytes([len(b)]) + b

    add_case('der_trailing_byte', msg0, sig0 + b'\x00', pub64(e0), False, 0)
    add_case('der_trailing_byte_counted', msg0, seq(body + b'\x00'), pub64(e0), False, 0)
    add_case('der_zero_padded_r', msg0, seq(b'\x02' + bytes([ri[1] + 1]) + b'\x00' + ri[2:] + si), pub64(e0), False, 0)
    add_case('der_long_form_length', msg0, b'\x30\x81' + bytes([len(body)]) + body, pub64(e0), False, 0)
    add_case('der_long_form_int_length', msg0, seq(b'\x02\x81' + ri[1:] + si), pub64(e0), False, 0)
    add_case('der_negative_r', msg0, seq(b'\x02' + bytes([ri[1] - 1]) + ri[3:] + si), pub64(e0), False, 0)
    add_case('der_r_zero', msg0, der_sig(0, s0), pub64(e0), False, 0)
    add_case('der_s_zero', msg0, der_sig(r0, 0), pub64(e0), False, 0)
    add_case('der_r_plus_n', msg0, der_sig(r0 + N, s0), pub64(e0), False, 0)
    add_case('der_s_plus_n', msg0, der_sig(r0, s0 + N), pub64(e0), False, 0)
    add_case('der_s_is_n', msg0, der_sig(r0, N), pub64(e0), False, 0)
    add_case('der_r_is_n', msg0, der_sig(N, s0), pub64(e0), False, 0)
    add_case('der_empty', msg0, b'', pub64(e0), False, 0)
    add_case('der_truncated', msg0, sig0[:-1], pub64(e0), False, 0)
    add_case('der_truncated_counted', msg0, seq(body[:-1]), pub64(e0), False, 0)
    add_case('der_wrong_tag', msg0, b'\x31' + sig0[1:], pub64(e0), False, 0)
    add_case('der_high_s', msg0, der_sig(r0, N - s0), pub64(e0), True, 2)

    # ---- constructed with a chosen R: Q = r^-1 (s R - e G) ----
    def recover(R, r, s, e):
        return mult(pow(r, -1, N), _add(mult(s, R), neg(mult(e, G))))

    msgc = b'constructed signature'
    for alg, want in (('sha1', 1), ('sha256', 2)):
        e = digest_int(alg, msgc)
        # (a) x(R) >= n: x = n + j for the first small j on the curve, r = j; and the twin at x = j
        j = next(j for j in range(1, 100) if lift(N + j) and lift(j))
        s = rng.randrange(1, N)
        for name, R in (('xR_above_n', lift(N + j)), ('xR_twin_below_n', lift(j))):
            add_case('%s_%s' % (name, alg), msgc, der_sig(j, s), xy64(recover(R, j, s, e)), True, want)
        # (b) R = infinity: r = -e / d
        d = rng.randrange(1, N)
        Q = mult(d, G)
        add_case('R_infinity_%s' % alg, msgc, der_sig(-e * pow(d, -1, N) % N, rng.randrange(1, N)), xy64(Q), True, 0)
        # (c) u1 G = u2 Q with a wrong signature: r = e / d; once with any s and once with u1 = e / s small,
        # a single comb window
        r = e * pow(d, -1, N) % N
        add_case('equal_halves_wrong_%s' % alg, msgc, der_sig(r, rng.randrange(1, N)), xy64(Q), True, 0)
        add_case('equal_halves_wrong_small_u1_%s' % alg, msgc, der_sig(r, e * pow(4660, -1, N) % N), xy64(Q), True, 0)
        # (d) valid, and the last addition is a doubling: r = x(k G) mod n, d = e / r, s = 2 e / k, Q = d G;
        # once with a random k and once with k / 2 inside one comb window
        for tag, k in (('', rng.randrange(1, N)), ('_small_u1', 2 * 0xbeef)):
            r = mult(k, G)[0] % N
            dd = e * pow(r, -1, N) % N
            add_case('valid_by_doubling%s_%s' % (tag, alg), msgc, der_sig(r, 2 * e * pow(k, -1, N) % N),
                     xy64(mult(dd, G)), True, want)

    # ---- digest-level cases: ECDSA_verify on a given 32-byte digest ----
    def ref_digest(key64, sig, digest):
        key = OpenSSL.EC_KEY_new_by_curve_name(OpenSSL.get_curve('secp256k1'))
        bx = OpenSSL.BN_bin2bn(key64[:32], 32, 0)
        by = OpenSSL.BN_bin2bn(key64[32:], 32, 0)
        group = OpenSSL.EC_KEY_get0_group(key)
        pt = OpenSSL.EC_POINT_new(group)
        try:
            if OpenSSL.EC_POINT_set_affine_coordinates_GFp(group, pt, bx, by, 0) == 0:
                return False
            if OpenSSL.EC_KEY_set_public_key(key, pt) == 0 or OpenSSL.EC_KEY_check_key(key) == 0:
                return False
            return OpenSSL.ECDSA_verify(0, OpenSSL.malloc(digest, 32), 32, OpenSSL.malloc(sig, len(sig)), len(sig), key) == 1
        finally:
            OpenSSL.EC_KEY_free(key)
            OpenSSL.BN_free(bx)
            OpenSSL.BN_free(by)
            OpenSSL.EC_POINT_free(pt)

    digest_cases = []
    for name, e in (('e_zero', 0), ('e_is_n', N), ('e_is_n_plus_1', N + 1), ('e_all_ones', 2 ** 256 - 1),
                    ('e_sha1_sized', rng.getrandbits(160)), ('e_random', rng.getrandbits(256))):
        k, s = rng.randrange(1, N), rng.randrange(1, N)
        R = mult(k, G)
        r = R[0] % N
        Q = recover(R, r, s, e)
        for tag, ee in (('', e), ('_other_digest', (e + 1) % 2 ** 256)):
            valid = ref_digest(xy64(Q), der_sig(r, s), be(ee))
            assert valid == (tag == ''), (name, tag)
            digest_cases.append({'name': name + tag, 'key': xy64(Q).hex(), 'r': be(r).hex(), 's': be(s).hex(),
                                 'e': be(ee).hex(), 'valid': valid})
            print('  digest %-28s valid=%s' % (name + tag, valid))

    # ---- whole objects for the extractors ----
    def obj_entry(name, fields, parts):
        verdict = None
        if parts is not None:
            verdict = bool(highlevelcrypto.verify(parts[0], parts[1], hexlify(b'\x04' + parts[2])))
        entry = dict(name=name, verdict=verdict,
                     parts=None if parts is None else {'signed': parts[0].hex(), 'sig': parts[1].hex(), 'key': parts[2].hex()})
        entry.update({k: v.hex() for k, v in fields.items()})
        print('  object %-30s verdict=%s' % (name, verdict))
        return entry

    pubkey_objects, msg_objects = [], []
    for i, (alg, stream, ntpb, extra) in enumerate((('sha256', 1, 1000, 1000), ('sha1', 300, 70000, 14000))):
        signer, enc = keys[i], keys[i + 2]
        head = be(rng.getrandbits(64), 8) + be(1760000000 + i, 8) + be(1, 4)
        signed_tail = varint(3) + varint(stream) + be(1, 4) + pub64(signer) + pub64(enc) + varint(ntpb) + varint(extra)
        signed = head[8:] + signed_tail
        sig = signer.sign(signed, digest_alg=ALG[alg])
        obj = head + signed_tail + varint(len(sig)) + sig
        pubkey_objects.append(obj_entry('pubkey_v3_%s' % alg, {'obj': obj}, (signed, sig, pub64(signer))))
        assert pubkey_objects[-1]['verdict'] is True
        if i == 0:
            pubkey_objects.append(obj_entry('pubkey_v3_below_170', {'obj': obj[:169]}, None))
            pubkey_objects.append(obj_entry('pubkey_v3_cut_in_signature', {'obj': obj[:-5]}, (signed, sig[:-5], pub64(signer))))
            assert pubkey_objects[-1]['verdict'] is False
    for i, (alg, ver, stream, text) in enumerate((('sha256', 4, 1, b'Subject:hi\nBody:' + b'x' * 300),
                                                 ('sha1', 3, 2, b'y' * 260))):
        signer, enc = keys[3 - i], keys[i]
        head = be(rng.getrandbits(64), 8) + be(1760000100 + i, 8) + be(2, 4)
        objhead = head + varint(1) + varint(stream)
        ack = bytes(rng.randrange(256) for _ in range(32)) if i == 0 else b''
        plain = (varint(ver) + varint(stream) + be(1, 4) + pub64(signer) + pub64(enc) + varint(1000) + varint(1000) +
                 bytes(rng.randrange(256) for _ in range(20)) + varint(2) + varint(len(text)) + text + varint(len(ack)) + ack)
        signed = head[8:] + varint(1) + varint(stream) + plain
        sig = signer.sign(signed, digest_alg=ALG[alg])
        full = plain + varint(len(sig)) + sig
        obj = objhead + bytes(rng.randrange(256) for _ in range(40))  # the encrypted part is not read
        msg_objects.append(obj_entry('msg_v%d_%s' % (ver, alg), {'obj': obj, 'plaintext': full}, (signed, sig, pub64(signer))))
        assert msg_objects[-1]['verdict'] is True
        if i == 0:
            msg_objects.append(obj_entry('msg_below_170', {'obj': obj, 'plaintext': full[:169]}, None))
            msg_objects.append(obj_entry('msg_cut_in_signature', {'obj': obj, 'plaintext': full[:-3]},
                                         (signed, sig[:-3], pub64(signer))))
            assert msg_objects[-1]['verdict'] is False
            msg_objects.append(obj_entry('msg_sender_version_0', {'obj': obj, 'plaintext': varint(0) + full[1:]}, None))
            msg_objects.append(obj_entry('msg_sender_version_5', {'obj': obj, 'plaintext': varint(5) + full[1:]}, None))
            msg_objects.append(obj_entry('msg_sender_stream_0', {'obj': obj, 'plaintext': full[:1] + varint(0) + full[2:]}, None))

    import ssl
    with open(os.path.join(HERE, 'sig_kats.json'), 'w') as f:
        json.dump({'source': 'reference pyelliptic.ECC sign / verify and highlevelcrypto.verify over ' + ssl.OPENSSL_VERSION,
                   'cases': cases, 'digest_cases': digest_cases, 'pubkey_objects': pubkey_objects,
                   'msg_objects': msg_objects}, f, indent=1)
    print('wrote sig_kats.json: %d cases, %d digest cases' % (len(cases), len(digest_cases)))


if __name__ == '__main__':
    main()
