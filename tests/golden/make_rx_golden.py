#!/usr/bin/env python3
"""Generate tests/golden/rx_kats.json -- msg-processing fixtures from the REFERENCE's own primitives (build
container only; needs /root/reference, read-only):

    BITMESSAGE_HOME=$(mktemp -d) PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_rx_golden.py

RIPEMD-160 needs OpenSSL's legacy provider; the script re-runs itself with an ``OPENSSL_CONF`` that activates
it, as make_ident_golden.py does.  ``ECC.sign`` and ``ECC.encrypt`` draw random nonces and ephemeral keys, so a
re-run gives a different but equally valid file; keys and messages are seeded.

The reference's ``processmsg`` (``src/class_objectProcessor.py:435-747``) does ``'\\x04' + bytes`` and cannot run
under this Python.  As make_ident_golden.py does, the msgs are composed here from the reference's primitives
(``highlevelcrypto.makeCryptor(...).sign`` / ``encrypt`` / ``pointMult``, ``encodeVarint``, ``encodeAddress``), and
each case states, from how it was put together, the line that decides it (``line``: null where ``processmsg``
reaches ``:582``), the fields the walk has read by then (``record``) and the final result (``result``).  The
statements are checked with the reference's primitives: a recipient's key does or does not open the object
(``makeCryptor(...).decrypt``), ``highlevelcrypto.verify`` says what the line claims about the signed data put
together from the stated fields, ``fallback.RIPEMD160Hash`` and ``encodeAddress`` give ``ripe`` and
``fromAddress``, ``decodeVarint`` raises on the bytes said to be malformed.

* ``recipients``: the user's addresses: ripe and private encryption key (``shared.myECCryptorObjects``).
* ``msgs``: ``name``, ``line``, ``obj``, ``toRipe`` and ``plaintext`` (what the recipient's key decrypts the object
  to; for ``:444`` and ``:478`` rows, which never decrypt, the plaintext the sender made), ``decrypts``, ``record``,
  ``signed`` (length and SHA-256 of ``signedData`` where the walk reaches ``:566``), ``digest`` (1 SHA-1, 2
  SHA-256) and ``result`` (``fromAddress``, ``ripe``, ``sigHash``) or null.
* ``acks``: ``ackDataHasAValidHeader`` (``:1020-1054``) restated over ``protocol.Header``'s format
  (``'!L12sL4s'``): ``ack`` plus ``zeros`` further zero bytes, the ``line`` that returns False, or null for True.
"""
import hashlib
import json
import os
import random
import struct
import subprocess
import sys
import tempfile
from binascii import hexlify

HERE = os.path.dirname(os.path.abspath(__file__))
REF_SRC = '/root/reference/src'
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
P = 2 ** 256 - 2 ** 32 - 977
CNF = '''openssl_conf = openssl_init
[openssl_init]
providers = provider_sect
[provider_sect]
default = default_sect
legacy = legacy_sect
[default_sect]
activate = 1
[legacy_sect]
activate = 1
'''


def be(v, n):
    return v.to_bytes(n, 'big')


def der_int(v, pad=0):
    b = be(v, max(1, (v.bit_length() + 7) // 8))
    if b[0] & 0x80:
        b = b'\x00' + b
    b = bytes(pad) + b
    return b'\x02' + bytes([len(b)]) + b


def der_sig(r, s, pad=0):
    body = der_int(r, pad) + der_int(s)
    return b'\x30' + bytes([len(body)]) + body


def der_decode(sig):
    assert sig[0] == 0x30 and sig[1] == len(sig) - 2 and sig[2] == 2
    lr = sig[3]
    assert sig[4 + lr] == 2 and sig[5 + lr] == len(sig) - 6 - lr
    return int.from_bytes(sig[4:4 + lr], 'big'), int.from_bytes(sig[6 + lr:], 'big')


def main():
    try:
        hashlib.new('ripemd160')
    except ValueError:
        with tempfile.NamedTemporaryFile('w', suffix='.cnf', delete=False) as f:
            f.write(CNF)
        env = dict(os.environ, OPENSSL_CONF=f.name)
        sys.exit(subprocess.call([sys.executable] + sys.argv, env=env))
    sys.path.insert(0, REF_SRC)
    import highlevelcrypto
    from addresses import decodeVarint, encodeAddress, encodeVarint, varintDecodeError
    from fallback import RIPEMD160Hash
    from pyelliptic.openssl import OpenSSL

    ALG = {1: OpenSSL.digest_ecdsa_sha1, 2: OpenSSL.EVP_sha256}
    rng = random.Random(20251021)

    def rand(n):
        return bytes(rng.randrange(256) for _ in range(n))

    def dsha(data):
        return hashlib.sha512(hashlib.sha512(data).digest()).digest()

    def raises_varint(data):
        try:
            decodeVarint(data)
        except varintDecodeError:
            return True
        return False

    class Key(object):
        def __init__(self):
            self.priv_s, self.priv_e = rand(32), rand(32)
            self.pub_s, self.pub_e = highlevelcrypto.pointMult(self.priv_s), highlevelcrypto.pointMult(self.priv_e)
            self.ripe = RIPEMD160Hash(hashlib.sha512(self.pub_s + self.pub_e).digest()).digest()
            self.cryptor = highlevelcrypto.makeCryptor(hexlify(self.priv_e))

    me, me2, stranger, alice, mallory = Key(), Key(), Key(), Key(), Key()
    recipients = [{'ripe': k.ripe.hex(), 'privkey': k.priv_e.hex()} for k in (me, me2)]

    def opens(key, payload):
        try:
            return key.cryptor.decrypt(payload)
        except Exception:  # noqa: BLE001 -- pyelliptic raises RuntimeError and plain Exception
            return None

    msgs = []

    def msg(name, line, version=4, claimed=1, inner=1, to=me, dest=None, sender=alice, signer=None, alg=2,
            message=b'Subject:hi\nBody:a msg', ack=b'', encoding=2, raw=None, head_raw=None, cut=None, spoil=None,
            tail=b'', key_s=None, resign=None, msg_version=1, reads=None, bad_varint=None, obj_cut=None, note=None, vals=None,
            overshoot=None):
        """One msg.  raw: field name -> the bytes that stand for it in the plaintext (a malformed or long
        varint, a length that overshoots); head_raw: the same for the object's 'msgver' / 'stream'.  reads: how
        many fields of the walk's order the walk reads before `line` returns (default: by the line).  vals:
        the values those raw bytes stand for.  overshoot: 'mlen' / 'alen' where that length runs past the end,
        so that the slice runs to the end and everything behind it is empty."""
        raw, head_raw = raw or {}, head_raw or {}
        head = be(rng.getrandbits(64), 8) + be(1760990000 + rng.randrange(1000), 8) + be(2, 4)
        head += head_raw.get('msgver', encodeVarint(msg_version)) + head_raw.get('stream', encodeVarint(claimed))
        dest = dest or to
        pieces = [('version', raw.get('version', encodeVarint(version))), ('stream', raw.get('stream', encodeVarint(inner))),
                  ('behaviour', be(1, 4)), ('key_s', key_s or sender.pub_s[1:]), ('key_e', sender.pub_e[1:])]
        if version >= 3:
            pieces += [('ntpb', raw.get('ntpb', encodeVarint(1000))), ('extra', raw.get('extra', encodeVarint(1000)))]
        pieces += [('toRipe', dest.ripe), ('encoding', raw.get('encoding', encodeVarint(encoding))),
                   ('mlen', raw.get('mlen', encodeVarint(len(message)))), ('message', message),
                   ('alen', raw.get('alen', encodeVarint(len(ack)))), ('ack', ack)]
        body = b''.join(b for _, b in pieces)
        signed = head[8:20] + encodeVarint(1) + encodeVarint(claimed) + body
        sig = highlevelcrypto.makeCryptor(hexlify((signer or sender).priv_s)).sign(signed, digest_alg=ALG[alg])
        if resign:
            sig = resign(*der_decode(sig))
        pieces += [('slen', raw.get('slen', encodeVarint(len(sig)))), ('sig', sig), ('tail', tail)]
        at, pos = {}, 0
        for nm, b in pieces:
            at[nm] = (pos, pos + len(b))
            pos += len(b)
        full = b''.join(b for _, b in pieces)
        if spoil is not None:
            full = full[:spoil] + bytes([full[spoil] ^ 1]) + full[spoil + 1:]
        if cut is not None:
            full = full[:cut]
        obj = head + highlevelcrypto.encrypt(full, hexlify(to.pub_e))
        if obj_cut is not None:
            obj = obj[:obj_cut]
        payload = obj[len(head):]
        decrypts = line != 478 and line != 444 and obj_cut is None and 'msgver' not in head_raw and 'stream' not in head_raw
        if decrypts:
            assert opens(to, payload) == full, name
        else:
            assert line in (444, 478), name
            if line == 478:
                assert opens(me, payload) is None and opens(me2, payload) is None, name
        if bad_varint is not None:
            assert line in ('varint', 444) and raises_varint(bad_varint), name

        def fld(nm):
            a, b = at[nm]
            return full[a:b]

        # what the walk has read when `line` returns, in its order
        order = ['senderVersion', 'senderStream', 'behaviour', 'nonceTrialsPerByte', 'extraBytes',
                 'endOfThePublicKeyPosition', 'encoding', 'message', 'ackData', 'signature']
        values = {'senderVersion': version, 'senderStream': inner, 'behaviour': fld('behaviour').hex(),
                  'nonceTrialsPerByte': 1000 if version >= 3 else 0, 'extraBytes': 1000 if version >= 3 else 0,
                  'endOfThePublicKeyPosition': at['toRipe'][0], 'encoding': encoding,
                  'message': fld('message').hex(), 'ackData': fld('ack').hex(), 'signature': fld('sig').hex()}
        bottom, sig_now = min(at['ack'][1], len(full)), fld('sig')
        if overshoot:
            bottom, sig_now = len(full), b''
            values['signature'] = ''
            if overshoot == 'mlen':
                values.update({'message': full[at['message'][0]:].hex(), 'ackData': ''})
            else:
                values['ackData'] = full[at['ack'][0]:].hex()
        values.update(vals or {})
        if reads is None:
            reads = {444: 0, 478: 0, 492: 1, 496: 1, 500: 1, 506: 2, 531: 6, 566: 10, None: 10}[line]
        record = {k: values[k] for k in order[:reads]}
        entry = {'name': name, 'line': line, 'obj': obj.hex(), 'toRipe': to.ripe.hex(), 'plaintext': full.hex(),
                 'decrypts': decrypts, 'record': record, 'signed': None, 'digest': 0, 'result': None}
        if note:
            entry['note'] = note
        if line in (None, 566):
            signed_now = head[8:20] + encodeVarint(1) + encodeVarint(claimed) + full[:bottom]
            key64 = fld('key_s')
            valid = bool(highlevelcrypto.verify(signed_now, sig_now, hexlify(b'\x04' + key64)))
            assert valid == (line is None), name
            entry['signed'] = {'len': len(signed_now), 'sha256': hashlib.sha256(signed_now).hexdigest()}
            if line is None:
                ripe = RIPEMD160Hash(hashlib.sha512(b'\x04' + key64 + b'\x04' + fld('key_e')).digest()).digest()
                assert ripe == sender.ripe
                entry['digest'] = alg
                entry['result'] = {'fromAddress': encodeAddress(version, inner, ripe), 'ripe': ripe.hex(),
                                   'sigHash': dsha(fld('sig'))[32:].hex()}
        msgs.append(entry)
        print('  %-40s line=%-6s len=%d' % (name, line, len(full)))
        return entry, at, full

    # ---- the lines ----
    _, at4, full4 = msg('ok_v4', None)
    msg('msg_version_2', 444, msg_version=2)
    msg('not_mine', 478, to=stranger)
    msg('sender_version_0', 492, version=0, raw={'version': encodeVarint(0)}, reads=1)
    msg('sender_version_5', 496, version=5)
    msg('sender_stream_0', 506, inner=0)
    msg('to_ripe_of_my_other_address', 531, to=me, dest=me2)
    # a malformed varint behind a wrong toRipe is still :531
    msg('to_ripe_wrong_then_bad_varint', 531, to=me, dest=me2, raw={'encoding': b'\xfd\x00\x02'})
    msg('signed_by_another_key', 566, signer=mallory)
    msg('message_bit_flipped', 566, spoil=at4['message'][0] + 3)
    msg('signature_bit_flipped', 566, spoil=-3)
    # ---- sender versions, stream widths (prefix 14 / 16 / 18 / 22), digests ----
    for v in (1, 2, 3, 4):
        msg('ok_sender_v%d' % v, None, version=v, alg=1 if v % 2 else 2)
    for claimed in (252, 300, 70000, 2 ** 32, 2 ** 64 - 1):
        msg('ok_stream_%d' % claimed, None, claimed=claimed, inner=claimed, alg=1 if claimed == 300 else 2)
    msg('ok_sha1', None, alg=1, message=b'x' * 301, ack=rand(40))
    msg('ok_inner_stream_differs', None, claimed=1, inner=7)
    msg('ok_empty_message', None, message=b'', encoding=3)
    msg('ok_trailing_bytes_behind_signature', None, tail=b'junk behind')
    # ---- malformed varints: not minimal at every position, truncated wherever the end can fall in one ----
    msg('head_msgver_not_minimal', 444, head_raw={'msgver': b'\xfd\x00\x01'}, bad_varint=b'\xfd\x00\x01')
    msg('head_msgver_truncated', 444, head_raw={'msgver': b'\xfd\x00'}, obj_cut=22, bad_varint=b'\xfd\x00')
    msg('head_stream_not_minimal', 444, head_raw={'stream': b'\xfe\x00\x00\x00\x05'}, bad_varint=b'\xfe\x00\x00\x00\x05')
    msg('head_stream_truncated', 444, head_raw={'stream': b'\xff\x00\x00\x00\x01'}, obj_cut=26, bad_varint=b'\xff\x00\x00\x00\x01')
    msg('version_not_minimal', 'varint', raw={'version': b'\xfd\x00\x04'}, reads=0, bad_varint=b'\xfd\x00\x04')
    msg('version_truncated', 'varint', raw={'version': b'\xfd\x01'}, cut=2, reads=0, bad_varint=b'\xfd\x01')
    msg('stream_not_minimal', 'varint', raw={'stream': b'\xfd\x00\x01'}, reads=1, bad_varint=b'\xfd\x00\x01')
    msg('ntpb_not_minimal', 'varint', raw={'ntpb': b'\xfe\x00\x00\x03\xe8'}, reads=3, bad_varint=b'\xfe\x00\x00\x03\xe8')
    msg('extra_not_minimal', 'varint', raw={'extra': b'\xff' + be(1000, 8)}, reads=4, bad_varint=b'\xff' + be(1000, 8))
    msg('encoding_not_minimal', 'varint', raw={'encoding': b'\xfd\x00\x02'}, reads=6, bad_varint=b'\xfd\x00\x02')
    msg('mlen_not_minimal', 'varint', raw={'mlen': b'\xfd\x00\x15'}, reads=7, bad_varint=b'\xfd\x00\x15')
    msg('alen_not_minimal', 'varint', raw={'alen': b'\xfd\x00\x00'}, reads=8, bad_varint=b'\xfd\x00\x00')
    msg('slen_not_minimal', 'varint', raw={'slen': b'\xfd\x00\x47'}, reads=9, bad_varint=b'\xfd\x00\x47')
    # the 170-byte floor (:500) keeps the end out of the sender's stream, ntpb and extra varints (they end by
    # byte 160); the encoding varint can reach it behind 9-byte stream, ntpb and extra varints
    long3 = {'stream': encodeVarint(2 ** 32), 'ntpb': encodeVarint(2 ** 32 + 1), 'extra': encodeVarint(2 ** 33)}
    lv = {'nonceTrialsPerByte': 2 ** 32 + 1, 'extraBytes': 2 ** 33}
    e, at, full = msg('encoding_truncated', 'varint', inner=2 ** 32, raw=dict(long3, encoding=b'\xfd\x01\x00'), cut=181,
                      reads=6, bad_varint=b'\xfd', vals=lv)
    assert at['toRipe'][0] == 160 and at['encoding'][0] == 180
    e, at, full = msg('mlen_truncated', 'varint', inner=2 ** 32, raw=dict(long3, mlen=b'\xfe\x00\x01\x00\x00'), cut=185,
                      reads=7, bad_varint=b'\xfe\x00\x01\x00', vals=lv)
    assert at['mlen'][0] == 181
    e, at, full = msg('alen_truncated', 'varint', inner=2 ** 32, raw=dict(long3, alen=b'\xfd\x01\x00'), cut=205, reads=8,
                      bad_varint=b'\xfd\x01', vals=lv)
    assert at['alen'][0] == 203
    e, at, full = msg('slen_truncated', 'varint', inner=2 ** 32, raw=dict(long3, slen=b'\xfd\x01\x00'), cut=205, reads=9,
                      bad_varint=b'\xfd', vals=lv)
    assert at['slen'][0] == 204
    # ---- lengths: the floor of :500 ----
    e, at, full = msg('plaintext_169', 500, version=2, message=b'', cut=169)
    e, at, full = msg('plaintext_170', 566, version=2, message=b'', cut=170, note='the signature is cut short by the end')
    assert at['sig'][0] < 170 < at['sig'][1]
    # ---- clipping: Python cuts a slice at the end of the data ----
    for nm, v in (('past_the_end', len(b'Subject:hi\nBody:a msg') + 200), ('2_32', 2 ** 32), ('2_64_minus_1', 2 ** 64 - 1)):
        msg('mlen_%s' % nm, 566, raw={'mlen': encodeVarint(v)}, overshoot='mlen',
            note='message runs to the end; ackData and the signature are empty')
    msg('alen_past_the_end', 566, ack=rand(32), raw={'alen': encodeVarint(2 ** 64 - 1)}, overshoot='alen')
    e, at, full = msg('signature_cut_short', 566, cut=-1)
    e, at, full = msg('slen_past_the_end', None, raw={'slen': encodeVarint(2 ** 64 - 1)},
                      note='the signature slice is cut at the end of the data, where the signature ends')
    # ---- keys the curve code must refuse ----
    msg('key_x_is_p', 566, key_s=be(P, 32) + alice.pub_s[33:])
    y = int.from_bytes(alice.pub_s[33:], 'big')
    msg('key_off_the_curve', 566, key_s=alice.pub_s[1:33] + be((y + 1) % P, 32))
    # ---- DER ----
    msg('der_r_padded', 566, resign=lambda r, s: der_sig(r, s, pad=1), note='a zero byte the sign does not need')
    msg('der_r_is_n', 566, resign=lambda r, s: der_sig(N, s))
    msg('der_s_is_0', 566, resign=lambda r, s: der_sig(r, 0))

    # ---- ackData headers ----
    def packet(payload, magic=0xE9BEB4D9, command=b'object', length=None, checksum=None):
        return struct.pack('!L12sL4s', magic, command, len(payload) if length is None else length,
                           hashlib.sha512(payload).digest()[:4] if checksum is None else checksum) + payload

    def ref_ack(ack):
        """:1020-1054 with protocol.Header = Struct('!L12sL4s')"""
        if len(ack) < 24:
            return 1022
        magic, command, length, checksum = struct.unpack('!L12sL4s', ack[:24])
        if magic != 0xE9BEB4D9:
            return 1030
        payload = ack[24:]
        if len(payload) != length:
            return 1034
        if length > 1600100:
            return 1040
        if checksum != hashlib.sha512(payload).digest()[0:4]:
            return 1048
        if command.rstrip(b'\x00') != b'object':
            return 1052
        return None

    pay = rand(60)
    big = struct.pack('!L12sL4s', 0xE9BEB4D9, b'object', 1600101, hashlib.sha512(bytes(1600101)).digest()[:4])
    acks = []
    for nm, ack, zeros, line in (('valid', packet(pay), 0, None), ('valid_empty_payload', packet(b''), 0, None),
                                 ('short', packet(pay)[:23], 0, 1022), ('empty', b'', 0, 1022),
                                 ('magic', packet(pay, magic=0xE9BEB4D8), 0, 1030),
                                 ('length_differs', packet(pay, length=59), 0, 1034), ('payload_cut', packet(pay)[:-1], 0, 1034),
                                 ('payload_too_long', big, 1600101, 1040),
                                 ('checksum', packet(pay, checksum=b'\x00\x01\x02\x03'), 0, 1048),
                                 ('command_getdata', packet(pay, command=b'getdata'), 0, 1052),
                                 ('command_object_padded', packet(pay, command=b'object\x00\x00x'), 0, 1052)):
        assert ref_ack(ack + bytes(zeros)) == line, nm
        acks.append({'name': nm, 'ack': ack.hex(), 'zeros': zeros, 'line': line})

    import ssl
    path = os.path.join(HERE, 'rx_kats.json')
    with open(path, 'w') as f:
        json.dump({'source': 'reference addresses.encodeAddress / encodeVarint / decodeVarint, fallback.RIPEMD160Hash, '
                             'highlevelcrypto.encrypt / verify / pointMult / makeCryptor, pyelliptic ECC.sign over '
                             + ssl.OPENSSL_VERSION,
                   'recipients': recipients, 'msgs': msgs, 'acks': acks}, f, indent=0, separators=(',', ':'))
    print('wrote rx_kats.json: %d msgs, %d acks, %d bytes' % (len(msgs), len(acks), os.path.getsize(path)))


if __name__ == '__main__':
    main()
