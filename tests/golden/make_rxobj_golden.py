#!/usr/bin/env python3
"""Generate tests/golden/rxobj_kats.json -- broadcast and pubkey processing fixtures from the REFERENCE's own
primitives (build container only; needs /root/reference, read-only):

    BITMESSAGE_HOME=$(mktemp -d) PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_rxobj_golden.py

RIPEMD-160 needs OpenSSL's legacy provider; the script re-runs itself with an ``OPENSSL_CONF`` that activates
it, as make_ident_golden.py does.  ``ECC.sign`` and ``ECC.encrypt`` draw random nonces and ephemeral keys, so a
re-run gives a different but equally valid file; keys and messages are seeded.

``processbroadcast``, ``processpubkey`` and ``decryptAndCheckPubkeyPayload`` do ``'\\x04' + bytes`` and cannot run
under this Python.  As make_ident_golden.py does, the objects are composed here from the reference's
primitives (``makeCryptor(...).sign``, ``highlevelcrypto.encrypt`` / ``verify`` / ``pointMult``, ``encodeVarint``,
``encodeAddress``, ``decodeAddress``), and each case states, from how it was put together, the line that decides
it (``line``: null where the reference goes on to store), the fields the walk has read by then (``record``), the
signed data where ``verify`` is reached (``signed``: length and SHA-256), the digest a valid signature was made
under (``digest``: 1 SHA-1, 2 SHA-256) and the result.  The statements are checked with the primitives: a key
does or does not open the object, ``highlevelcrypto.verify`` says what the line claims about the signed data,
``fallback.RIPEMD160Hash`` gives the ripe the comparison needs, ``decodeVarint`` raises on the bytes said to be
malformed, the lengths are those the sanity checks compare.

This file holds what ident_kats.json lacks: clear v2 / v3 pubkeys with every returning line of
``processpubkey``, the crossings of the ripe / tag comparison with the checks behind it in ``processbroadcast``,
signing keys the curve refuses under the right ripe, the signature-before-ripe order of encrypted pubkeys,
stream varints of every width in every kind of header, and the front of ``processpubkey``'s v4 branch.

* ``subscriptions``: the address strings subscribed to; ``needed``: ``state.neededPubkeys`` as tag -> address.
* ``broadcasts``: ``obj``, ``plaintext`` (null where nothing decrypts it), ``expect`` (the ripe of the v2 / v3
  subscription key that opens a v4 broadcast).  ``pubkeys_v4``: ``obj``, ``plaintext`` (null where the reference
  never decrypts), ``expect`` (the ripe of the address in ``needed``), ``address``.  ``pubkeys``: ``obj``.
"""
import hashlib
import json
import os
import random
import subprocess
import sys
import tempfile
from binascii import hexlify

HERE = os.path.dirname(os.path.abspath(__file__))
REF_SRC = '/root/reference/src'
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
    from addresses import decodeAddress, decodeVarint, encodeAddress, encodeVarint, varintDecodeError
    from fallback import RIPEMD160Hash
    from pyelliptic.openssl import OpenSSL

    ALG = {1: OpenSSL.digest_ecdsa_sha1, 2: OpenSSL.EVP_sha256}
    rng = random.Random(20251024)

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

    def ref_ripe(key_s64, key_e64):
        return RIPEMD160Hash(hashlib.sha512(b'\x04' + key_s64 + b'\x04' + key_e64).digest()).digest()

    def ref_verify(signed, sig, key_s64):
        return bool(highlevelcrypto.verify(signed, sig, hexlify(b'\x04' + key_s64)))

    def sign(data, priv, alg):
        return highlevelcrypto.makeCryptor(hexlify(priv)).sign(data, digest_alg=ALG[alg])

    class Key(object):
        def __init__(self, pub_s=None):
            self.priv_s, self.priv_e = rand(32), rand(32)
            self.pub_s = pub_s or highlevelcrypto.pointMult(self.priv_s)
            self.pub_e = highlevelcrypto.pointMult(self.priv_e)
            self.ripe = ref_ripe(self.pub_s[1:], self.pub_e[1:])

    class Sender(object):
        """A key pair under an address version and stream, and what a subscriber to (or someone waiting for the
        pubkey of) that address holds: the private key and the ripe or tag it is looked up by."""

        def __init__(self, key, version, stream):
            self.key, self.version, self.stream = key, version, stream
            self.address = encodeAddress(version, stream, key.ripe)
            assert list(decodeAddress(self.address)) == ['success', version, stream, key.ripe]
            data = encodeVarint(version) + encodeVarint(stream) + key.ripe
            if version <= 3:
                self.priv, self.lookup = hashlib.sha512(data).digest()[:32], key.ripe
            else:
                self.priv, self.lookup = dsha(data)[:32], dsha(data)[32:]
            self.cryptor = highlevelcrypto.makeCryptor(hexlify(self.priv))
            self.pub = highlevelcrypto.pointMult(self.priv)

    def opens(sender, payload):
        try:
            return sender.cryptor.decrypt(payload)
        except Exception:  # noqa: BLE001 -- pyelliptic raises RuntimeError and plain Exception
            return None

    def header(object_type, version_bytes, stream_bytes):
        return be(rng.getrandbits(64), 8) + be(1761000000 + rng.randrange(1000), 8) + be(object_type, 4) + version_bytes + stream_bytes

    STREAMS = (1, 300, 70000, 2 ** 32)  # varints of 1, 3, 5 and 9 bytes
    good = Key()
    off_x = int.from_bytes(good.pub_s[1:33], 'big')
    off_curve = Key(pub_s=good.pub_s[:64] + bytes([good.pub_s[64] ^ 1]))
    assert (int.from_bytes(off_curve.pub_s[33:], 'big') ** 2 - off_x ** 3 - 7) % P != 0
    x_is_p = Key(pub_s=b'\x04' + be(P, 32) + good.pub_s[33:])

    # ------------------------------------------------------------------ senders, subscriptions, needed pubkeys
    S2, S3 = Sender(Key(), 2, 1), Sender(Key(), 3, 1)
    S3w = {s: Sender(Key(), 3, s) for s in STREAMS[1:]}
    S4 = Sender(Key(), 4, 1)
    S4w = {s: Sender(Key(), 4, s) for s in STREAMS[1:]}
    S3off, S3p = Sender(off_curve, 3, 1), Sender(x_is_p, 3, 1)
    S4off = Sender(off_curve, 4, 1)
    U3, U4 = Sender(Key(), 3, 1), Sender(Key(), 4, 1)  # nobody subscribes to these or waits for their pubkeys
    subscribed = [S2, S3, S4, S3off, S3p, S4off] + list(S3w.values()) + list(S4w.values())
    subscriptions = [s.address for s in subscribed]
    # pubkeys waited for: N4 and the wide streams; M4s / M4v stand in neededPubkeys under their own tag but with
    # an address of another stream / version (protocol.py:428, :423)
    N4, M4s, M4v = Sender(Key(), 4, 1), Sender(Key(), 4, 1), Sender(Key(), 4, 1)
    N4w = {s: Sender(Key(), 4, s) for s in STREAMS[1:]}
    needed = {s.lookup.hex(): s.address for s in [N4] + list(N4w.values())}
    needed[M4s.lookup.hex()] = encodeAddress(4, 2, M4s.key.ripe)
    needed[M4v.lookup.hex()] = encodeAddress(3, 1, M4v.key.ripe)

    class Case(object):
        pass

    def compose(head, pieces, priv_s, alg, to_pub, raw_siglen=None, cut=None, spoil=None, tail=b''):
        """head || encrypt(pieces || siglen || signature): where each piece lies, the plaintext as the cut or the
        spoiled byte leaves it, and the signature over head[8:] || pieces."""
        body = b''.join(b for _, b in pieces)
        sig = sign(head[8:] + body, priv_s, alg)
        pieces = pieces + [('siglen', raw_siglen or encodeVarint(len(sig))), ('sig', sig)]
        c = Case()
        c.at, pos = {}, 0
        for name, b in pieces:
            c.at[name] = (pos, pos + len(b))
            pos += len(b)
        full = b''.join(b for _, b in pieces) + tail
        if spoil is not None:
            spoil %= len(full)
            full = full[:spoil] + bytes([full[spoil] ^ 1]) + full[spoil + 1:]
        if cut is not None:
            full = full[:cut]
        c.head, c.full, c.alg = head, full, alg
        if to_pub is not None:
            c.obj = head + highlevelcrypto.encrypt(full, hexlify(to_pub))
        return c

    def field(c, name):
        a, b = c.at[name]
        return c.full[a:b]

    # ------------------------------------------------------------------ broadcasts
    broadcasts = []

    def broadcast(name, line, bv, sender, to=None, version=None, inner=None, outer=None, encoding=2, alg=2,
                  message=b'Subject:hello\nBody:a broadcast', signer=None, raw=None, bad=None, cut=None, spoil=None,
                  tag=None, bv_bytes=None, decrypts=True):
        """raw: field -> the bytes that stand for it; bad: the field whose raw bytes decodeVarint refuses."""
        to, raw = to or sender, raw or {}
        version = sender.version if version is None else version
        inner = sender.stream if inner is None else inner
        outer = sender.stream if outer is None else outer
        head = header(3, bv_bytes or encodeVarint(bv), raw.get('outer') or encodeVarint(outer))
        tag_off = len(head)
        if bv == 5:
            head += to.lookup if tag is None else tag
        pieces = [('version', encodeVarint(version)), ('stream', encodeVarint(inner)), ('behaviour', be(1, 4)),
                  ('key_s', sender.key.pub_s[1:]), ('key_e', sender.key.pub_e[1:])]
        if version >= 3:
            pieces += [('ntpb', raw.get('ntpb') or encodeVarint(1000)), ('extra', raw.get('extra') or encodeVarint(2000))]
        pieces += [('encoding', raw.get('encoding') or encodeVarint(encoding)),
                   ('mlen', raw.get('mlen') or encodeVarint(len(message))), ('message', message)]
        c = compose(head, pieces, (signer or sender).key.priv_s, alg, to.pub, raw.get('siglen'), cut, spoil)
        payload = c.obj[len(head):]
        if bad is not None:
            assert line == 'varint' and raises_varint(raw[bad]), name
        if decrypts:
            assert opens(to, payload) == c.full, name
        else:
            assert all(opens(s, payload) is None for s in subscribed), name
        key_s, key_e, sig = field(c, 'key_s'), field(c, 'key_e'), field(c, 'sig')
        ripe = ref_ripe(key_s, key_e)
        own = ripe if bv == 4 else dsha(encodeVarint(version) + encodeVarint(inner) + ripe)[32:]
        e = {'name': name, 'line': line, 'obj': c.obj.hex(), 'plaintext': c.full.hex() if decrypts else None,
             'expect': to.key.ripe.hex() if bv == 4 and decrypts else '', 'record': None, 'signed': None, 'digest': 0,
             'result': None}
        # how far the reference has read when it returns: 0 the header, 1 the sender's version, 2 its stream,
        # 3 the behaviour, the keys and their difficulty, 5 the encoding, 7 the message and the signature
        got = {760: -1, 801: 0, 810: 0, 820: 0, 830: 1, 838: 1, 848: 2, 882: 3, 893: 3, 901: 5, 916: 7, None: 7,
                 'varint': {'bv': -1, 'outer': -1, 'ntpb': 2, 'extra': 2, 'encoding': 3, 'mlen': 5, 'siglen': 5}.get(bad)}[line]
        if decrypts and got >= 0:
            rec = {'objectVersion': bv, 'objectStream': outer, 'tagOff': tag_off, 'payloadOff': len(head)}
            if got >= 1:
                rec['senderVersion'] = version
            if got >= 2:
                rec['senderStream'] = inner
            if got >= 3:
                rec.update(behaviour='00000001', nonceTrialsPerByte=1000 if version >= 3 else 0, extraBytes=2000 if version >= 3 else 0,
                           pubkeyData=c.full[:c.at['encoding'][0]].hex())
            if got >= 5:
                rec['encoding'] = encoding
            if got >= 7:
                rec.update(message=field(c, 'message').hex(), signature=sig.hex())
            e['record'] = rec
        elif not decrypts and line in (801, 810, 820):
            e['record'] = {'objectVersion': bv, 'objectStream': outer, 'tagOff': tag_off, 'payloadOff': len(head)}
        if line in (882, 893, 901, 916, None) or (line == 'varint' and bad in ('encoding', 'mlen', 'siglen')):
            assert (own == to.lookup) == (line not in (882, 893)), name        # :882 / :893
        if line in (916, None):
            signed = head[8:] + c.full[:c.at['message'][1]]
            e['signed'] = {'len': len(signed), 'sha256': hashlib.sha256(signed).hexdigest()}
            assert ref_verify(signed, sig, key_s) == (line is None), name
        if line is None:
            e['digest'] = alg
            e['result'] = {'fromAddress': encodeAddress(version, inner, ripe), 'ripe': ripe.hex(), 'sigHash': dsha(sig)[32:].hex()}
            assert e['result']['fromAddress'] == sender.address
        broadcasts.append(e)
        print('  broadcast %-44s line=%s' % (name, line))

    NM = b'\xfd\x00\x20'  # a varint that is not minimal
    for k, s in enumerate(STREAMS):
        broadcast('v4_ok_stream_%d' % s, None, 4, S3 if s == 1 else S3w[s], alg=1 + k % 2, message=rand(40 + 17 * k))
        broadcast('v5_ok_stream_%d' % s, None, 5, S4 if s == 1 else S4w[s], alg=2 - k % 2, message=rand(200 + 31 * k))
    broadcast('v4_ok_sender_v2', None, 4, S2, alg=1)
    broadcast('v5_ok_empty_message_encoding_3', None, 5, S4, encoding=3, message=b'')
    broadcast('broadcast_version_3', 760, 4, U3, bv_bytes=encodeVarint(3), decrypts=False)
    broadcast('broadcast_version_not_minimal', 'varint', 4, U3, bv_bytes=b'\xfd\x00\x04', decrypts=False,
              raw={'bv': b'\xfd\x00\x04'}, bad='bv')
    broadcast('outer_stream_not_minimal', 'varint', 5, U4, raw={'outer': b'\xfd\x00\x01'}, bad='outer', decrypts=False)
    broadcast('v4_no_key_decrypts', 801, 4, U3, decrypts=False)
    broadcast('v5_tag_unknown', 810, 5, U4, decrypts=False)
    broadcast('v5_tag_known_wrong_key', 820, 5, U4, tag=S4.lookup, decrypts=False)
    broadcast('v4_sender_version_4', 830, 4, S3, version=4)
    broadcast('v5_sender_version_3', 838, 5, S4, version=3)
    broadcast('v4_inner_stream_differs', 848, 4, S3, inner=2)
    broadcast('v5_inner_stream_differs_wide', 848, 5, S4w[2 ** 32], inner=2 ** 32 + 1)
    broadcast('v4_keys_of_another_sender', 882, 4, S2, to=S3, version=3)
    broadcast('v5_keys_of_another_sender', 893, 5, U4, to=S4)
    broadcast('v4_encoding_0', 901, 4, S3, encoding=0)
    broadcast('v5_encoding_0', 901, 5, S4, encoding=0)
    broadcast('v4_signed_by_another_key', 916, 4, S3, signer=S2)
    broadcast('v5_signature_bit_flipped', 916, 5, S4, spoil=-3)
    # the comparison sits in front of everything behind the keys
    broadcast('v4_wrong_ripe_and_encoding_0', 882, 4, U3, to=S3, encoding=0)
    broadcast('v4_wrong_ripe_and_encoding_not_minimal', 882, 4, U3, to=S3, raw={'encoding': NM})
    broadcast('v5_wrong_tag_and_mlen_not_minimal', 893, 5, U4, to=S4, raw={'mlen': NM})
    broadcast('v5_wrong_tag_and_siglen_not_minimal', 893, 5, U4, to=S4, raw={'siglen': b'\xfd\x00\x47'})
    broadcast('v5_right_tag_siglen_not_minimal', 'varint', 5, S4, raw={'siglen': b'\xfd\x00\x47'}, bad='siglen')
    broadcast('v5_right_tag_mlen_not_minimal', 'varint', 5, S4, raw={'mlen': NM}, bad='mlen')
    broadcast('v4_right_ripe_encoding_not_minimal', 'varint', 4, S3, raw={'encoding': NM}, bad='encoding')
    # ... and behind the difficulty varints
    broadcast('v4_wrong_ripe_and_ntpb_not_minimal', 'varint', 4, U3, to=S3, raw={'ntpb': NM}, bad='ntpb')
    broadcast('v5_right_tag_extra_not_minimal', 'varint', 5, S4, raw={'extra': NM}, bad='extra')
    # keys the curve kernels or the range check refuse, under the ripe and the tag made from them
    broadcast('v4_signing_key_off_the_curve_right_ripe', 916, 4, S3off, signer=S3)
    broadcast('v5_signing_key_off_the_curve_right_tag', 916, 5, S4off, signer=S4)
    broadcast('v4_signing_key_x_is_p_right_ripe', 916, 4, S3p, signer=S3)

    # ------------------------------------------------------------------ encrypted (v4) pubkeys
    pubkeys_v4 = []

    def pubkey_v4(name, line, owner, to=None, address=None, alg=2, signer=None, raw=None, bad=None, spoil=None,
                  obj_len=None, version_bytes=None, enc_to=None):
        to, raw = to or owner, raw or {}
        head = header(1, version_bytes or encodeVarint(4), raw.get('stream') or encodeVarint(owner.stream))
        tag_off = len(head)
        head += to.lookup
        pieces = [('behaviour', be(1, 4)), ('key_s', owner.key.pub_s[1:]), ('key_e', owner.key.pub_e[1:]),
                  ('ntpb', raw.get('ntpb') or encodeVarint(1000)), ('extra', raw.get('extra') or encodeVarint(2000))]
        c = compose(head, pieces, (signer or owner).key.priv_s, alg, (enc_to or to).pub, raw.get('siglen'), None, spoil)
        if obj_len is not None:
            c.obj = c.obj[:obj_len]
        if bad is not None:
            assert line == 'varint' and raises_varint(raw[bad]), name
        address = needed.get(to.lookup.hex()) if address is None else address
        plain = opens(to, c.obj[len(head):])
        front = {411: len(c.obj) < 350, 417: len(c.obj) >= 350 and to.lookup.hex() not in needed}
        assert (plain is None) == (line in (411, 457)) and (line not in front or front[line]), name
        if line in (423, 428):
            st, av, astream = decodeAddress(address)[:3]
            assert st == 'success' and ((av != 4) if line == 423 else (av == 4 and astream != owner.stream)), name
        decrypted = line not in (411, 417, 423, 428, 457) and not (line == 'varint' and bad in ('version', 'stream'))
        e = {'name': name, 'line': line, 'obj': c.obj.hex(), 'address': address, 'plaintext': c.full.hex() if decrypted else None,
             'expect': decodeAddress(address)[3].hex() if decrypted else '', 'record': None, 'signed': None, 'digest': 0,
             'result': None}
        if not (line == 'varint' and bad in ('version', 'stream')):
            e['record'] = {'objectVersion': 4, 'objectStream': owner.stream, 'tagOff': tag_off, 'payloadOff': len(head)}
        if decrypted and line != 'varint':
            end = c.at['siglen'][0]
            key_s, key_e, sig = field(c, 'key_s'), field(c, 'key_e'), field(c, 'sig')
            signed, stored = head[8:] + c.full[:end], head[20:tag_off] + c.full[:end]
            e['record'].update(behaviour='00000001', nonceTrialsPerByte=1000, extraBytes=2000, signature=sig.hex(),
                               storedData=stored.hex())
            e['signed'] = {'len': len(signed), 'sha256': hashlib.sha256(signed).hexdigest()}
            assert ref_verify(signed, sig, key_s) == (line in (None, 497)), name                       # :484
            if line in (None, 497):
                assert (ref_ripe(key_s, key_e) == decodeAddress(address)[3]) == (line is None), name   # :497
            if line is None:
                e['digest'] = alg
                e['result'] = {'fromAddress': address, 'ripe': owner.key.ripe.hex(), 'storedData': stored.hex()}
                assert address == owner.address
        pubkeys_v4.append(e)
        print('  pubkey_v4 %-44s line=%s' % (name, line))

    for k, s in enumerate(STREAMS):
        pubkey_v4('ok_stream_%d' % s, None, N4 if s == 1 else N4w[s], alg=1 + k % 2)
    pubkey_v4('signed_by_another_key', 484, N4, signer=U4)
    pubkey_v4('keys_of_another_address', 497, U4, to=N4)
    pubkey_v4('wrong_ripe_and_signature_bit_flipped', 484, U4, to=N4, spoil=-2)
    pubkey_v4('wrong_ripe_and_signed_by_another_key', 484, U4, to=N4, signer=N4)
    pubkey_v4('ntpb_not_minimal', 'varint', N4, raw={'ntpb': NM}, bad='ntpb')
    pubkey_v4('siglen_not_minimal_wrong_ripe', 'varint', U4, to=N4, raw={'siglen': b'\xfd\x00\x47'}, bad='siglen')
    pubkey_v4('stream_not_minimal', 'varint', N4, raw={'stream': b'\xfd\x00\x01'}, bad='stream')
    pubkey_v4('length_349', 411, N4, obj_len=349)
    pubkey_v4('length_350_does_not_decrypt', 457, N4, obj_len=350)
    pubkey_v4('tag_not_needed', 417, U4)
    pubkey_v4('needed_under_another_stream', 428, M4s)
    pubkey_v4('needed_under_another_version', 423, M4v)
    pubkey_v4('needed_tag_payload_for_another_key', 457, N4, enc_to=U4)

    # ------------------------------------------------------------------ clear (v2 / v3) pubkeys
    pubkeys = []

    def pubkey(name, line, key, version, stream=1, alg=2, signer=None, raw=None, bad=None, spoil=None, obj_len=None,
               tail=b''):
        raw = raw or {}
        head = header(1, raw.get('version') or encodeVarint(version), raw.get('stream') or encodeVarint(stream))
        pieces = [('behaviour', be(1, 4)), ('key_s', key.pub_s[1:]), ('key_e', key.pub_e[1:])]
        if version != 2:
            pieces += [('ntpb', raw.get('ntpb') or encodeVarint(1000)), ('extra', raw.get('extra') or encodeVarint(2000))]
        c = compose(head, pieces, (signer or key).priv_s, alg, None, raw.get('siglen'), None, None, tail)
        end = len(head) + c.at['siglen'][0]
        obj = head + (c.full if version != 2 else c.full[:c.at['siglen'][0]] + tail)
        if spoil is not None:
            spoil %= len(obj)
            obj = obj[:spoil] + bytes([obj[spoil] ^ 1]) + obj[spoil + 1:]
        if obj_len is not None:
            obj = obj[:obj_len]
        if bad is not None:
            assert line == 'varint' and raises_varint(raw[bad]), name
        e = {'name': name, 'line': line, 'obj': obj.hex(), 'record': None, 'signed': None, 'digest': 0, 'result': None}
        if not (line == 'varint' and bad in ('version', 'stream')):
            e['record'] = {'objectVersion': version, 'objectStream': stream}
        sanity = {293: version == 2 and len(obj) < 146, 346: version == 3 and len(obj) < 170,
                  304: version == 2 and len(obj) >= 146 and len(obj[len(head) + 68:len(head) + 132]) < 64,
                  283: version == 0, 287: version == 1 or version > 4, 410: version == 4}
        assert line not in sanity or sanity[line], name
        if version in (2, 3) and line in (None, 374):
            assert len(obj) >= (146 if version == 2 else 170), name
            ripe = ref_ripe(obj[len(head) + 4:len(head) + 68], obj[len(head) + 68:len(head) + 132])
            e['record'].update(behaviour='00000001', storedData=obj[20:end].hex())
            if version == 3:
                sig = obj[end + len(field(c, 'siglen')):][:len(field(c, 'sig'))]
                e['record'].update(nonceTrialsPerByte=1000, extraBytes=2000, signature=sig.hex())
                e['signed'] = {'len': end - 8, 'sha256': hashlib.sha256(obj[8:end]).hexdigest()}
                assert ref_verify(obj[8:end], sig, obj[len(head) + 4:len(head) + 68]) == (line is None), name  # :374
            if line is None:
                e['digest'] = alg if version == 3 else 0
                e['result'] = {'fromAddress': encodeAddress(version, stream, ripe), 'ripe': ripe.hex(),
                               'storedData': obj[20:end].hex()}
        pubkeys.append(e)
        print('  pubkey    %-44s line=%s len=%d' % (name, line, len(obj)))

    k2, k3 = Key(), Key()
    pubkey('v2_ok', None, k2, 2)
    pubkey('v2_ok_trailing_bytes', None, k2, 2, tail=rand(9))
    pubkey('v3_ok_sha1', None, k3, 3, alg=1)
    pubkey('v3_ok_sha256', None, k3, 3, alg=2)
    pubkey('v3_ok_trailing_bytes', None, k3, 3, tail=rand(5))
    for s in STREAMS[1:]:
        pubkey('v3_ok_stream_%d' % s, None, Key(), 3, stream=s, alg=1 + s % 2)
        pubkey('v2_ok_stream_%d' % s, None, Key(), 2, stream=s)
    pubkey('version_0', 283, k3, 0)
    pubkey('version_1', 287, k3, 1)
    pubkey('version_5', 287, k3, 5)
    pubkey('version_4_needs_decryption', 410, k3, 4)
    pubkey('version_not_minimal', 'varint', k3, 3, raw={'version': b'\xfd\x00\x03'}, bad='version')
    pubkey('stream_truncated', 'varint', k2, 2, raw={'stream': b'\xfe\x00\x01'}, bad='stream', obj_len=23)
    pubkey('v2_length_145', 293, k2, 2, obj_len=145)
    pubkey('v2_length_146_encryption_key_short', 304, k2, 2, obj_len=146)
    pubkey('v2_length_153_encryption_key_short', 304, k2, 2, obj_len=153)
    pubkey('v3_length_169', 346, k3, 3, obj_len=169)
    pubkey('v3_length_170_signature_cut_short', 374, k3, 3, obj_len=170)
    pubkey('v3_ntpb_not_minimal', 'varint', k3, 3, raw={'ntpb': NM}, bad='ntpb')
    pubkey('v3_extra_not_minimal', 'varint', k3, 3, raw={'extra': NM}, bad='extra')
    pubkey('v3_siglen_not_minimal', 'varint', k3, 3, raw={'siglen': b'\xfd\x00\x47'}, bad='siglen')
    pubkey('v3_signed_by_another_key', 374, k3, 3, signer=k2)
    pubkey('v3_signature_bit_flipped', 374, k3, 3, spoil=-3)
    pubkey('v3_encryption_key_bit_flipped', 374, k3, 3, spoil=100)
    pubkey('v3_signing_key_off_the_curve', 374, off_curve, 3, signer=k3)
    pubkey('v3_signing_key_x_is_p', 374, x_is_p, 3, signer=k3)
    pubkey('v2_signing_key_off_the_curve_is_stored', None, off_curve, 2)

    import ssl
    out = os.path.join(HERE, 'rxobj_kats.json')
    with open(out, 'w') as f:
        json.dump({'source': 'reference addresses.encodeAddress / decodeAddress / encodeVarint / decodeVarint, '
                             'fallback.RIPEMD160Hash, highlevelcrypto.encrypt / verify / pointMult / makeCryptor(...).sign / '
                             '.decrypt over ' + ssl.OPENSSL_VERSION,
                   'subscriptions': subscriptions, 'needed': needed, 'broadcasts': broadcasts, 'pubkeys_v4': pubkeys_v4,
                   'pubkeys': pubkeys}, f, indent=0, separators=(',', ':'))
    print('wrote rxobj_kats.json: %d broadcasts, %d encrypted and %d clear pubkeys, %d bytes' %
          (len(broadcasts), len(pubkeys_v4), len(pubkeys), os.path.getsize(out)))
    assert os.path.getsize(out) < 200 * 1024


if __name__ == '__main__':
    main()
