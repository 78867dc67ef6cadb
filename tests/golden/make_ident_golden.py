#!/usr/bin/env python3
"""Generate tests/golden/ident_kats.json -- sender-identification fixtures from the REFERENCE's own
primitives (build container only; needs /root/reference, read-only):

    BITMESSAGE_HOME=$(mktemp -d) PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_ident_golden.py

RIPEMD-160 needs OpenSSL's legacy provider; the script re-runs itself with an ``OPENSSL_CONF`` that
activates it, as make_addr_golden.py does.  ``ECC.sign`` and ``ECC.encrypt`` draw random nonces and
ephemeral keys, so a re-run gives a different but equally valid file; keys, ripes and messages are seeded.

The reference's ``processbroadcast`` and ``decryptAndCheckPubkeyPayload`` do ``'\\x04' + bytes`` and cannot
run under this Python.  As make_sig_golden.py does, the objects are composed here from the reference's
primitives (``highlevelcrypto.sign`` / ``encrypt`` / ``pointMult``, ``encodeVarint``, ``encodeAddress``), and
each case states, from how it was put together, the reference line that decides it, what the extractor must
hand on and the final result.  The statements are checked with the reference's primitives: the subscription
key does or does not open the object (``makeCryptor(...).decrypt``), ``highlevelcrypto.verify`` says what the
line claims, ``fallback.RIPEMD160Hash`` gives the ripe the comparison needs, ``decodeVarint`` raises on the
bytes said to be malformed.

* ``addresses``: ``encodeAddress(version, stream, ripe)`` and ``decodeAddress`` of the result (null where it is
  ``'success'`` with the same version, stream and ripe); ``edge_addresses``: ``encodeAddress`` for version 0,
  stream 0 and 2^64 - 1; and
  ``malformed``: ``decodeAddress`` of strings that reach every status string a string can reach
  (``'otherproblem'`` stands behind conditions that exclude one another, ``src/addresses.py:250-263``).
* ``keys``: key pairs with the reference's ripe, the one- and two-zero-byte keys of addr_kats.json included.
* ``subscriptions``: addresses with the private key and the lookup value (ripe or tag) a subscriber derives
  from them.
* ``broadcasts`` / ``pubkeys_v4``: objects with the line that decides them, what the extractor must return
  for (object, plaintext), and ``result``: what the final record adds to those parts (``fromAddress``,
  ``ripe``, ``sigHash``) or null.
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
    from addresses import (decodeAddress, decodeVarint, encodeAddress, encodeBase58, encodeVarint,
                           varintDecodeError)
    from fallback import RIPEMD160Hash

    rng = random.Random(20251020)

    def rand(n):
        return bytes(rng.randrange(256) for _ in range(n))

    def dsha(data):
        return hashlib.sha512(hashlib.sha512(data).digest()).digest()

    def ripe_of(pubs, pube):
        return RIPEMD160Hash(hashlib.sha512(pubs + pube).digest()).digest()

    def decoded(address):
        status, version, stream, ripe = decodeAddress(address)
        return [status, version, stream, hexlify(ripe).decode() if ripe else '']

    # ------------------------------------------------------------------ addresses
    addresses = []
    for zeros in (0, 1, 2, 3, 19, 20):
        for version in (1, 2, 3, 4, 5, 252, 253):
            for stream in (1, 252, 253, 65535, 65536, 2 ** 32, 2 ** 64 - 1):
                ripe = bytes(zeros) + bytes(rng.randrange(1, 256) for _ in range(20 - zeros))
                address = encodeAddress(version, stream, ripe)
                back = decoded(address)
                addresses.append({'version': version, 'stream': stream, 'ripe': ripe.hex(), 'address': address,
                                  'decoded': None if back == ['success', version, stream, ripe.hex()] else back})
    print('addresses:', len(addresses))
    # beyond the protocol's versions and streams: what encodeAddress makes of version 0 (the data's leading zero
    # byte vanishes in the integer), stream 0 and the largest varints
    edge_addresses = []
    for zeros in (0, 1, 20):
        for version, stream in ((0, 1), (0, 0), (0, 2 ** 64 - 1), (1, 0), (4, 0), (2 ** 64 - 1, 1), (2 ** 64 - 1, 2 ** 64 - 1)):
            ripe = bytes(zeros) + bytes(rng.randrange(1, 256) for _ in range(20 - zeros))
            edge_addresses.append({'version': version, 'stream': stream, 'ripe': ripe.hex(),
                                   'address': encodeAddress(version, stream, ripe)})

    def raw_address(data):
        return 'BM-' + encodeBase58(int(hexlify(data + dsha(data)[:4]), 16))

    good = encodeAddress(4, 1, rand(20))
    r20 = bytes(rng.randrange(1, 256) for _ in range(20))
    malformed = [('zero_digit', good[:10] + '0' + good[11:]), ('space_inside', good[:10] + ' ' + good[11:]),
                 ('empty', ''), ('only_prefix', 'BM-'),
                 ('last_character_changed', good[:-1] + ('2' if good[-1] != '2' else '3')),
                 ('version_varint_not_minimal', raw_address(b'\xfd\x00\x04' + b'\x01' + r20)),
                 ('version_varint_truncated', raw_address(b'\xff\x01\x02')),
                 ('stream_varint_not_minimal', raw_address(b'\x04\xfe\x00\x00\x00\x01' + r20)),
                 ('stream_varint_truncated', raw_address(b'\x03\xfd')),
                 ('version_5', encodeAddress(5, 1, r20)), ('version_253', encodeAddress(253, 1, r20)),
                 ('no_data_version_0', raw_address(b'')),
                 ('v3_ripe_17', raw_address(b'\x03\x01' + r20[:17])), ('v2_ripe_0', raw_address(b'\x02\x01')),
                 ('v4_ripe_3', raw_address(b'\x04\x01' + r20[:3])), ('v4_ripe_all_zero', encodeAddress(4, 1, bytes(20))),
                 ('v3_ripe_21', raw_address(b'\x03\x01' + r20 + b'\x07')), ('v4_ripe_21', raw_address(b'\x04\x01' + r20 + b'\x07')),
                 ('v4_leading_zero_kept', raw_address(b'\x04\x01' + b'\x00' + r20[:19])),
                 ('v4_ripe_4', raw_address(b'\x04\x01' + r20[:4])), ('v1', raw_address(b'\x01\x01' + r20)),
                 ('no_prefix', good[3:]), ('whitespace_around', '  ' + good + '\n')]
    malformed = [{'name': n, 'address': a, 'decoded': decoded(a)} for n, a in malformed]
    seen = sorted({m['decoded'][0] for m in malformed})
    print('statuses:', seen)
    assert seen == ['checksumfailed', 'encodingproblem', 'invalidcharacters', 'ripetoolong', 'ripetooshort', 'success',
                    'varintmalformed', 'versiontoohigh']

    # ------------------------------------------------------------------ keys
    class Key(object):
        def __init__(self, priv_s, priv_e):
            self.priv_s, self.priv_e = priv_s, priv_e
            self.pub_s, self.pub_e = highlevelcrypto.pointMult(priv_s), highlevelcrypto.pointMult(priv_e)
            self.ripe = ripe_of(self.pub_s, self.pub_e)

    keys = [Key(rand(32), rand(32)) for _ in range(32)]
    with open(os.path.join(HERE, 'addr_kats.json')) as f:
        for s in json.load(f)['search_kats']:
            pp = bytes.fromhex(s['passphrase'])
            k = Key(hashlib.sha512(pp + encodeVarint(2 * s['k'])).digest()[:32],
                    hashlib.sha512(pp + encodeVarint(2 * s['k'] + 1)).digest()[:32])
            assert k.ripe.hex() == s['ripe'] and k.ripe[:s['null_bytes']] == bytes(s['null_bytes'])
            keys.append(k)
    key_rows = [{'pub_signing': k.pub_s.hex(), 'pub_encryption': k.pub_e.hex(), 'ripe': k.ripe.hex()} for k in keys]
    print('keys:', len(key_rows), 'with leading zero bytes:', sum(k.ripe[0] == 0 for k in keys))

    # ------------------------------------------------------------------ senders and subscriptions
    class Sender(object):
        """A key pair under an address version and stream, and what a subscriber to that address holds: the
        private key that opens the sender's broadcasts (and, for version 4, its encrypted pubkey) and the value
        it is looked up by -- the ripe up to version 3, the tag from version 4."""

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

    zero1 = next(k for k in keys if k.ripe[0] == 0 and k.ripe[1] != 0)
    zero2 = next(k for k in keys if k.ripe[:2] == b'\x00\x00')
    S2, S3, S3z = Sender(keys[0], 2, 1), Sender(keys[1], 3, 1), Sender(zero2, 3, 300)
    S4, S4z, S4s = Sender(keys[2], 4, 1), Sender(zero1, 4, 1), Sender(keys[3], 4, 70000)
    subscribed = [S2, S3, S3z, S4, S4z, S4s]
    U3, U4 = Sender(keys[4], 3, 1), Sender(keys[5], 4, 1)  # nobody subscribes to these
    subscriptions = [{'address': s.address, 'version': s.version, 'stream': s.stream, 'ripe': s.key.ripe.hex(),
                      'lookup_key': s.lookup.hex(), 'privkey': s.priv.hex()} for s in subscribed]

    def opens(sender, payload):
        """The plaintext under the sender's subscription key, or None where the reference's decrypt raises."""
        try:
            return sender.cryptor.decrypt(payload)
        except Exception:  # noqa: BLE001 -- pyelliptic raises RuntimeError and plain Exception
            return None

    def raises_varint(data):
        try:
            decodeVarint(data)
        except varintDecodeError:
            return True
        return False

    def ref_ripe(key_s64, key_e64):
        return RIPEMD160Hash(hashlib.sha512(b'\x04' + key_s64 + b'\x04' + key_e64).digest()).digest()

    class Case(object):
        """An object as it was put together: the bytes in front of the encrypted part, the plaintext, and
        where each field of the plaintext starts and ends."""

    def compose(head, pieces, signer, to, cut=None, spoil=None):
        body = b''.join(b for _, b in pieces)
        sig = highlevelcrypto.sign(head[8:] + body, hexlify(signer.key.priv_s))
        pieces = pieces + [('siglen', encodeVarint(len(sig))), ('sig', sig)]
        c = Case()
        c.at, pos = {}, 0
        for name, b in pieces:
            c.at[name] = (pos, pos + len(b))
            pos += len(b)
        full = body + encodeVarint(len(sig)) + sig
        if spoil is not None:
            full = full[:spoil] + bytes([full[spoil] ^ 1]) + full[spoil + 1:]
        if cut is not None:
            full = full[:cut]
        c.head, c.full, c.to = head, full, to
        c.obj = head + highlevelcrypto.encrypt(full, hexlify(to.pub))
        return c

    def field(c, name, end=None):
        """The bytes of a field as far as the (possibly cut) plaintext holds them."""
        a, b = c.at[name]
        return c.full[a:b if end is None else end]

    # ------------------------------------------------------------------ broadcasts
    def broadcast(bv, sender, to=None, version=None, inner_stream=None, outer_stream=None, encoding=2,
                  message=b'Subject:hello\nBody:a broadcast', signer=None, tag=None, raw_ntpb=None, cut=None,
                  spoil=None, bv_bytes=None, stream_bytes=None):
        """One broadcast.  to: the subscription whose key it is encrypted to (default: the sender's own)."""
        to = to or sender
        version = sender.version if version is None else version
        inner = sender.stream if inner_stream is None else inner_stream
        outer = sender.stream if outer_stream is None else outer_stream
        head = be(rng.getrandbits(64), 8) + be(1760900000 + rng.randrange(1000), 8) + be(3, 4)
        head += (bv_bytes or encodeVarint(bv)) + (stream_bytes or encodeVarint(outer))
        if bv == 5:
            head += to.lookup if tag is None else tag
        pieces = [('version', encodeVarint(version)), ('stream', encodeVarint(inner)), ('behaviour', be(1, 4)),
                  ('key_s', sender.key.pub_s[1:]), ('key_e', sender.key.pub_e[1:])]
        if version >= 3:
            pieces += [('ntpb', raw_ntpb or encodeVarint(1000)), ('extra', encodeVarint(1000))]
        pieces += [('encoding', encodeVarint(encoding)), ('mlen', encodeVarint(len(message))), ('message', message)]
        c = compose(head, pieces, signer or sender, to, cut, spoil)
        c.bv, c.version, c.inner, c.encoding, c.sender = bv, version, inner, encoding, sender
        return c

    broadcasts = []

    def add_broadcast(name, line, c, decrypts=True, parts=None, bad_varint=None):
        """line: where processbroadcast returns (None: it goes on to store the message).  decrypts: a
        subscription key opens the object.  parts: the plaintext gets through the extractor (default: wherever
        the reference reaches its comparisons with every varint read)."""
        payload = c.obj[len(c.head):]
        if parts is None:
            parts = decrypts and line in (None, 882, 893, 916)
        if bad_varint is not None:
            assert line == 'varint' and raises_varint(bad_varint), name
        if decrypts:
            assert opens(c.to, payload) == c.full, name
        else:
            assert line in (760, 801, 810, 820, 'varint') and all(opens(s, payload) is None for s in subscribed), name
        entry = {'name': name, 'line': line, 'obj': c.obj.hex(), 'plaintext': c.full.hex() if decrypts else None,
                 'parts': None, 'result': None}
        if parts:
            key_s, key_e = field(c, 'key_s'), field(c, 'key_e')
            signed = c.head[8:] + c.full[:c.at['message'][1]]
            sig = field(c, 'sig')
            entry['parts'] = {'signedData': signed.hex(), 'signature': sig.hex(), 'pubSigningKey64': key_s.hex(),
                              'pubEncryptionKey64': key_e.hex(), 'senderVersion': c.version, 'senderStream': c.inner,
                              'encoding': c.encoding, 'message': field(c, 'message').hex(),
                              'pubkeyData': c.full[:c.at['encoding'][0]].hex()}
            ripe = ref_ripe(key_s, key_e)
            own = ripe if c.bv == 4 else dsha(encodeVarint(c.version) + encodeVarint(c.inner) + ripe)[32:]
            assert (own == c.to.lookup) == (line in (None, 916)), name        # :882 / :893
            if line in (None, 916):
                assert bool(highlevelcrypto.verify(signed, sig, hexlify(b'\x04' + key_s))) == (line is None), name
            if line is None:
                entry['result'] = {'fromAddress': encodeAddress(c.version, c.inner, ripe), 'ripe': ripe.hex(),
                                   'sigHash': dsha(sig)[32:].hex()}
                assert entry['result']['fromAddress'] == c.sender.address
        broadcasts.append(entry)
        print('  broadcast %-36s line=%-6s %s' % (name, line, entry['result']['fromAddress'] if entry['result'] else ''))

    add_broadcast('v4_sender_v2', None, broadcast(4, S2))
    add_broadcast('v4_sender_v3', None, broadcast(4, S3))
    add_broadcast('v4_sender_v3_two_zero_bytes', None, broadcast(4, S3z))
    add_broadcast('v5_sender_v4', None, broadcast(5, S4))
    add_broadcast('v5_sender_v4_one_zero_byte', None, broadcast(5, S4z, message=b'x' * 300))
    add_broadcast('v5_sender_v4_stream_70000', None, broadcast(5, S4s, encoding=3, message=b''))
    # a v5 sender cannot be subscribed to (decodeAddress: 'versiontoohigh'): under the tag and key of a v4
    # subscription its own tag, made with version 5, differs
    add_broadcast('v5_sender_v5', 893, broadcast(5, S4, version=5))
    for bv in (3, 6):
        add_broadcast('broadcast_version_%d' % bv, 760, broadcast(4, U3, bv_bytes=encodeVarint(bv)), decrypts=False)
    add_broadcast('broadcast_version_varint_not_minimal', 'varint', broadcast(4, U3, bv_bytes=b'\xfd\x00\x04'),
                  decrypts=False, bad_varint=b'\xfd\x00\x04')
    add_broadcast('stream_varint_not_minimal', 'varint', broadcast(5, U4, stream_bytes=b'\xfd\x00\x01'),
                  decrypts=False, bad_varint=b'\xfd\x00\x01')
    add_broadcast('v4_no_key_decrypts', 801, broadcast(4, U3), decrypts=False)
    c = broadcast(5, U4)
    assert all(c.head[22:54] != s.lookup for s in subscribed)
    add_broadcast('v5_tag_unknown', 810, c, decrypts=False)
    c = broadcast(5, U4, tag=S4.lookup[:18])  # the object ends inside the tag
    c.obj = c.head
    add_broadcast('v5_tag_cut_short', 810, c, decrypts=False)
    add_broadcast('v5_tag_known_wrong_key', 820, broadcast(5, U4, tag=S4.lookup), decrypts=False)
    add_broadcast('v4_sender_version_4', 830, broadcast(4, S3, version=4))
    add_broadcast('v4_sender_version_1', 830, broadcast(4, S3, version=1))
    add_broadcast('v5_sender_version_3', 838, broadcast(5, S4, version=3))
    add_broadcast('v4_inner_stream_differs', 848, broadcast(4, S3, inner_stream=2))
    add_broadcast('v5_outer_stream_differs', 848, broadcast(5, S4, outer_stream=2))
    add_broadcast('v4_keys_of_another_sender', 882, broadcast(4, S2, to=S3, version=3))
    add_broadcast('v4_keys_of_unsubscribed_sender', 882, broadcast(4, U3, to=S3))
    add_broadcast('v5_keys_of_another_sender', 893, broadcast(5, U4, to=S4))
    add_broadcast('v5_sender_stream_not_subscribed', 893, broadcast(5, S4, to=S4s, inner_stream=70000, outer_stream=70000))
    add_broadcast('v4_encoding_0', 901, broadcast(4, S3, encoding=0))
    add_broadcast('v5_encoding_0', 901, broadcast(5, S4, encoding=0))
    add_broadcast('v4_signed_by_another_key', 916, broadcast(4, S3, signer=S2))
    c = broadcast(5, S4)
    add_broadcast('v5_message_bit_flipped', 916, broadcast(5, S4, spoil=c.at['message'][0] + 5))
    add_broadcast('v5_signature_bit_flipped', 916, broadcast(5, S4, spoil=-3))
    add_broadcast('v4_ntpb_varint_not_minimal', 'varint', broadcast(4, S3, raw_ntpb=b'\xfd\x00\x10'), bad_varint=b'\xfd\x00\x10')
    # Every strict prefix class of one plaintext: a cut inside and at the end of every field.  The fields of
    # this plaintext: version 0, stream 1, behaviour 2-6, keys 6-70-134, ntpb 134-137 (fd 03 e8), extra 137-140,
    # encoding 140, message length 141, message 142-172, signature length 172, signature from 173.  A varint that
    # is missing altogether reads as 0 (decodeVarint of nothing is (0, 0)); one cut inside raises.
    at = c.at
    assert [at[n] for n in ('version', 'stream', 'behaviour', 'key_s', 'key_e', 'ntpb', 'extra', 'encoding', 'mlen',
                            'message', 'siglen')] == [(0, 1), (1, 2), (2, 6), (6, 70), (70, 134), (134, 137), (137, 140),
                                                      (140, 141), (141, 142), (142, 172), (172, 173)]
    cuts = [(0, 838),      # sender version reads as 0
            (1, 848),      # sender stream reads as 0, the object says 1
            (2, 893), (4, 893), (6, 893), (38, 893), (70, 893), (102, 893),  # keys cut short: another ripe, another tag
            (134, 901),    # keys whole, tag right; both difficulty varints and the encoding read as 0
            (135, 'varint'), (137, 901), (138, 'varint'), (140, 901),
            (141, 916),    # encoding read; message and signature empty: verify says False
            (142, 916), (157, 916), (172, 916), (173, 916), (193, 916), (-1, 916)]
    for cut, line in cuts:
        c = broadcast(5, S4, cut=cut)
        if line == 893:
            assert ref_ripe(field(c, 'key_s'), field(c, 'key_e')) != S4.key.ripe
        add_broadcast('v5_plaintext_cut_at_%d' % cut if cut >= 0 else 'v5_plaintext_last_byte_cut', line, c,
                      parts=line == 916, bad_varint=c.full[134:137] if cut == 135 else c.full[137:140] if cut == 138 else None)

    # ------------------------------------------------------------------ encrypted (v4) pubkeys
    def pubkey(owner, to=None, version=4, stream=None, tag=None, signer=None, raw_ntpb=None, cut=None, spoil=None,
               version_bytes=None):
        to = to or owner
        head = be(rng.getrandbits(64), 8) + be(1760900000 + rng.randrange(1000), 8) + be(1, 4)
        head += (version_bytes or encodeVarint(version)) + encodeVarint(owner.stream if stream is None else stream)
        c_tag_at = len(head)
        head += to.lookup if tag is None else tag
        pieces = [('behaviour', be(1, 4)), ('key_s', owner.key.pub_s[1:]), ('key_e', owner.key.pub_e[1:]),
                  ('ntpb', raw_ntpb or encodeVarint(1000)), ('extra', encodeVarint(1000))]
        c = compose(head, pieces, signer or owner, to, cut, spoil)
        c.tag_at, c.version, c.stream = c_tag_at, version, owner.stream if stream is None else stream
        return c

    pubkeys_v4 = []

    def add_pubkey(name, line, c, address, asked=S4, decrypts=True, end=138, bad_varint=None):
        """line: where decryptAndCheckPubkeyPayload returns 'failed' (None: 'successful').  asked: the sender
        whose address this is, or comes closest to; decrypts: its key opens the object.  end: how far the
        plaintext's signed part reaches as the varints read (None: a varint of the object or the plaintext
        raises)."""
        payload = c.obj[len(c.head):]
        if bad_varint is not None:
            assert line == 'varint' and raises_varint(bad_varint), name
        assert opens(c.to, payload) == c.full and (opens(asked, payload) == c.full) == decrypts, name
        entry = {'name': name, 'line': line, 'obj': c.obj.hex(), 'address': address, 'plaintext': c.full.hex(),
                 'parts': None, 'storedData': None}
        if end is not None:
            key_s, key_e = field(c, 'key_s'), field(c, 'key_e')
            signed, stored = c.head[8:] + c.full[:end], c.head[20:c.tag_at] + c.full[:end]
            sig = field(c, 'sig')
            entry['parts'] = {'signedData': signed.hex(), 'signature': sig.hex(), 'pubSigningKey64': key_s.hex(),
                              'pubEncryptionKey64': key_e.hex(), 'storedData': stored.hex(), 'addressVersion': c.version,
                              'stream': c.stream, 'tag': c.head[c.tag_at:].hex()}
            valid = bool(highlevelcrypto.verify(signed, sig, hexlify(b'\x04' + key_s)))
            assert valid == (line in (None, 497, 423, 428, 442, 457)), name
            if line in (None, 497):
                assert (ref_ripe(key_s, key_e) == decodeAddress(address)[3]) == (line is None), name
            if line is None:
                entry['storedData'] = stored.hex()
        pubkeys_v4.append(entry)
        print('  pubkey    %-36s line=%s' % (name, line))

    add_pubkey('valid', None, pubkey(S4), S4.address)
    add_pubkey('valid_one_zero_byte', None, pubkey(S4z), S4z.address, asked=S4z)
    add_pubkey('valid_stream_70000', None, pubkey(S4s), S4s.address, asked=S4s)
    add_pubkey('address_version_3', 423, pubkey(S4), encodeAddress(3, 1, S4.key.ripe))
    add_pubkey('object_version_5', 423, pubkey(S4, version=5), S4.address)
    add_pubkey('address_stream_2', 428, pubkey(S4), encodeAddress(4, 2, S4.key.ripe))
    # no entry of neededPubkeys under the object's tag: the KeyError ends in `except Exception`
    add_pubkey('tag_of_another_address', 442, pubkey(S4, tag=U4.lookup), S4.address)
    bad = S4.address[:-1] + ('2' if S4.address[-1] != '2' else '3')
    assert decodeAddress(bad)[:2] == ('checksumfailed', 0)                               # version 0 against the object's 4
    add_pubkey('address_does_not_decode', 423, pubkey(S4), bad)
    add_pubkey('wrong_key', 457, pubkey(S4, to=U4, tag=S4.lookup), S4.address, decrypts=False)
    add_pubkey('signed_by_another_key', 484, pubkey(S4, signer=U4), S4.address)
    add_pubkey('signature_bit_flipped', 484, pubkey(S4, spoil=-2), S4.address)
    add_pubkey('keys_of_another_address', 497, pubkey(U4, to=S4), S4.address)
    add_pubkey('ntpb_varint_not_minimal', 'varint', pubkey(S4, raw_ntpb=b'\xfd\x00\x10'), S4.address, end=None,
               bad_varint=b'\xfd\x00\x10')
    add_pubkey('version_varint_not_minimal', 'varint', pubkey(S4, version_bytes=b'\xfd\x00\x04'), S4.address, end=None,
               bad_varint=b'\xfd\x00\x04')
    # Prefixes of one plaintext: behaviour 0-4, keys 4-68-132, ntpb 132-135 (fd 03 e8), extra 135-138, signature
    # length 138, signature from 139.  Missing varints read as 0, so the signed part ends at 132 until both are
    # there; the signature is then empty or short and verify says False.
    for cut, line, end in [(0, 484, 132), (3, 484, 132), (4, 484, 132), (36, 484, 132), (68, 484, 132), (100, 484, 132),
                           (132, 484, 132), (134, 'varint', None), (138, 484, 138), (139, 484, 138), (170, 484, 138)]:
        c = pubkey(S4, cut=cut)
        assert [c.at[n] for n in ('key_s', 'key_e', 'ntpb', 'extra', 'siglen')] == [(4, 68), (68, 132), (132, 135),
                                                                                  (135, 138), (138, 139)]
        add_pubkey('plaintext_cut_at_%d' % cut, line, c, S4.address, end=end,
                   bad_varint=c.full[132:135] if line == 'varint' else None)

    import ssl
    with open(os.path.join(HERE, 'ident_kats.json'), 'w') as f:
        json.dump({'source': 'reference addresses.encodeAddress / decodeAddress / encodeVarint / decodeVarint, '
                             'fallback.RIPEMD160Hash, highlevelcrypto.sign / encrypt / verify / pointMult / makeCryptor over '
                             + ssl.OPENSSL_VERSION,
                   'addresses': addresses, 'edge_addresses': edge_addresses, 'malformed': malformed, 'keys': key_rows, 'subscriptions': subscriptions,
                   'broadcasts': broadcasts, 'pubkeys_v4': pubkeys_v4}, f, indent=0, separators=(',', ':'))
    print('wrote ident_kats.json: %d addresses, %d keys, %d broadcasts, %d pubkeys' %
          (len(addresses), len(key_rows), len(broadcasts), len(pubkeys_v4)))


if __name__ == '__main__':
    main()
