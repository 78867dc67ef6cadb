#!/usr/bin/env python3
"""Generate tests/golden/tx_kats.json -- whole outgoing objects assembled with the REFERENCE's own primitives
(``addresses.encodeVarint``, ``highlevelcrypto.sign`` / ``encrypt`` / ``pointMult`` over OpenSSL; build
container only; needs /root/reference, read-only):

    BITMESSAGE_HOME=$(mktemp -d) PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_tx_golden.py

Each entry is one msg, broadcast or pubkey put together in the order ``class_singleWorker`` does it (sendMsg
:1136-1255, sendBroadcast :606-665, sendOutOrStoreMyV3Pubkey :343-373, sendOutOrStoreMyV4Pubkey :418-466):
head, body, ``sign(head + body)``, the length-prefixed signature, and for the encrypted kinds ``encrypt`` to
the recipient's key.  What the reference draws at random is recovered so that a test can replay it: the
ephemeral key through a recording ``ECC`` subclass (as make_send_golden.py), the IV from the blob's first 16
bytes, and the signature's nonce as ``k = s^-1 (e + r d) mod n``, checked by signing again with
``oracle/ecdsa_oracle.py``.  The reference's ``verify`` and ``decrypt`` are asserted on every entry.  The
keys and messages are seeded; OpenSSL's draws are not, so a re-run gives a different, equally valid file.
"""
import hashlib
import json
import os
import random
import subprocess
import sys
import tempfile
from binascii import hexlify
from struct import pack

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF_SRC = '/root/reference/src'
# RIPEMD-160 lives in OpenSSL 3's legacy provider: switch it on for a child of this script where it is off
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


def main():
    try:
        hashlib.new('ripemd160')
    except ValueError:
        with tempfile.NamedTemporaryFile('w', suffix='.cnf', delete=False) as f:
            f.write(CNF)
        sys.exit(subprocess.call([sys.executable] + sys.argv, env=dict(os.environ, OPENSSL_CONF=f.name)))
    sys.path.insert(0, ROOT)
    sys.path.insert(1, REF_SRC)
    from oracle import ecdsa_oracle as eo
    import highlevelcrypto
    import pyelliptic.ecc as eccmod
    from addresses import encodeVarint
    from fallback import RIPEMD160Hash
    from pyelliptic.openssl import OpenSSL

    rng = random.Random(20261020)
    N = eo.N
    RefECC = eccmod.ECC
    made = []

    class Recorder(RefECC):
        def __init__(self, *args, **kwargs):
            RefECC.__init__(self, *args, **kwargs)
            if not args and set(kwargs) <= {'curve'}:
                made.append(self.privkey)

    def rand(n):
        return bytes(rng.randrange(256) for _ in range(n))

    def be(v):
        return v.to_bytes(32, 'big')

    class Identity(object):
        def __init__(self, version, stream):
            self.version, self.stream = version, stream
            self.priv_s, self.priv_e = be(rng.randrange(1, N)), be(rng.randrange(1, N))
            self.pub_s, self.pub_e = highlevelcrypto.pointMult(self.priv_s), highlevelcrypto.pointMult(self.priv_e)
            self.ripe = RIPEMD160Hash(hashlib.sha512(self.pub_s + self.pub_e).digest()).digest()
            data = encodeVarint(version) + encodeVarint(stream) + self.ripe
            single, double = hashlib.sha512(data).digest(), hashlib.sha512(hashlib.sha512(data).digest()).digest()
            self.address_priv = single[:32] if version <= 3 else double[:32]  # :655-661, :463
            self.tag = double[32:]

    def sign(data, priv, alg):
        if alg == 'sha256':
            sig = highlevelcrypto.sign(data, hexlify(priv))  # the default digestalg
        else:
            sig = highlevelcrypto.makeCryptor(hexlify(priv)).sign(data, digest_alg=OpenSSL.digest_ecdsa_sha1)
        d = int.from_bytes(priv, 'big')
        e = int.from_bytes(hashlib.new(alg, data).digest(), 'big')
        r, s = eo.der_decode(sig)
        k = pow(s, -1, N) * (e + r * d) % N
        assert eo.sign(d, k, e) == (r, s) and eo.der_encode(r, s) == sig
        assert highlevelcrypto.verify(data, sig, hexlify(b'\x04' + eo.xy_key(eo.mult_g(d))))
        return sig, k

    def encrypt(plain, recipient_priv):
        pub = highlevelcrypto.pointMult(recipient_priv)
        del made[:]
        eccmod.ECC = Recorder
        try:
            blob = highlevelcrypto.encrypt(plain, hexlify(pub))
        finally:
            eccmod.ECC = RefECC
        assert len(made) == 1 and highlevelcrypto.decrypt(blob, hexlify(recipient_priv)) == plain
        return blob, made[0].rjust(32, b'\x00'), pub[1:]

    entries = []

    def add(name, kind, alg, fields, head, body, priv, recipient_priv=None):
        sig, k = sign(head + body, priv, alg)
        plain = body + encodeVarint(len(sig)) + sig
        entry = {'name': name, 'kind': kind, 'digest': alg, 'fields': fields, 'head': head.hex(), 'body': body.hex(),
                 'priv': priv.hex(), 'nonce': be(k).hex(), 'signature': sig.hex()}
        if kind == 'sealed':
            blob, eph, pub = encrypt(plain, recipient_priv)
            payload = head + blob
            entry.update(recipient_priv=recipient_priv.hex(), recipient_pub=pub.hex(), ephemeral=eph.hex(), iv=blob[:16].hex())
        else:
            payload = head + plain
        assert 12 <= len(head) <= 62 and len(body) < 1000
        entry.update(payload=payload.hex(), initial_hash=hashlib.sha512(payload).hexdigest())
        entries.append(entry)

    def common(kind, who, t, **more):
        f = {'type': kind, 'embeddedTime': t, 'version': who.version, 'stream': who.stream, 'bitfield': '00000001',
             'pubSigningKey': who.pub_s.hex(), 'pubEncryptionKey': who.pub_e.hex(), 'ripe': who.ripe.hex(),
             'ntpb': 1000, 'extra': 1000}
        f.update(more)
        return f

    def keys_and_difficulty(who, f):
        out = who.pub_s[1:] + who.pub_e[1:]
        if who.version >= 3:
            out += encodeVarint(f['ntpb']) + encodeVarint(f['extra'])
        return out

    def msg(name, who, to, alg='sha256', message=b'hello', ack=b'', ntpb=1000, extra=1000):
        t = 1790000000 + rng.randrange(10 ** 6)
        f = common('msg', who, t, toStream=to.stream, toRipe=to.ripe.hex(), encoding=2, message=message.hex(),
                   fullAckPayload=ack.hex(), ntpb=ntpb, extra=extra)
        head = pack('>Q', t) + b'\x00\x00\x00\x02' + encodeVarint(1) + encodeVarint(to.stream)  # :1224, :1252-1254
        body = encodeVarint(who.version) + encodeVarint(who.stream) + bytes.fromhex(f['bitfield'])  # :1136-1223
        body += keys_and_difficulty(who, f) + to.ripe + encodeVarint(2) + encodeVarint(len(message)) + message
        body += encodeVarint(len(ack)) + ack
        add(name, 'sealed', alg, f, head, body, who.priv_s, to.priv_e)

    def broadcast(name, who, alg='sha256', message=b'Subject:s\nBody:b'):
        t = 1790000000 + rng.randrange(10 ** 6)
        f = common('broadcast', who, t, encoding=2, message=message.hex())
        head = pack('>Q', t) + b'\x00\x00\x00\x03' + encodeVarint(4 if who.version <= 3 else 5) + encodeVarint(who.stream)
        if who.version >= 4:
            head += who.tag
        body = encodeVarint(who.version) + encodeVarint(who.stream) + bytes.fromhex(f['bitfield'])  # :625-640
        body += keys_and_difficulty(who, f) + encodeVarint(2) + encodeVarint(len(message)) + message
        add(name, 'sealed', alg, f, head, body, who.priv_s, who.address_priv)

    def pubkey(name, who, alg='sha256'):
        t = 1790000000 + rng.randrange(10 ** 6)
        f = common('pubkey', who, t)
        head = pack('>Q', t) + b'\x00\x00\x00\x01' + encodeVarint(who.version) + encodeVarint(who.stream)
        body = bytes.fromhex(f['bitfield']) + who.pub_s[1:] + who.pub_e[1:] + encodeVarint(1000) + encodeVarint(1000)
        if who.version >= 4:
            add(name, 'sealed', alg, f, head + who.tag, body, who.priv_s, who.address_priv)  # :418-466
        else:
            add(name, 'clear', alg, f, head, body, who.priv_s)  # :343-373

    v2, v3, v4 = Identity(2, 1), Identity(3, 1), Identity(4, 1)
    far3, far5, far9 = Identity(4, 300), Identity(4, 70000), Identity(3, 2 ** 32 + 5)  # varints of 3, 5 and 9 bytes
    msg('msg_from_v2', v2, v4)
    msg('msg_from_v3', v3, v4, message=rand(100), ack=rand(60))
    msg('msg_from_v4', v4, v3, message=rand(333), ack=rand(176))
    msg('msg_empty_message', v4, v3, message=b'')
    msg('msg_no_ack', v4, v2, message=rand(57))
    msg('msg_sha1', v3, v4, alg='sha1', message=rand(41), ack=rand(60))
    msg('msg_stream_3_bytes', far3, far3, message=rand(20))
    msg('msg_stream_5_bytes', far5, far5, message=rand(21), ack=rand(33))
    msg('msg_stream_9_bytes', far9, far9, message=rand(22))
    msg('msg_own_difficulty', v4, far3, message=rand(64), ntpb=70000, extra=2 ** 32 + 1)
    broadcast('broadcast_v4_from_v2', v2)
    broadcast('broadcast_v4_from_v3', v3, message=rand(200))
    broadcast('broadcast_v5', v4, message=rand(90))
    broadcast('broadcast_v5_sha1', v4, alg='sha1', message=b'')
    broadcast('broadcast_v5_stream_5_bytes', far5, message=rand(15))
    broadcast('broadcast_v4_stream_9_bytes', far9, message=rand(16))
    pubkey('pubkey_v3', v3)
    pubkey('pubkey_v3_sha1', v3, alg='sha1')
    pubkey('pubkey_v3_stream_9_bytes', far9)
    pubkey('pubkey_v4', v4)
    pubkey('pubkey_v4_sha1', v4, alg='sha1')
    pubkey('pubkey_v4_stream_3_bytes', far3)

    import ssl
    with open(os.path.join(HERE, 'tx_kats.json'), 'w') as f:
        json.dump({'source': 'reference highlevelcrypto.sign / encrypt / pointMult, addresses.encodeVarint over '
                             + ssl.OPENSSL_VERSION, 'objects': entries}, f, indent=1)
    print('wrote tx_kats.json: %d objects' % len(entries))


if __name__ == '__main__':
    main()
