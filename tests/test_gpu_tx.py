"""Outgoing objects built on the GPU in one call (``bmpow_tx_objects``, ``pybitmessage_amd.outgoing``,
``worker.send_msgs_built`` / ``send_broadcasts`` / ``send_pubkeys``) against the reference-made fixture
``tests/golden/tx_kats.json`` (tests/golden/make_tx_golden.py), against the composition of the calls that
were there before (``sender.sign_batch``, ``sender.encrypt_batch``, ``hashlib.sha512``) under the same
nonces, ephemeral keys and IVs, and against the project's own receive path (``ecies.decrypt_batch``,
``receive.open_msgs`` / ``open_broadcasts`` / ``open_pubkeys``), which ``rx_kats.json`` and
``rxobj_kats.json`` pin to the reference."""
import hashlib
import random

import numpy as np
import pytest

from oracle import ecdsa_oracle as eo
from pybitmessage_amd import _lib, addresses, ecies, intake, outgoing, receive, sender, signatures, targets, worker
from pybitmessage_amd.worker import _varint

pytestmark = pytest.mark.gpu

P, N = eo.P, eo.N
SEALED, CLEAR = outgoing.SEALED, outgoing.CLEAR


def b32(v):
    return v.to_bytes(32, 'big')


def pub64(k):
    return eo.xy_key(eo.mult_g(k))


class Identity(object):
    """An address of the given version and stream with seeded keys."""

    def __init__(self, rng, version, stream=1):
        self.version, self.stream = version, stream
        self.ks, self.ke = rng.randrange(1, N), rng.randrange(1, N)
        self.priv_s, self.priv_e = b32(self.ks), b32(self.ke)
        self.pub_s, self.pub_e = b'\x04' + pub64(self.ks), b'\x04' + pub64(self.ke)
        ident = addresses.derive_batch([self.pub_s], [self.pub_e], [version], [stream])
        self.ripe, self.address, self.tag = ident.ripe[0].tobytes(), ident.address(0), ident.tag[0].tobytes()


@pytest.fixture(scope='module')
def kats(golden):
    return golden('tx_kats.json')['objects']


@pytest.fixture(scope='module')
def send_kats(golden):
    return golden('send_kats.json')


@pytest.fixture(scope='module')
def people(gpulib):
    rng = random.Random(20261020)
    return {'v2': Identity(rng, 2), 'v3': Identity(rng, 3), 'v4': Identity(rng, 4), 'far': Identity(rng, 4, 70000)}


def compose(kinds, heads, bodies, privs, pubs, alg, nonces, ephemeral, ivs):
    """What the separate calls give: per row (payload or None, signature, hashlib's initialHash or None)."""
    sigs = sender.sign_batch([h + b for h, b in zip(heads, bodies)], privs, alg, nonces)
    tails = [_varint(len(s)) + s for s in sigs]
    sealed = [i for i, k in enumerate(kinds) if k == SEALED]
    blobs = dict(zip(sealed, sender.encrypt_batch([bodies[i] + tails[i] for i in sealed], [pubs[i] for i in sealed],
                                                  [ephemeral[i] for i in sealed], [ivs[i] for i in sealed])))
    out = []
    for i, kind in enumerate(kinds):
        rest = blobs[i] if kind == SEALED else bodies[i] + tails[i]
        payload = None if rest is None else heads[i] + rest
        out.append((payload, sigs[i], None if payload is None else hashlib.sha512(payload).digest()))
    return out


# ------------------------------------------------------------------ the reference's own objects
def test_reference_fixture_bit_for_bit(gpulib, kats):
    for alg in ('sha1', 'sha256'):
        rows = [k for k in kats if k['digest'] == alg]
        assert rows
        built = outgoing.build_objects(
            [SEALED if k['kind'] == 'sealed' else CLEAR for k in rows], [bytes.fromhex(k['head']) for k in rows],
            [bytes.fromhex(k['body']) for k in rows], [bytes.fromhex(k['priv']) for k in rows],
            [bytes.fromhex(k['recipient_pub']) if k['kind'] == 'sealed' else None for k in rows], alg,
            nonces=[bytes.fromhex(k['nonce']) for k in rows],
            ephemeral=[bytes.fromhex(k['ephemeral']) if k['kind'] == 'sealed' else None for k in rows],
            ivs=[bytes.fromhex(k['iv']) if k['kind'] == 'sealed' else None for k in rows])
        assert built.accepted() == list(range(len(rows)))
        for i, k in enumerate(rows):
            assert built.payload(i).hex() == k['payload'], k['name']
            assert built.initial_hash(i).hex() == k['initial_hash'], k['name']
            assert built.signature(i).hex() == k['signature'], k['name']
            assert built.recs[i]['digest'] == sender.DIGESTS[alg] and built.recs[i]['kind'] == (k['kind'] != 'sealed')
            assert built.obj_len[i] == len(k['payload']) // 2
            assert built.plain_len[i] == len(k['body']) // 2 + 1 + len(k['signature']) // 2


def test_field_builders_reproduce_the_fixture(gpulib, kats):
    """The same entries from their fields: the recipient key of a broadcast or a v4 pubkey is derived here."""
    for alg in ('sha1', 'sha256'):
        for kind, make, build in (('msg', _msg_fields, outgoing.build_msgs), ('broadcast', _broadcast_fields, outgoing.build_broadcasts),
                                  ('pubkey', _pubkey_fields, outgoing.build_pubkeys)):
            rows = [k for k in kats if k['digest'] == alg and k['fields']['type'] == kind]
            if not rows:
                continue
            built = build([make(k) for k in rows], alg, nonces=[bytes.fromhex(k['nonce']) for k in rows],
                          ephemeral=[bytes.fromhex(k.get('ephemeral', '01')) for k in rows],
                          ivs=[bytes.fromhex(k.get('iv', '00' * 16)) for k in rows])
            for i, k in enumerate(rows):
                assert built.status[i] == outgoing.OK, k['name']
                assert built.payload(i).hex() == k['payload'], k['name']
                assert built.initial_hash(i).hex() == k['initial_hash'], k['name']


def _hexes(f, *names):
    return [bytes.fromhex(f[n]) for n in names]


def _msg_fields(k):
    f = k['fields']
    bitfield, ps, pe, to_ripe, message, ack = _hexes(f, 'bitfield', 'pubSigningKey', 'pubEncryptionKey', 'toRipe', 'message',
                                                     'fullAckPayload')
    return outgoing.MsgFields(f['embeddedTime'], f['toStream'], f['version'], f['stream'], bitfield, ps, pe, to_ripe,
                              f['encoding'], message, ack, f['ntpb'], f['extra'], bytes.fromhex(k['priv']),
                              bytes.fromhex(k['recipient_pub']))


def _broadcast_fields(k):
    f = k['fields']
    bitfield, ps, pe, ripe, message = _hexes(f, 'bitfield', 'pubSigningKey', 'pubEncryptionKey', 'ripe', 'message')
    return outgoing.BroadcastFields(f['embeddedTime'], f['version'], f['stream'], ripe, bitfield, ps, pe, f['encoding'], message,
                                    f['ntpb'], f['extra'], bytes.fromhex(k['priv']))


def _pubkey_fields(k):
    f = k['fields']
    bitfield, ps, pe, ripe = _hexes(f, 'bitfield', 'pubSigningKey', 'pubEncryptionKey', 'ripe')
    return outgoing.PubkeyFields(f['embeddedTime'], f['version'], f['stream'], ripe, bitfield, ps, pe, f['ntpb'], f['extra'],
                                 bytes.fromhex(k['priv']))


# ------------------------------------------------------------------ against the separate calls
def _mixed_rows(send_kats):
    """A few hundred rows of all four object kinds with fixed random inputs.  Head lengths 14, 16, 18, 22 (msgs
    and v3 pubkeys over streams of 1, 3, 5 and 9 bytes), 46 (broadcast v5, v4 pubkey) and 62; under the
    14-byte head every body length 0 .. 140, so every residue of the signed length mod 64 and of the
    plaintext length mod 16 occurs whatever the signatures' lengths."""
    rng = random.Random(7)
    tag = bytes(rng.randrange(256) for _ in range(32))
    t = 1790000000
    heads = {14: outgoing.msg_head(t, 1), 16: outgoing.msg_head(t, 300), 18: outgoing.msg_head(t, 70000),
             22: outgoing.pubkey_head(t, 3, 2 ** 32 + 5), 46: outgoing.broadcast_head(t, 4, 1, tag),
             62: outgoing.pubkey_head(t, 2 ** 32 + 1, 2 ** 32 + 5, tag)}
    assert {len(h) for h in heads.values()} == set(heads)
    keys = [rng.randrange(1, N) for _ in range(4)]
    recips = [rng.randrange(1, N) for _ in range(3)]
    rpubs = [pub64(k) for k in recips]
    rows = []

    def add(kind, head_len, body_len, nonce=None, eph=None):
        rows.append({'kind': kind, 'head': heads[head_len], 'body': bytes(rng.randrange(256) for _ in range(body_len)),
                     'priv': b32(keys[len(rows) % 4]), 'pub': rpubs[len(rows) % 3], 'recip': recips[len(rows) % 3],
                     'nonce': nonce or b32(rng.randrange(1, N)), 'eph': eph or b32(rng.randrange(1, N)),
                     'iv': bytes(rng.randrange(256) for _ in range(16))})

    for body_len in range(141):
        add(SEALED, 14, body_len)
    for head_len in (16, 18, 46, 62):
        for _ in range(30):
            add(SEALED, head_len, rng.randrange(301))
    for head_len in (14, 22):  # v3 pubkeys
        for body_len in list(range(40)) + [rng.randrange(301) for _ in range(10)]:
            add(CLEAR, head_len, body_len)
    short_r = [bytes.fromhex(s['nonce']) for s in send_kats['sign_kats'] if 'short_r' in s['name']]
    short_xy = [bytes.fromhex(e['ephemeral']) for e in send_kats['encrypt_kats'] if e['coord_lens'] != [32, 32]]
    assert len(short_r) >= 2 and len(short_xy) >= 2
    for j, k in enumerate(short_r):
        add(SEALED if j % 2 else CLEAR, 14, 50 + j, nonce=k)
    for e in short_xy:
        add(SEALED, 46, 77, eph=e)
    return rows, len(short_r), len(short_xy)


@pytest.mark.parametrize('alg', ['sha1', 'sha256'])
def test_mixed_kinds_equal_the_composition(gpulib, send_kats, alg):
    rows, n_short_r, n_short_xy = _mixed_rows(send_kats)
    cols = [[r[c] for r in rows] for c in ('kind', 'head', 'body', 'priv', 'pub')]
    rand = [[r[c] for r in rows] for c in ('nonce', 'eph', 'iv')]
    want = compose(*cols, alg, *rand)
    built = outgoing.build_objects(*cols, alg, *rand)
    assert built.accepted() == list(range(len(rows)))
    signed_mod, plain_mod, sig_lens = set(), set(), set()
    for i, (r, (payload, sig, ih)) in enumerate(zip(rows, want)):
        assert payload is not None and built.payload(i) == payload, i
        assert built.signature(i) == sig and built.initial_hash(i) == ih, i
        assert built.plain_len[i] == len(r['body']) + 1 + len(sig) and built.obj_len[i] == len(payload)
        signed_mod.add((len(r['head']) + len(r['body'])) % 64)
        plain_mod.add(int(built.plain_len[i]) % 16)
        sig_lens.add(len(sig))
    assert signed_mod >= {55, 56, 63, 64 % 64, 0} and plain_mod >= {15, 0, 1}
    assert sig_lens >= {70, 71, 72}
    assert any(len(r['body']) == 0 for r in rows)
    n = len(rows)
    for i in range(n - n_short_xy - n_short_r, n - n_short_xy):  # r below 2^248: leading zero bytes DER must drop
        sig = built.signature(i)
        assert int.from_bytes(sig[4:4 + sig[3]], 'big') < 2 ** 248 and sig[3] <= 32 and len(sig) <= 71
    for i in range(n - n_short_xy, n):  # an ephemeral point with a 31-byte coordinate
        blob = built.payload(i)[46:]
        xl = int.from_bytes(blob[18:20], 'big')
        yl = int.from_bytes(blob[20 + xl:22 + xl], 'big')
        assert (xl, yl) != (32, 32)


# ------------------------------------------------------------------ through the receive path
def _sig_hash(sig):
    return hashlib.sha512(hashlib.sha512(sig).digest()).digest()[32:]


def _open_msg_rows(built, heads, recips):
    """Decrypt each built msg with its recipient's key and open it: (OpenedMsgs, plaintexts)."""
    plains = []
    for i, (head, who) in enumerate(zip(heads, recips)):
        got = ecies.decrypt_batch([built.payload(i)[len(head):]], [who.priv_e])[0]
        assert got is not None and got[0] == 0
        plains.append(got[1])
    objs = [bytes(8) + built.payload(i) for i in range(len(heads))]
    return receive.open_msgs(objs, plains, [who.ripe for who in recips]), plains


def test_built_msgs_open_on_the_receive_path(gpulib, people):
    rng = random.Random(11)
    rows, recips = [], []
    for sender_name, to_name, message, ack in (('v2', 'v4', b'from a v2 address', b''), ('v3', 'v4', b'', bytes(range(60))),
                                               ('v4', 'v3', bytes(rng.randrange(256) for _ in range(300)), bytes(176)),
                                               ('far', 'far', b'streams of five bytes', b'')):
        me, to = people[sender_name], people[to_name]
        rows.append(outgoing.MsgFields(1790000000, to.stream, me.version, me.stream, worker.get_bitfield(), me.pub_s, me.pub_e,
                                       to.ripe, 2, message, ack, 1000, 1000, me.priv_s, to.pub_e))
        recips.append((me, to, message, ack))
    for alg in ('sha256', 'sha1'):
        built = outgoing.build_msgs(rows, alg)
        assert built.accepted() == list(range(len(rows)))
        heads = [outgoing.msg_head(m.embeddedTime, m.toStream) for m in rows]
        opened, _ = _open_msg_rows(built, heads, [r[1] for r in recips])
        assert list(opened.status) == [receive.OK] * len(rows)
        for i, (me, _to, message, ack) in enumerate(recips):
            assert opened.fromAddress(i) == me.address and opened.message(i) == message and opened.ackData(i) == ack
            assert opened.signature(i) == built.signature(i) and opened.sigHash(i) == _sig_hash(built.signature(i))
            assert opened.digest[i] == sender.DIGESTS[alg]
            assert built.initial_hash(i) == hashlib.sha512(built.payload(i)).digest()


def test_built_broadcasts_and_pubkeys_open_on_the_receive_path(gpulib, people):
    who = [people['v3'], people['v4'], people['far'], people['v2']]
    bcs = [outgoing.BroadcastFields(1790000000, p.version, p.stream, p.ripe, worker.get_bitfield(), p.pub_s, p.pub_e, 2,
                                    b'Subject:s\nBody:' + p.address.encode(), 1000, 1000, p.priv_s) for p in who]
    built = outgoing.build_broadcasts(bcs)
    assert built.accepted() == list(range(len(bcs)))
    objs = [bytes(8) + built.payload(i) for i in range(len(bcs))]
    opened = receive.open_broadcasts(objs, [p.address for p in who])
    assert list(opened.status) == [receive.OBJ_OK] * len(bcs)
    for i, p in enumerate(who):
        assert opened.fromAddress(i) == p.address and opened.message(i) == bcs[i].message
        assert opened.sigHash(i) == _sig_hash(built.signature(i)) and opened.signature(i) == built.signature(i)
        assert built.initial_hash(i) == hashlib.sha512(built.payload(i)).digest()
    who = [people['v3'], people['v4'], people['far']]
    pks = [outgoing.PubkeyFields(1790000000, p.version, p.stream, p.ripe, worker.get_bitfield(), p.pub_s, p.pub_e, 1000, 1000,
                                 p.priv_s) for p in who]
    built = outgoing.build_pubkeys(pks)
    assert built.accepted() == list(range(len(pks)))
    assert list(built.kind) == [CLEAR, SEALED, SEALED]
    objs = [bytes(8) + built.payload(i) for i in range(len(pks))]
    opened = receive.open_pubkeys(objs, {p.tag: p.address for p in who if p.version >= 4})
    assert list(opened.status) == [receive.OBJ_OK] * len(pks)
    for i, p in enumerate(who):
        assert opened.fromAddress(i) == p.address and opened.ripe(i) == p.ripe
        assert built.initial_hash(i) == hashlib.sha512(built.payload(i)).digest()


# ------------------------------------------------------------------ statuses
def test_bad_recipients_among_good_rows(gpulib, people):
    me, to = people['v4'], people['v3']
    x, y = eo.key_xy(to.pub_e[1:])
    pubs = [to.pub_e, b32(x) + b32((y + 1) % P), b32(P) + b32(y), b32(x) + b32(P + 1), to.pub_e[1:], to.pub_e[1:-1], None]
    n = len(pubs)
    rng = random.Random(5)
    heads = [outgoing.msg_head(1790000000, 1)] * n
    bodies = [bytes(rng.randrange(256) for _ in range(100 + i)) for i in range(n)]
    rand = [[b32(rng.randrange(1, N)) for _ in range(n)], [b32(rng.randrange(1, N)) for _ in range(n)],
            [bytes(rng.randrange(256) for _ in range(16)) for _ in range(n)]]
    built = outgoing.build_objects([SEALED] * n, heads, bodies, [me.priv_s] * n, pubs, 'sha256', *rand)
    assert list(built.status) == [outgoing.OK, outgoing.BAD_RECIPIENT, outgoing.BAD_RECIPIENT, outgoing.BAD_RECIPIENT,
                                  outgoing.OK, outgoing.BAD_RECIPIENT, outgoing.BAD_RECIPIENT]
    good = [0, 4]
    want = compose([SEALED] * 2, [heads[i] for i in good], [bodies[i] for i in good], [me.priv_s] * 2, [pubs[i] for i in good],
                   'sha256', *[[col[i] for i in good] for col in rand])
    for i, (payload, sig, ih) in zip(good, want):
        assert built.payload(i) == payload and built.signature(i) == sig and built.initial_hash(i) == ih
    for i in (1, 2, 3, 5, 6):
        assert built.payload(i) is None and built.initial_hash(i) is None and built.obj_len[i] == 0


def test_object_size_limit(gpulib, people, send_kats):
    me, to = people['v4'], people['v3']
    eph = next(bytes.fromhex(e['ephemeral']) for e in send_kats['encrypt_kats'] if e['coord_lens'] == [32, 32])
    head = outgoing.msg_head(1790000000, 70000)
    assert len(head) == 18
    # 8 + 18 + 118 + 16 m = 2^18 with m = 16375 blocks: a plaintext of 261,984 .. 261,999 bytes, which a body of
    # 261,913 gives under a signature of 70, 71 or 72 bytes
    body = bytes(261913)
    rng = random.Random(3)
    rand = [[b32(rng.randrange(1, N))] * 2, [eph] * 2, [bytes(16)] * 2]
    built = outgoing.build_objects([SEALED] * 2, [head] * 2, [body, body + bytes(16)], [me.priv_s] * 2, [to.pub_e] * 2,
                                   'sha256', *rand)
    assert 70 <= built.recs[0]['sig_len'] <= 72
    assert list(built.status) == [outgoing.OK, outgoing.TOO_LARGE]
    assert built.obj_len[0] == 2 ** 18 - 8 and built.obj_len[1] == 2 ** 18 - 8 + 16
    payload = built.payload(0)
    assert len(payload) == 2 ** 18 - 8 and built.initial_hash(0) == hashlib.sha512(payload).digest()
    want = compose([SEALED], [head], [body], [me.priv_s], [to.pub_e], 'sha256', *[col[:1] for col in rand])[0]
    assert payload == want[0]
    assert built.payload(1) is None
    # a body no object can hold never reaches the device
    outgoing.reset_stats()
    before = outgoing.stats()
    built = outgoing.build_objects([SEALED, CLEAR], [head] * 2, [bytes(2 ** 18 + 1)] * 2, [me.priv_s] * 2, [to.pub_e, None])
    assert list(built.status) == [outgoing.TOO_LARGE] * 2
    after = outgoing.stats()
    assert after['launches'] == before['launches'] == 0 and after['sets'] == 0 and after['rows'] == 0


def test_out_of_range_scalars_raise(gpulib, people):
    me, to = people['v4'], people['v3']
    head = outgoing.msg_head(1790000000, 1)

    def call(priv=me.priv_s, nonce=None, eph=None):
        return outgoing.build_objects([SEALED], [head], [b'body'], [priv], [to.pub_e], 'sha256',
                                      None if nonce is None else [nonce], None if eph is None else [eph])

    for bad in (dict(priv=bytes(32)), dict(priv=b32(N)), dict(nonce=bytes(32)), dict(nonce=b32(N)), dict(eph=bytes(32)),
                dict(eph=b32(N))):
        with pytest.raises(_lib.BmpowError) as e:
            call(**bad)
        assert e.value.code == _lib.E_ARG
    assert call().accepted() == [0]


def test_abort_is_honoured(gpulib, people):
    me, to = people['v4'], people['v3']
    args = ([SEALED], [outgoing.msg_head(1790000000, 1)], [b'body'], [me.priv_s], [to.pub_e])
    gpulib.bmpow_abort()
    try:
        with pytest.raises(_lib.BmpowError) as e:
            outgoing.build_objects(*args)
        assert e.value.code == _lib.E_ABORTED
    finally:
        gpulib.bmpow_clear_abort()
    assert outgoing.build_objects(*args).accepted() == [0]


# ------------------------------------------------------------------ more than one set
def test_two_sets(gpulib, people):
    me, to = people['v4'], people['v3']
    n = 2 ** 18 + 1
    head = outgoing.msg_head(1790000000, 1)
    body = worker.msg_plaintext(me.version, me.stream, worker.get_bitfield(), me.pub_s, me.pub_e, to.ripe, 2, b'', b'', 1000,
                                1000)
    gen = np.random.default_rng(20261020)
    scalars = gen.integers(0, 256, size=(2, n, 32), dtype=np.uint8)
    scalars[:, :, 0] = 0  # below the group order
    scalars[:, :, 31] |= 1  # and not zero
    nonces = [scalars[0, i].tobytes() for i in range(n)]
    ephs = [scalars[1, i].tobytes() for i in range(n)]
    ivs = [v.tobytes() for v in gen.integers(0, 256, size=(n, 16), dtype=np.uint8)]
    outgoing.reset_stats()
    built = outgoing.build_objects([SEALED] * n, [head] * n, [body] * n, [me.priv_s] * n, [to.pub_e] * n, 'sha256', nonces, ephs,
                                   ivs)
    st = outgoing.stats()
    assert st['sets'] == 2 and st['rows'] == n and st['calls'] == 1 and st['launches'] == 22
    assert int((built.status == outgoing.OK).sum()) == n
    payloads = [built.payload(i) for i in range(n)]
    hashes = built.recs['initial_hash']
    for i, p in enumerate(payloads):
        assert hashes[i].tobytes() == hashlib.sha512(p).digest(), i
    pick = sorted({0, 1, 2 ** 18 - 1, 2 ** 18, n - 1} | set(random.Random(1).sample(range(n), 256)))
    want = compose([SEALED] * len(pick), [head] * len(pick), [body] * len(pick), [me.priv_s] * len(pick), [to.pub_e] * len(pick),
                   'sha256', [nonces[i] for i in pick], [ephs[i] for i in pick], [ivs[i] for i in pick])
    for i, (payload, sig, _ih) in zip(pick, want):
        assert payloads[i] == payload and built.signature(i) == sig, i


# ------------------------------------------------------------------ drawn randomness
def test_drawn_randomness(gpulib, people):
    me, to = people['v4'], people['v3']
    n = 6
    kinds = [SEALED, CLEAR] * 3
    heads = [outgoing.msg_head(1790000000, 1) if k == SEALED else outgoing.pubkey_head(1790000000, 3, 1) for k in kinds]
    bodies = [b'drawn %d' % i * 20 for i in range(n)]
    runs = [outgoing.build_objects(kinds, heads, bodies, [me.priv_s] * n, [to.pub_e] * n) for _ in range(2)]
    for built in runs:
        assert built.accepted() == list(range(n))
        sigs = [built.signature(i) for i in range(n)]
        assert signatures.verify_batch([h + b for h, b in zip(heads, bodies)], sigs, [me.pub_s] * n) == [True] * n
        for i in range(n):
            rest = built.payload(i)[len(heads[i]):]
            assert built.payload(i)[:len(heads[i])] == heads[i]
            if kinds[i] == SEALED:
                got = ecies.decrypt_batch([rest], [to.priv_e])[0]
                assert got is not None
                rest = got[1]
            assert rest == bodies[i] + _varint(len(sigs[i])) + sigs[i]
            assert built.initial_hash(i) == hashlib.sha512(built.payload(i)).digest()
    assert all(runs[0].payload(i) != runs[1].payload(i) for i in range(n))
    assert all(runs[0].signature(i) != runs[1].signature(i) for i in range(n))


# ------------------------------------------------------------------ the worker
def test_send_msgs_built_through_the_receive_path(gpulib, people):
    me, a, b = people['v4'], people['v3'], people['v2']
    now = 1760000000
    x, y = eo.key_xy(a.pub_e[1:])
    seen = {}

    def build_plain(ctx, ack):
        seen[ctx['name']] = ack
        plain = worker.msg_plaintext(me.version, me.stream, worker.get_bitfield(), me.pub_s, me.pub_e, ctx['to'].ripe, 2,
                                     b'Subject:hello\nBody:' + ctx['name'].encode() * 20, ack, 10, 10)
        return plain, me.priv_s, ctx['key'], ctx['to'].version, 1, 4 * 24 * 3600, 10, 10

    rng = random.Random(83)
    ackdata = [b'\x00\x00\x00\x02\x01\x01' + bytes(rng.randrange(256) for _ in range(32)) for _ in range(2)]
    jobs = [(ackdata[0], 4 * 24 * 3600, {'name': 'to_a', 'to': a, 'key': a.pub_e}),
            (None, 4 * 24 * 3600, {'name': 'to_b_no_ack', 'to': b, 'key': b.pub_e[1:]}),
            (ackdata[1], 4 * 24 * 3600, {'name': 'bad_key', 'to': a, 'key': b32(x) + b32((y + 1) % P)})]
    out = worker.send_msgs_built(jobs, build_plain, rng=random.Random(84), now=now)
    assert out[2] is None and out[0] is not None and out[1] is not None
    assert seen['to_b_no_ack'] == b'' and len(seen['to_a']) > 24
    objs = out[:2]
    # the recipients ask for the test-mode difficulty (10, 10); the sender works to the network minimum, which is
    # what every receiver holds an object to whatever lower demand it is given
    for o in objs:
        assert targets.isProofOfWorkSufficient(o, 10, 10, recvTime=now)
    res = intake.check_objects(objs, streams=(1,), nonceTrialsPerByte=10, payloadLengthExtraBytes=10, now=now)
    assert list(res.status) == [intake.OK, intake.OK] and list(res.objectType) == [worker.OBJECT_MSG] * 2
    got = receive.process_msgs(objs, {a.ripe: a.priv_e, b.ripe: b.priv_e})
    for m, name, to in zip(got, ('to_a', 'to_b_no_ack'), (a, b)):
        assert m is not None and m.fromAddress == me.address and m.toRipe == to.ripe
        assert m.message == b'Subject:hello\nBody:' + name.encode() * 20 and m.ackData == seen[name]
        assert m.digest == signatures.SHA256
    ack = seen['to_a']
    assert ack[:4] == b'\xe9\xbe\xb4\xd9' and ack[24 + 8 + 8:] == ackdata[0]


def test_send_broadcasts_and_pubkeys(gpulib, people):
    now = 1760000000
    who = [people['v3'], people['v4']]
    jobs = [(outgoing.BroadcastFields(None, p.version, p.stream, p.ripe, worker.get_bitfield(), p.pub_s, p.pub_e, 2,
                                      b'Subject:s\nBody:' + p.address.encode(), None, None, p.priv_s), 2 * 24 * 3600) for p in who]
    objs = worker.send_broadcasts(jobs, rng=random.Random(1), now=now)
    assert all(o is not None for o in objs)
    for o in objs:
        assert targets.isProofOfWorkSufficient(o, recvTime=now)
    res = intake.check_objects(objs, streams=(1,), now=now)
    assert list(res.status) == [intake.OK] * 2 and list(res.objectType) == [worker.OBJECT_BROADCAST] * 2
    opened = receive.open_broadcasts(objs, [p.address for p in who])
    assert list(opened.status) == [receive.OBJ_OK] * 2
    for i, p in enumerate(who):
        assert opened.fromAddress(i) == p.address and opened.message(i) == b'Subject:s\nBody:' + p.address.encode()
    jobs = [outgoing.PubkeyFields(None, p.version, p.stream, p.ripe, worker.get_bitfield(), p.pub_s, p.pub_e, None, None,
                                  p.priv_s) for p in who]
    objs = worker.send_pubkeys(jobs, rng=random.Random(2), now=now)
    assert all(o is not None for o in objs)
    for o in objs:
        assert targets.isProofOfWorkSufficient(o, recvTime=now)
    res = intake.check_objects(objs, streams=(1,), now=now)
    assert list(res.status) == [intake.OK] * 2 and list(res.objectType) == [worker.OBJECT_PUBKEY] * 2
    opened = receive.open_pubkeys(objs, {who[1].tag: who[1].address})
    assert list(opened.status) == [receive.OBJ_OK] * 2
    assert [opened.fromAddress(i) for i in range(2)] == [p.address for p in who]
