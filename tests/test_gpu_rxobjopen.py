"""The one-call opening of received broadcasts and pubkeys on the GPU (include/bmpow_rxobjopen.h,
pybitmessage_amd/receive.py: open_sealed_objects, open_sealed_broadcasts, open_sealed_pubkeys) against
tests/golden/rxobj_kats.json, which tests/test_rxobj.py pins to the reference, and against the compositions it
replaces (``receive.open_broadcasts`` and ``receive.open_pubkeys``: one ``bmpow_rx_walk_object`` per object, one
``decrypt_batch`` per distinct key, then ``bmpow_rx_objects``).  Everything is bit-exact."""
import ctypes
import hashlib
import hmac
import random

import numpy as np
import pytest

from tests.conftest import load_golden

pytestmark = pytest.mark.gpu

BROADCAST, PUBKEY_V4, PUBKEY = 0, 1, 2
# the reference's returning line -> BMPOW_RXO_* (include/bmpow_rx.h), per kind
LINE_STATUS = {
    BROADCAST: {None: 0, 'varint': 1, 760: 2, 830: 3, 838: 3, 848: 4, 882: 5, 893: 6, 901: 7, 916: 8, 801: 14, 810: 14, 820: 15},
    PUBKEY_V4: {None: 0, 'varint': 1, 484: 8, 497: 5, 457: 15, 417: 16, 442: 16, 423: 17, 428: 17, 411: 18},
    PUBKEY: {None: 0, 'varint': 1, 283: 9, 287: 10, 410: 11, 293: 12, 346: 12, 304: 13, 374: 8},
}
ORDER = int('fffffffffffffffffffffffffffffffebaaedce6af48a03bbfd25e8cd0364141', 16)
SET = 1 << 18  # objects of one ECIES set
TAIL = len(b'encrypted payload')
ROW_UP, ROW_DOWN = 120 + 16, 216 + 4  # a matched row's descriptors (rxo_row, rxs_row); its record and opened[]
SIZES = (0, 1, 7, 60, 200, 2000)


@pytest.fixture(scope='module')
def kats():
    return load_golden('rxobj_kats.json')


@pytest.fixture(scope='module')
def senders(gpulib):
    """Eight key pairs: (priv_signing, pub_signing64, pub_encryption64)."""
    from pybitmessage_amd import sender
    rng = random.Random(12)
    privs = [bytes(rng.randrange(1, 256) for _ in range(32)) for _ in range(16)]
    pubs = sender.priv_to_pub(privs)
    return [(privs[2 * i], pubs[2 * i][1:], pubs[2 * i + 1][1:]) for i in range(8)]


# ------------------------------------------------------------------ the fixture's field-by-field check
def walked_fields(res, i=0):
    r = res.recs[i]
    out = {'objectVersion': int(r['object_version']), 'objectStream': int(r['object_stream']), 'tagOff': int(r['tag_off']),
           'payloadOff': int(r['payload_off']), 'senderVersion': int(r['sender_version']),
           'senderStream': int(r['sender_stream']), 'behaviour': r['behaviour'].tobytes().hex(),
           'nonceTrialsPerByte': int(r['ntpb']), 'extraBytes': int(r['extra']), 'encoding': int(r['encoding']),
           'message': res.message(i).hex(), 'signature': res.signature(i).hex()}
    if r['kind'] == BROADCAST:
        out['pubkeyData'] = res.pubkeyData(i).hex()
    else:
        out['storedData'] = res.storedData(i).hex()
    return out


def check_row_against_fixture(kind, e, res, i):
    """The record went through the device: the comparisons and the verdict count."""
    want, rec = LINE_STATUS[kind][e['line']], res.recs[i]
    assert int(rec['kind']) == kind
    assert int(rec['status']) == want, e['name']
    if want in (5, 6) and kind == BROADCAST:  # the reference returns before it reads on
        assert (int(rec['encoding']), int(rec['msg_len']), int(rec['sig_len']), int(rec['bottom'])) == (0, 0, 0, 0)
    got = walked_fields(res, i)
    for k, v in (e['record'] or {}).items():
        assert got[k] == v, (e['name'], k)
    if e['signed'] is not None:
        signed = res.signedData(i)
        assert (len(signed), hashlib.sha256(signed).hexdigest()) == (e['signed']['len'], e['signed']['sha256']), e['name']
        assert int(rec['prefix_len']) == (0 if kind == PUBKEY else int(rec['payload_off']) - 8)


# ------------------------------------------------------------------ the compositions
def assert_equals_composition(kinds, objs, subs=(), needed=None):
    """Every row of open_sealed_objects against open_broadcasts / open_pubkeys, byte for byte; gives the batch."""
    from pybitmessage_amd import receive
    got = receive.open_sealed_objects(kinds, objs, subs, needed)
    assert len(got) == len(objs)
    for kind, old in ((BROADCAST, lambda o: receive.open_broadcasts(o, subs)), (PUBKEY, lambda o: receive.open_pubkeys(o, needed or {}))):
        idx = [i for i, k in enumerate(kinds) if k == kind]
        if not idx:
            continue
        want = old([objs[i] for i in idx])
        assert got.recs[idx].tobytes() == want.recs.tobytes(), \
            [(i, int(got.status[i]), int(want.status[j])) for j, i in enumerate(idx) if got.recs[i].tobytes() != want.recs[j].tobytes()]
        assert [got.plaintexts[i] for i in idx] == list(want.plaintexts)
        assert [i for i in got.accepted() if kinds[i] == kind] == [idx[j] for j in want.accepted()]
    return got


# ------------------------------------------------------------------ 1. the fixture
def test_fixture_in_one_call(gpulib, kats):
    from pybitmessage_amd import receive
    objs = [bytes.fromhex(e['obj']) for e in kats['broadcasts']]
    res = receive.open_sealed_broadcasts(objs, kats['subscriptions'])
    for i, e in enumerate(kats['broadcasts']):
        assert int(res.status[i]) == LINE_STATUS[BROADCAST][e['line']], e['name']
        assert res.plaintexts[i].hex() == (e['plaintext'] or ''), e['name']
        assert (int(res.match[i]) >= 0) == (e['plaintext'] is not None), e['name']
        if e['plaintext'] is not None:
            check_row_against_fixture(BROADCAST, e, res, i)
            assert int(res.digest[i]) == e['digest'], e['name']
        if e['result'] is not None:
            got = {'fromAddress': res.fromAddress(i), 'ripe': res.ripe(i).hex(), 'sigHash': res.sigHash(i).hex()}
            assert got == e['result'], e['name']
    assert res.accepted() == [i for i, e in enumerate(kats['broadcasts']) if e['line'] is None]
    assert_equals_composition([BROADCAST] * len(objs), objs, kats['subscriptions'])

    pk = kats['pubkeys_v4'] + kats['pubkeys']
    objs = [bytes.fromhex(e['obj']) for e in pk]
    needed = {bytes.fromhex(t): a for t, a in kats['needed'].items()}
    res = receive.open_sealed_pubkeys(objs, needed)
    n4 = len(kats['pubkeys_v4'])
    for i, e in enumerate(pk):
        kind = PUBKEY_V4 if i < n4 else PUBKEY
        line = e['line']
        if kind == PUBKEY and line == 410:
            line, kind = 411, PUBKEY_V4  # the call routes it: a clear pubkey's 233 bytes are below :411's floor
        if e['record'] is None:
            kind = PUBKEY  # a header varint raises before the version is known
        assert int(res.status[i]) == LINE_STATUS[kind][line] and int(res.kind[i]) == kind, e['name']
        if i < n4:
            if kind == PUBKEY_V4 and int(res.status[i]) not in (14, 15, 16, 17, 18):  # it was decrypted
                assert res.plaintexts[i].hex() == e['plaintext'] and int(res.match[i]) >= 0, e['name']
                check_row_against_fixture(kind, e, res, i)
            else:
                assert res.plaintexts[i] == b'', e['name']
        elif e['line'] != 410:
            check_row_against_fixture(kind, e, res, i)
            assert res.plaintexts[i] == b'' and int(res.match[i]) == -1
        if e['result'] is not None:
            assert (res.fromAddress(i), res.ripe(i).hex(), res.storedData(i).hex()) == \
                (e['result']['fromAddress'], e['result']['ripe'], e['result']['storedData']), e['name']
            assert res.sigHash(i) == bytes(32)
    assert res.accepted() == [i for i, e in enumerate(pk) if e['line'] is None]
    assert_equals_composition([PUBKEY] * len(objs), objs, (), needed)
    # both kinds, interleaved, in one call
    both = [(BROADCAST, bytes.fromhex(e['obj'])) for e in kats['broadcasts']]
    for k, o in enumerate(objs):
        both.insert(2 * k + 1, (PUBKEY, o))
    assert_equals_composition([k for k, _ in both], [o for _, o in both], kats['subscriptions'], needed)


# ------------------------------------------------------------------ sealed rows made here
def row(seed, kind, **kw):
    r = {'kind': kind, 'bv': 5, 'stream': 1, 'version': None, 'sender': seed % 8, 'message': b'Subject:s\nBody:b', 'alg': 'sha256',
         'seed': seed, 'ntpb': 1000, 'extra': 1000, 'spoil': None, 'cut': None}
    r.update(kw)
    if r['version'] is None:
        r['version'] = 3 if kind == PUBKEY or (kind == BROADCAST and r['bv'] == 4) else 4
    return r


def split_blob(blob):
    xl = int.from_bytes(blob[18:20], 'big')
    yl = int.from_bytes(blob[20 + xl:22 + xl], 'big')
    return blob[:18], blob[20:20 + xl], blob[22 + xl:22 + xl + yl], blob[22 + xl + yl:-32], blob[-32:]


def keys_of(priv, X, Y):
    from pybitmessage_amd import ecies
    h = hashlib.sha512(ecies.ecdh([priv], [(X, Y)])[0]).digest()
    return h[:32], h[32:]


def blob_of(front, X, Y, cipher, priv, zx=0):
    """A blob whose X carries zx extra leading zero bytes, MACed for the holder of priv."""
    body = front + (len(X) + zx).to_bytes(2, 'big') + bytes(zx) + X + len(Y).to_bytes(2, 'big') + Y + cipher
    return body + hmac.new(keys_of(priv, X, Y)[1], body, hashlib.sha256).digest()


def compose(rows, senders):
    """Signed objects of the three kinds made on the device, as tests/test_gpu_rxobj.py composes them but with every
    signature's nonce fixed by the row's seed, so that the same rows give the same bytes (and the same DER
    lengths) in every run: (kind, obj with b'encrypted payload' where the blob goes, plaintext) per row."""
    from pybitmessage_amd import addresses, sender
    from pybitmessage_amd.addressgen import encodeVarint as ev
    ident = addresses.derive_batch([senders[r['sender']][1] for r in rows], [senders[r['sender']][2] for r in rows],
                                   [r['version'] for r in rows], [r['stream'] for r in rows])
    heads, bodies = [], []
    for i, r in enumerate(rows):
        rng = random.Random(r['seed'])
        _, pub_s, pub_e = senders[r['sender']]
        keys = b'\x00\x00\x00\x01' + pub_s + pub_e
        head = bytes(rng.randrange(256) for _ in range(16))
        if r['kind'] == BROADCAST:
            head += b'\x00\x00\x00\x03' + ev(r['bv']) + ev(r['stream']) + (ident.tag[i].tobytes() if r['bv'] == 5 else b'')
            body = ev(r['version']) + ev(r['stream']) + keys
            if r['version'] >= 3:
                body += ev(r['ntpb']) + ev(r['extra'])
            body += ev(2) + ev(len(r['message'])) + r['message']
        elif r['kind'] == PUBKEY_V4:
            head += b'\x00\x00\x00\x01' + ev(4) + ev(r['stream']) + ident.tag[i].tobytes()
            body = keys + ev(r['ntpb']) + ev(r['extra'])
        else:
            head += b'\x00\x00\x00\x01' + ev(3) + ev(r['stream'])
            body = keys + ev(r['ntpb']) + ev(r['extra'])
        heads.append(head)
        bodies.append(body)
    sigs = [None] * len(rows)
    for alg in ('sha1', 'sha256'):
        idx = [i for i, r in enumerate(rows) if r['alg'] == alg]
        nonces = [hashlib.sha256(b'nonce of row %d' % rows[i]['seed']).digest() for i in idx]
        signed = [heads[i][8:] + bodies[i] for i in idx]
        for i, sig in zip(idx, sender.sign_batch(signed, [senders[rows[i]['sender']][0] for i in idx], alg, nonces=nonces)):
            assert sig is not None
            sigs[i] = sig
    out = []
    for r, h, b, sig in zip(rows, heads, bodies, sigs):
        tail = ev(len(sig)) + sig
        out.append((PUBKEY, h + b + tail, None) if r['kind'] == PUBKEY else (r['kind'], h + b'encrypted payload', b + tail))
    return out


def sealed(rows, senders, seed=1):
    """Wire objects of the three kinds, signed and sealed on the device: ``(kinds, objs, addresses, privs)`` with
    the address each object is filed under and its private key (None for a clear pubkey).  ``spoil``: 'mac',
    'padding', 'signature', 'keys', 'tag', 'stream'; ``cut``: only that many bytes of the plaintext are sealed."""
    from pybitmessage_amd import addresses, ecies, sender
    made = compose(rows, senders)
    # 'keys': the address is that of the next sender, whose keys the object does not carry
    owner = [(r['sender'] + 1) % 8 if r['spoil'] == 'keys' else r['sender'] for r in rows]
    ident = addresses.derive_batch([senders[s][1] for s in owner], [senders[s][2] for s in owner], [r['version'] for r in rows],
                                   [r['stream'] for r in rows])
    addrs = [ident.address(i) for i in range(len(rows))]
    keys = addresses.address_keys(addrs)
    privs = [ecies._key32(k[5]) for k in keys]
    pubs = [p[1:] for p in sender.priv_to_pub(privs)]
    rng = random.Random(seed)
    kinds, objs = [], []
    enc = [i for i, r in enumerate(rows) if r['kind'] != PUBKEY]
    plains = []
    for i in enc:
        plain, r = made[i][2], rows[i]
        if r['spoil'] == 'signature':
            plain = plain[:-1] + bytes([plain[-1] ^ 1])
        if r['spoil'] == 'stream' and r['kind'] == BROADCAST:
            plain = plain[:1] + bytes([plain[1] ^ 2]) + plain[2:]  # the inner stream, one byte
        if r['cut'] is not None:
            assert r['cut'] <= len(plain)
            plain = plain[:r['cut']]
        plains.append(plain)
    eph = [bytes(rng.randrange(1, 256) for _ in range(32)) for _ in enc]
    ivs = [bytes(rng.randrange(256) for _ in range(16)) for _ in enc]
    blobs = dict(zip(enc, sender.encrypt_batch(plains, [pubs[i] for i in enc], ephemeral=eph, ivs=ivs)))
    for i, r in enumerate(rows):
        kind, obj = made[i][0], made[i][1]
        if kind != PUBKEY:
            blob = blobs[i]
            if r['spoil'] == 'mac':
                blob = blob[:-1] + bytes([blob[-1] ^ 1])
            if r['spoil'] == 'padding':
                # CBC: the top bit of the last byte of the block before the last flips the top bit of the pad byte,
                # which is then above 16; the MAC is made again over the changed ciphertext, so it verifies
                front, X, Y, cipher, _mac = split_blob(blob)
                assert len(cipher) >= 32
                blob = blob_of(front, X, Y, cipher[:-17] + bytes([cipher[-17] ^ 0x80]) + cipher[-16:], privs[i])
            obj = obj[:-TAIL] + blob
            at = len(obj) - len(blob) - 32
            if r['spoil'] == 'keys' and (kind == PUBKEY_V4 or r['bv'] == 5):  # filed under the owner's tag
                obj = obj[:at] + ident.tag[i].tobytes() + obj[at + 32:]
            if r['spoil'] == 'tag':
                obj = obj[:at] + bytes([obj[at] ^ 1]) + obj[at + 1:]
            if r['spoil'] == 'stream' and kind == PUBKEY_V4:
                obj = obj[:21] + bytes([obj[21] ^ 2]) + obj[22:]  # the outer stream: the address's is another
            kind = PUBKEY if kind == PUBKEY_V4 else kind
        kinds.append(kind)
        objs.append(obj)
    return kinds, objs, addrs, [None if r['kind'] == PUBKEY else p for r, p in zip(rows, privs)]


def tables_for(rows, addrs):
    """(subscriptions, needed) that hold every row's address."""
    from pybitmessage_amd import addresses
    subs = [a for r, a in zip(rows, addrs) if r['kind'] == BROADCAST]
    want = [a for r, a in zip(rows, addrs) if r['kind'] == PUBKEY_V4]
    needed = {k[4]: a for a, k in zip(want, addresses.address_keys(want))}
    return list(dict.fromkeys(subs)), needed


N_MIXED = 320


def mixed_rows():
    rows = []
    for k in range(N_MIXED):
        kind = (BROADCAST, BROADCAST, PUBKEY_V4, PUBKEY)[k % 4]
        bv = (5, 4)[(k // 4) % 2] if k % 4 < 2 else 5
        # a tagged row has its own stream: its own address, key and tag.  A v2 / v3 subscription is kept under its
        # ripe, which the stream does not enter (``shared.py:170``): one address per sender, its stream fixed
        who = (k // 8) % 8 if kind == BROADCAST and bv == 4 else k % 8
        rows.append(row(k, kind, bv=bv, stream=30 + (who if kind == BROADCAST and bv == 4 else k), sender=who,
                        message=bytes([k % 251]) * SIZES[k % 6], alg=('sha1', 'sha256')[(k // 3) % 2]))
    for j, spoil in enumerate(('mac', 'padding', 'signature', 'keys', 'tag', 'stream')):
        rows.append(row(300 + j, BROADCAST, bv=5, stream=20 + j, spoil=spoil, message=b'spoiled v5 ' * 5))
        # sealed to a subscribed v3 address: the sender's own, or for 'keys' the next sender's
        rows.append(row(320 + j, BROADCAST, bv=4, sender=j, stream=30 + (j + 1 if spoil == 'keys' else j),
                        spoil=spoil if spoil != 'tag' else 'mac', message=b'spoiled v4'))
        rows.append(row(340 + j, PUBKEY_V4, stream=20 + j, spoil=spoil))
    return rows


# ------------------------------------------------------------------ 2. equals the composition
def test_equals_the_composition_on_mixed_rows(gpulib, senders):
    from pybitmessage_amd import receive
    rows = mixed_rows()
    kinds, objs, addrs, _ = sealed(rows, senders)
    subs, needed = tables_for(rows, addrs)
    tables = receive.sealed_tables(subs, needed)
    assert len(tables.tags) + len(tables.needed_tags) >= 70 and len(tables.tags) >= 70  # one wave, more than 64 keys
    assert len(tables.trial_privs) >= 8
    got = assert_equals_composition(kinds, objs, subs, needed)
    st = got.status[:N_MIXED].tolist()
    assert st == [receive.OBJ_OK] * N_MIXED
    assert [got.message(i) for i in range(N_MIXED) if rows[i]['kind'] == BROADCAST] == [r['message'] for r in rows[:N_MIXED] if r['kind'] == BROADCAST]
    seen = {(rows[i]['kind'], rows[i]['spoil'], int(got.status[i])) for i in range(N_MIXED, len(rows))}
    assert {(BROADCAST, 'mac', receive.OBJ_NOT_DECRYPTED), (BROADCAST, 'mac', receive.OBJ_NOT_SUBSCRIBED),
            (BROADCAST, 'padding', receive.OBJ_NOT_DECRYPTED), (BROADCAST, 'signature', receive.OBJ_BAD_SIGNATURE),
            (BROADCAST, 'keys', receive.OBJ_WRONG_TAG), (BROADCAST, 'keys', receive.OBJ_WRONG_RIPE),
            (BROADCAST, 'tag', receive.OBJ_NOT_SUBSCRIBED), (BROADCAST, 'stream', receive.OBJ_STREAM_MISMATCH),
            (PUBKEY_V4, 'mac', receive.OBJ_NOT_DECRYPTED), (PUBKEY_V4, 'padding', receive.OBJ_NOT_DECRYPTED),
            (PUBKEY_V4, 'signature', receive.OBJ_BAD_SIGNATURE), (PUBKEY_V4, 'keys', receive.OBJ_BAD_SIGNATURE),
            (PUBKEY_V4, 'tag', receive.OBJ_NOT_NEEDED), (PUBKEY_V4, 'stream', receive.OBJ_ADDRESS_MISMATCH)} <= seen
    # a MAC that verifies over bad padding names its key and leaves no plaintext
    for i in range(N_MIXED, len(rows)):
        if rows[i]['spoil'] == 'padding':
            assert int(got.match[i]) >= 0 and got.plaintexts[i] == b''
    # match[] indexes the table that opened the row
    for i in range(N_MIXED):
        if rows[i]['kind'] == PUBKEY:
            assert int(got.match[i]) == -1
        elif rows[i]['kind'] == PUBKEY_V4:
            assert tables.needed_tags[int(got.match[i])] == objs[i][int(got.recs[i]['tag_off']):int(got.recs[i]['payload_off'])]
        elif rows[i]['bv'] == 5:
            assert tables.tags[int(got.match[i])] == objs[i][int(got.recs[i]['tag_off']):int(got.recs[i]['payload_off'])]
        else:
            assert tables.trial_ripes[int(got.match[i])] == got.ripe(i)


# ------------------------------------------------------------------ 3. per-lane keys, by the raw tables
def tagged_broadcast(tag, blob, seed):
    return bytes(random.Random(seed).randrange(256) for _ in range(16)) + b'\x00\x00\x00\x03\x05\x01' + tag + blob


def test_per_lane_keys_on_constructed_scalars(gpulib):
    from pybitmessage_amd import ecies, receive, sender
    rng = random.Random(77)
    scalars = [1, 2, ORDER - 1, ORDER - 2, int('0' + 'f' * 63, 16), int('f' * 32, 16), int('f' * 31 + '0' * 32 + '1', 16)]
    scalars += [1 << k for k in (1, 4, 5, 31, 32, 63, 64, 127, 128, 200, 252, 255)]
    scalars += [(1 << k) - 1 for k in (4, 5, 64, 129, 255)] + [ORDER - (1 << k) for k in (4, 64, 128)]
    while len(scalars) < 64:
        scalars.append(rng.randrange(1, ORDER))
    privs = [s.to_bytes(32, 'big') for s in scalars]
    pubs = [p[1:] for p in sender.priv_to_pub(privs)]
    tags = [hashlib.sha256(b'tag %d' % k).digest() for k in range(64)]
    # wave 0: 64 rows under key 0 .. wave 1: 64 rows under 64 different keys; then three rows of entries that repeat
    use = [5] * 64 + list(range(64)) + [0, 63, 2]
    plains = [bytes([k % 256]) * 40 + b'row %d' % k for k in range(len(use))]
    eph = [bytes(rng.randrange(1, 256) for _ in range(32)) for _ in use]
    ivs = [bytes(rng.randrange(256) for _ in range(16)) for _ in use]
    blobs = sender.encrypt_batch(plains, [pubs[u] for u in use], ephemeral=eph, ivs=ivs)
    objs = [tagged_broadcast(tags[u], b, k) for k, (u, b) in enumerate(zip(use, blobs))]
    # the last row: filed under tag 2 but sealed to key 3 -- its own key must not open it
    objs[-1] = tagged_broadcast(tags[2], sender.encrypt_batch([b'x' * 46], [pubs[3]], ephemeral=[eph[0]], ivs=[ivs[0]])[0], 999)
    tables = receive.SealedTables(tags=(tags, privs))
    receive.sealed_obj_reset_stats()
    got = receive.open_sealed_tables([BROADCAST] * len(objs), objs, tables)
    st = receive.sealed_obj_stats()
    assert (st['tagged_tries'], st['trial_tries'], st['sets']) == (len(objs), 0, 1)
    assert got.match.tolist() == use[:-1] + [-1]
    for k, (u, o) in enumerate(zip(use, objs)):
        want = ecies.decrypt_batch([o[54:]], [privs[2 if k == len(use) - 1 else u]])[0]
        if k == len(use) - 1:
            assert want is None and got.plaintexts[k] == b'' and int(got.status[k]) == receive.OBJ_NOT_DECRYPTED
        else:
            assert want == (0, plains[k]) and got.plaintexts[k] == plains[k], (k, hex(scalars[u]))


# ------------------------------------------------------------------ 4. row counts
@pytest.fixture(scope='module')
def handful(gpulib, senders):
    """Objects of about one size: tagged and trial broadcasts and v4 pubkeys for the tables (one spoiled), the
    same for nobody's tables, clear pubkeys, one head that refuses: (mine, others, clear, refused, subs, needed)."""
    rows = [row(20 + k, (BROADCAST, BROADCAST, PUBKEY_V4)[k % 3], bv=(5, 4, 5)[k % 3], stream=2 + k, message=bytes([k]) * (40 + k),
                spoil='signature' if k == 5 else None) for k in range(6)]
    rows += [row(30 + k, (BROADCAST, BROADCAST, PUBKEY_V4, BROADCAST)[k], bv=(5, 4, 5, 5)[k], stream=40 + k, message=bytes([k]) * 44)
             for k in range(4)]
    rows += [row(50, PUBKEY), row(51, PUBKEY, stream=300)]
    kinds, objs, addrs, _ = sealed(rows, senders, seed=6)
    subs, needed = tables_for(rows[:6], addrs[:6])
    mine, others, clear = list(zip(kinds[:6], objs[:6])), list(zip(kinds[6:10], objs[6:10])), list(zip(kinds[10:], objs[10:]))
    refused = (BROADCAST, objs[0][:20] + b'\x03' + objs[0][21:])
    return mine, others, clear, refused, subs, needed


def run(batch, subs, needed):
    return assert_equals_composition([k for k, _ in batch], [o for _, o in batch], subs, needed)


@pytest.mark.parametrize('n', [1, 63, 64, 65, 129])
def test_row_counts_and_interleaved_matches(gpulib, handful, n):
    from pybitmessage_amd import receive
    mine, others, _clear, refused, subs, needed = handful
    batch = [mine[(k // 2) % 6] if k % 2 == 0 else (others + [refused])[(k // 2) % 5] for k in range(n)]
    receive.sealed_obj_reset_stats()
    got = run(batch, subs, needed)
    st = receive.sealed_obj_stats()
    assert (st['calls'], st['rows'], st['sets'], st['matched'], st['clear']) == (1, n, 1, (n + 1) // 2, 0)
    assert st['rx_launches'] == 10 and st['launches'] == 11 + (3 if n > 2 else 0) + 3
    assert [int(m) >= 0 for m in got.match] == [k % 2 == 0 for k in range(n)]


def test_no_match_at_all_and_every_row_matches(gpulib, handful):
    from pybitmessage_amd import receive
    mine, others, _clear, refused, subs, needed = handful
    receive.sealed_obj_reset_stats()
    got = run(others * 20 + [refused], subs, needed)
    st = receive.sealed_obj_stats()
    assert got.match.tolist() == [-1] * 81 and got.accepted() == []
    # only the v4 broadcasts of nobody's tables are tried at all: their tags and needed entries are unknown
    assert (st['calls'], st['sets'], st['matched'], st['rx_launches'], st['launches']) == (1, 1, 0, 0, 4)
    assert (st['trial_tries'], st['tagged_tries']) == (20 * len(receive.sealed_tables(subs, needed).trial_privs), 0)
    assert st['open_ms'] == 0 and st['walk_ms'] == 0 and st['curve_ms'] == 0 and st['match_ms'] > 0
    receive.sealed_obj_reset_stats()
    got = run(mine * 11, subs, needed)
    st = receive.sealed_obj_stats()
    assert all(int(m) >= 0 for m in got.match) and (st['matched'], st['rx_launches'], st['launches']) == (66, 10, 17)
    assert all(st[k] > 0 for k in ('match_ms', 'open_ms', 'walk_ms', 'hash_ms', 'scalar_ms', 'curve_ms', 'ident_ms',
                                   'finish_ms', 'host_ms'))


# ------------------------------------------------------------------ 5. ciphertext alignments and padding
def test_alignments_and_padding_on_both_sides_of_a_block(gpulib, senders):
    from pybitmessage_amd import receive
    # One v5 broadcast, one v4 broadcast and one v4 pubkey, each sealed whole and cut to every length of a span that
    # crosses 16-byte and 64-byte boundaries of the ciphertext: every pad length 1 .. 16 by construction, whatever
    # the signatures' lengths.  A cut plaintext has lost its signature's end: the composition says what it is then.
    # (A v4 pubkey object needs 350 bytes, :411: a ciphertext of 192 bytes at least, a plaintext of 176.)
    spans = ((BROADCAST, 5, range(120, 201)), (BROADCAST, 4, range(120, 201)), (PUBKEY_V4, 5, range(176, 209)))
    rows = []
    for kind, bv, span in spans:
        rows += [row(60, kind, bv=bv, stream=3, message=b'm' * 40, extra=70000, cut=n) for n in span]
        rows.append(row(60, kind, bv=bv, stream=3, message=b'm' * 40, extra=70000))
    kinds, objs, addrs, privs = sealed(rows, senders, seed=9)
    subs, needed = tables_for(rows, addrs)
    got = run(list(zip(kinds, objs)), subs, needed)
    plans = [receive.sealed_object_plan(k, o) for k, o in zip(kinds, objs)]
    clens = [p[6] for p in plans]
    at = 0
    for kind, bv, span in spans:
        cut = list(range(at, at + len(span)))
        assert [len(got.plaintexts[i]) for i in cut] == list(span)
        assert [clens[i] for i in cut] == [16 * (n // 16 + 1) for n in span]
        assert {clens[i] - len(got.plaintexts[i]) for i in cut} == set(range(1, 17))
        assert len({len(got.plaintexts[i]) // 64 for i in cut}) >= 2 and all(int(got.match[i]) >= 0 for i in cut)
        assert int(got.status[at + len(span)]) == receive.OBJ_OK  # the whole one
        at += len(span) + 1
    # every alignment of the ciphertext in the pool: X re-encoded with leading zero bytes and MACed again
    i = len(spans[0][2])  # the whole v5 broadcast
    at = plans[i][3]
    front, X, Y, cipher, _mac = split_blob(objs[i][at:])
    moved = [objs[i][:at] + blob_of(front, X, Y, cipher, privs[i], zx=z) for z in range(16)]
    got = run([(BROADCAST, o) for o in moved], subs, needed)
    assert {receive.sealed_object_plan(BROADCAST, o)[5] % 16 for o in moved} == set(range(16))
    assert all(got.recs[k].tobytes() == got.recs[0].tobytes() and got.plaintexts[k] == got.plaintexts[0] for k in range(16))
    assert got.status.tolist() == [receive.OBJ_OK] * 16
    # a MAC that verifies over a ciphertext of 8 bytes and of none
    bad = [objs[i][:at] + blob_of(front, X, Y, c, privs[i]) for c in (cipher[:8], b'', cipher[:17])]
    got = run([(BROADCAST, o) for o in bad], subs, needed)
    assert got.status.tolist() == [receive.OBJ_NOT_DECRYPTED] * 3 and all(int(m) >= 0 for m in got.match)


# ------------------------------------------------------------------ 6. two sets
def test_two_sets(gpulib, handful):
    """2^18 + 2 tried objects of one MAC block count, so the sets split in input order: tagged and trial rows, and
    matches of both, on either side."""
    from pybitmessage_amd import receive
    mine, others, _clear, _refused, subs, needed = handful
    blocks = lambda o: (len(o) - receive.sealed_object_plan(BROADCAST, o)[3] - 32 + 9 + 63) // 64  # noqa: E731
    v4_other, v5_mine, v4_mine = others[1][1], mine[0][1], mine[1][1]
    # a v5 broadcast under a subscribed tag that its key does not open: tried, never matched
    v5_other = v5_mine[:-1] + bytes([v5_mine[-1] ^ 1])
    assert len({blocks(o) for o in (v4_other, v5_mine, v4_mine, v5_other)}) == 1
    n = SET + 2
    hits = {0: v5_mine, 77: v4_mine, SET - 1: v5_mine, SET: v4_mine, SET + 1: v5_mine}
    objs = [hits.get(i, v4_other if i % 2 else v5_other) for i in range(n)]
    small = receive.open_sealed_broadcasts([v4_other, v5_mine, v4_mine, v5_other], subs)
    record = {o: small.recs[k].tobytes() for k, o in enumerate([v4_other, v5_mine, v4_mine, v5_other])}
    plain = {o: small.plaintexts[k] for k, o in enumerate([v4_other, v5_mine, v4_mine, v5_other])}
    receive.sealed_obj_reset_stats()
    got = receive.open_sealed_broadcasts(objs, subs)
    st = receive.sealed_obj_stats()
    groups = 1  # the trial keys fit one group
    assert (st['calls'], st['rows'], st['sets'], st['matched'], st['rx_launches']) == (1, n, 2, 5, 20)
    assert st['launches'] == 2 * (1 + 3 * groups + 3 + 10)
    assert st['tagged_tries'] > 0 and st['trial_tries'] > 0 and st['tagged_tries'] + st['trial_tries'] // len(
        receive.sealed_tables(subs).trial_privs) == n
    assert np.flatnonzero(got.status == receive.OBJ_OK).tolist() == sorted(hits)
    for i in list(hits) + [1, 2, 3, 4, SET - 2, SET - 3]:
        assert got.recs[i].tobytes() == record[objs[i]] and got.plaintexts[i] == plain[objs[i]], i


# ------------------------------------------------------------------ 7. abort, empty input, degenerate tables
def test_abort_empty_input_and_degenerate_tables(gpulib, handful):
    from pybitmessage_amd import _lib, addresses, receive
    mine, others, clear, refused, subs, needed = handful
    batch = mine + others + clear + [refused]
    gpulib.bmpow_abort()
    try:
        with pytest.raises(_lib.BmpowError) as e:
            receive.open_sealed_objects([k for k, _ in batch], [o for _, o in batch], subs, needed)
        assert e.value.code == _lib.E_ABORTED
    finally:
        gpulib.bmpow_clear_abort()
    got = run(batch, subs, needed)
    assert [int(m) >= 0 for m in got.match] == [True] * 6 + [False] * 7
    assert len(receive.open_sealed_objects([], [], subs, needed)) == 0
    assert len(receive.open_sealed_broadcasts([], subs)) == 0 and len(receive.open_sealed_pubkeys([], needed)) == 0
    # empty tables: nothing that needs a key is launched, the clear pubkeys still take their nine
    receive.sealed_obj_reset_stats()
    got = run(batch, (), None)
    st = receive.sealed_obj_stats()
    assert (st['sets'], st['tagged_tries'], st['trial_tries'], st['matched'], st['clear'], st['launches']) == (0, 0, 0, 0, 2, 9)
    assert got.accepted() == [10, 11] and got.match.tolist() == [-1] * 13
    # only trial keys; only tags
    v3 = [a for a, k in zip(subs, addresses.address_keys(subs)) if k[1] <= 3]
    v4 = [a for a in subs if a not in v3]
    assert v3 and v4
    receive.sealed_obj_reset_stats()
    got = run(batch, v3, None)
    st = receive.sealed_obj_stats()
    assert st['tagged_tries'] == 0 and st['trial_tries'] > 0 and got.accepted() == [1, 4, 10, 11]
    receive.sealed_obj_reset_stats()
    got = run(batch, v4, None)
    st = receive.sealed_obj_stats()
    assert st['tagged_tries'] == 2 and st['trial_tries'] == 0 and got.accepted() == [0, 3, 10, 11]
    # a tag twice in the table: the first entry wins, whatever the second one's key
    t = receive.sealed_tables(subs, needed)
    tag = mine[0][1][22:54]
    at = t.tags.index(tag)
    other_key = bytes(31) + b'\x07'
    first = receive.SealedTables(tags=([tag, tag], [t.tag_privs[at], other_key]))
    second = receive.SealedTables(tags=([tag, tag], [other_key, t.tag_privs[at]]))
    got = receive.open_sealed_tables([BROADCAST], [mine[0][1]], first)
    assert (int(got.status[0]), int(got.match[0])) == (receive.OBJ_OK, 0)
    got = receive.open_sealed_tables([BROADCAST], [mine[0][1]], second)
    assert (int(got.status[0]), int(got.match[0]), got.plaintexts[0]) == (receive.OBJ_NOT_DECRYPTED, -1, b'')


# ------------------------------------------------------------------ 8. what crosses the bus
def test_byte_counters(gpulib, handful):
    from pybitmessage_amd import receive
    mine, others, clear, refused, subs, needed = handful
    batch = (mine + others) * 3 + clear + [refused]
    t = receive.sealed_tables(subs, needed)
    plans = [receive.sealed_object_plan(k, o) for k, o in batch]
    # tried: everything of mine, and of the others the v4 broadcast (every trial key tries it)
    tried = [i for i, (k, o) in enumerate(batch) if (k, o) in mine or (k, o) == others[1]]
    pool = sum((len(batch[i][1]) - plans[i][3] - 32 + 9 + 63) // 64 * 64 for i in tried)
    opened = [plans[i][6] for i in tried if batch[i] in mine]
    tagged = sum(1 for i in tried if batch[i] in mine and not (batch[i][0] == BROADCAST and plans[i][3] == plans[i][4]))
    receive.sealed_obj_reset_stats()
    got = receive.open_sealed_objects([k for k, _ in batch], [o for _, o in batch], subs, needed)
    st = receive.sealed_obj_stats()
    assert int((got.match >= 0).sum()) == st['matched'] == 18 and st['clear'] == 2 and st['tagged_tries'] == tagged == 12
    keys = len(t.trial_privs) + len(t.tags) + len(t.needed_tags)
    clear_up = sum((len(o) + 15) // 16 * 16 + 120 for _, o in clear)
    # up: the padded MAC pool (each ciphertext once), a point (64 B) and an ec_obj (40 B) per tried object, 64 digits
    # of 4 B per key, a key index per tagged row, the matched rows' descriptors, the clear pubkeys and theirs --
    # and not a byte of plaintext
    assert st['bytes_up'] == pool + len(tried) * (64 + 40) + keys * 64 * 4 + 4 * tagged + 18 * ROW_UP + clear_up
    # down: match[] of the tried objects; per matched row its record, opened[] and its plaintext slot; a clear
    # pubkey's record
    assert st['bytes_down'] == 4 * len(tried) + 18 * ROW_DOWN + sum(opened) + 2 * 216


# ------------------------------------------------------------------ 9. the neighbours
def test_neighbours_are_unchanged_in_the_same_process(gpulib, handful, kats):
    from pybitmessage_amd import _lib, ecies, receive, sender
    from tests.test_rxobj import device_rows
    mine, others, clear, refused, subs, needed = handful
    rx = load_golden('rx_kats.json')
    msg_keys = {bytes.fromhex(k['ripe']): bytes.fromhex(k['privkey']) for k in rx['recipients']}
    msgs = [bytes.fromhex(m['obj']) for m in rx['msgs']]
    rows = device_rows(kats)
    bcs = [bytes.fromhex(e['obj']) for e in kats['broadcasts']]
    payloads = [o[receive.sealed_object_plan(k, o)[3]:] for k, o in mine]
    privs = receive.sealed_tables(subs, needed).trial_privs

    def neighbours():
        a = receive.open_sealed_msgs(msgs, msg_keys)
        b = receive.open_objects([r[0] for r in rows], [r[2] for r in rows], [r[3] for r in rows], [r[4] for r in rows])
        c = receive.open_broadcasts(bcs, kats['subscriptions'])
        return (a.recs.tobytes(), list(a.plaintexts), a.match.tolist(), b.recs.tobytes(), c.recs.tobytes(), list(c.plaintexts),
                ecies.match_keys(payloads, privs))

    def counters():
        st = _lib.BmpowEciesStats()
        assert gpulib.bmpow_ecies_get_stats(ctypes.byref(st)) == 0
        return ([getattr(st, f) for f, _ in st._fields_], receive.stats(), sender.seal_stats(), receive.obj_stats(),
                receive.sealed_stats())

    before = neighbours()
    quiet = counters()
    batch = mine + others + clear + [refused]
    got = receive.open_sealed_objects([k for k, _ in batch], [o for _, o in batch], subs, needed)
    assert len(got.accepted()) == 7
    assert counters() == quiet
    assert neighbours() == before
