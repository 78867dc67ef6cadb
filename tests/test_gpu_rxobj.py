"""Broadcast and pubkey processing on the GPU (include/bmpow_rx.h: bmpow_rx_objects; pybitmessage_amd/receive.py:
open_objects, open_broadcasts, open_pubkeys) against tests/golden/rxobj_kats.json and the broadcasts and encrypted
pubkeys of ident_kats.json, which tests/test_rxobj.py pins to the reference, and against the composition the
library offered before (the extractors of ``signatures`` per object, ``verify_batch_digest``, ``derive_batch``,
comparisons and hashlib in Python; ``process_broadcasts``, ``check_pubkeys_v4``).  Everything is bit-exact."""
import hashlib
import random

import numpy as np
import pytest

from tests.conftest import load_golden
from tests.test_rxobj import BROADCAST, LINE_STATUS, PUBKEY, PUBKEY_V4, check_row_against_fixture, device_rows

pytestmark = pytest.mark.gpu

SET = 1 << 18  # rows of one launch set
STREAMS = (7, 300, 70000, 2 ** 32)  # varints of 1, 3, 5 and 9 bytes


@pytest.fixture(scope='module')
def kats():
    return load_golden('rxobj_kats.json')


@pytest.fixture(scope='module')
def ident_kats():
    return load_golden('ident_kats.json')


@pytest.fixture(scope='module')
def senders(gpulib):
    """Eight key pairs: (priv_signing, pub_signing64, pub_encryption64)."""
    from pybitmessage_amd import sender
    rng = random.Random(12)
    privs = [bytes(rng.randrange(1, 256) for _ in range(32)) for _ in range(16)]
    pubs = sender.priv_to_pub(privs)
    return [(privs[2 * i], pubs[2 * i][1:], pubs[2 * i + 1][1:]) for i in range(8)]


def row(seed, kind, **kw):
    r = {'kind': kind, 'bv': 5, 'stream': 1, 'version': None, 'sender': seed % 8, 'message': b'Subject:s\nBody:b', 'alg': 'sha256',
         'seed': seed, 'ntpb': 1000, 'extra': 1000}
    r.update(kw)
    if r['version'] is None:
        r['version'] = 3 if kind == PUBKEY or (kind == BROADCAST and r['bv'] == 4) else 4
    return r


def compose(rows, senders):
    """Signed objects of the three kinds made on the device: (kind, obj, plaintext, expect) per row, and the
    signed data.  A broadcast's plaintext carries the message, a pubkey's the difficulty varints only."""
    from pybitmessage_amd import addresses, sender
    from pybitmessage_amd.addressgen import encodeVarint as ev
    ident = addresses.derive_batch([senders[r['sender']][1] for r in rows], [senders[r['sender']][2] for r in rows],
                                   [r['version'] for r in rows], [r['stream'] for r in rows])
    heads, bodies, expects = [], [], []
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
        expects.append(ident.ripe[i].tobytes())
    signed = [h[8:] + b for h, b in zip(heads, bodies)]
    sigs = [None] * len(rows)
    for alg in ('sha1', 'sha256'):
        idx = [i for i, r in enumerate(rows) if r['alg'] == alg]
        for i, s in zip(idx, sender.sign_batch([signed[i] for i in idx], [senders[rows[i]['sender']][0] for i in idx], alg)):
            assert s is not None
            sigs[i] = s
    out = []
    for r, h, b, s, e in zip(rows, heads, bodies, sigs, expects):
        tail = ev(len(s)) + s
        if r['kind'] == PUBKEY:
            out.append((PUBKEY, h + b + tail, None, None))
        else:
            out.append((r['kind'], h + b'encrypted payload', b + tail, e))
    return out, signed


def open_rows(rows):
    from pybitmessage_amd import receive
    return receive.open_objects([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows])


def composition(rows):
    """The older route for raw rows: per row None, or (digest, ripe, fromAddress, sigHash or None, signature)."""
    from pybitmessage_amd import addresses, signatures
    got = []
    for kind, obj, plain, _expect in rows:
        if kind == BROADCAST:
            p = signatures.broadcast_signed_parts(obj, plain)
            got.append(None if p is None else (p.signedData, p.signature, p.pubSigningKey64, p.pubEncryptionKey64, p.senderVersion, p.senderStream))
        elif kind == PUBKEY_V4:
            p = signatures.pubkey_v4_signed_parts(obj, plain)
            got.append(None if p is None else (p.signedData, p.signature, p.pubSigningKey64, p.pubEncryptionKey64, p.addressVersion, p.stream))
        else:
            p, head = signatures.pubkey_v3_signed_parts(obj), signatures.pubkey_v4_header(obj)
            at = 0 if head is None else head[3] - 32 + 4 + 64
            got.append(None if p is None else (p[0], p[1], p[2], obj[at:at + 64], head[0], head[1]))
    live = [i for i, g in enumerate(got) if g is not None and len(g[2]) == 64 and len(g[3]) == 64]
    verdicts = signatures.verify_batch_digest([got[i][0] for i in live], [got[i][1] for i in live], [got[i][2] for i in live])
    ident = addresses.derive_batch([got[i][2] for i in live], [got[i][3] for i in live], [got[i][4] for i in live],
                                   [got[i][5] for i in live])
    out = [None] * len(rows)
    # an encrypted pubkey's key cut short by the end of the plaintext is no key: verify says False (protocol.py:484)
    bad_signature = [i for i, g in enumerate(got) if g is not None and i not in set(live) and rows[i][0] == PUBKEY_V4]
    for j, i in enumerate(live):
        kind, obj, _plain, expect = rows[i]
        ripe = ident.ripe[j].tobytes()
        if kind == BROADCAST:
            head = signatures.broadcast_header(obj)
            same = ripe == expect if head[0] == 4 else ident.tag[j].tobytes() == head[2]
        else:
            same = kind == PUBKEY or ripe == expect
        if not verdicts[j] and (same or kind != BROADCAST):
            bad_signature.append(i)
        if same and verdicts[j]:
            sig_hash = hashlib.sha512(hashlib.sha512(got[i][1]).digest()).digest()[32:] if kind == BROADCAST else None
            out[i] = (verdicts[j], ripe, ident.address(j), sig_hash, got[i][1])
    return out, sorted(bad_signature)


def assert_equals_composition(res, rows):
    from pybitmessage_amd import receive
    want, bad_signature = composition(rows)
    assert res.accepted() == [i for i, w in enumerate(want) if w is not None]
    for i in res.accepted():
        sig_hash = res.sigHash(i) if rows[i][0] == BROADCAST else None
        assert (int(res.digest[i]), res.ripe(i), res.fromAddress(i), sig_hash, res.signature(i)) == want[i], i
        if rows[i][0] != BROADCAST:
            assert res.sigHash(i) == bytes(32)
    assert [i for i in range(len(rows)) if res.status[i] == receive.OBJ_BAD_SIGNATURE] == bad_signature
    return want, bad_signature


@pytest.fixture(scope='module')
def ident_rows(gpulib, ident_kats):
    """(kind, entry, obj, plaintext, expect) of ident_kats.json's rows that have a plaintext; a v4 broadcast's
    expected ripe is that of the subscription key that opens it."""
    from pybitmessage_amd import addresses, ecies, signatures
    subs = [(bytes.fromhex(s['ripe']), bytes.fromhex(s['privkey'])) for s in ident_kats['subscriptions'] if s['version'] <= 3]
    out = []
    for b in ident_kats['broadcasts']:
        if b['plaintext'] is None:
            continue
        obj, expect = bytes.fromhex(b['obj']), b''
        head = signatures.broadcast_header(obj)
        if head[0] == 4:
            opened = ecies.decrypt_batch([obj[head[3]:]], [k for _, k in subs])[0]
            assert opened is not None and opened[1].hex() == b['plaintext']
            expect = subs[opened[0]][0]
        out.append((BROADCAST, b, obj, bytes.fromhex(b['plaintext']), expect))
    for k in ident_kats['pubkeys_v4']:
        ripe = addresses.decodeAddress(k['address'])[3]
        out.append((PUBKEY_V4, k, bytes.fromhex(k['obj']), bytes.fromhex(k['plaintext']), ripe if len(ripe) == 20 else b''))
    return out


def test_both_fixtures_in_one_call(gpulib, kats, ident_rows):
    from pybitmessage_amd import receive
    own = device_rows(kats)
    rows, a, b = [], list(own), list(ident_rows)
    while a or b:  # the kinds and the two fixtures interleaved
        for src in (a, b):
            if src:
                rows.append(src.pop(len(src) // 2))
    res = receive.open_objects([r[0] for r in rows], [r[2] for r in rows], [r[3] for r in rows], [r[4] for r in rows])
    assert len(res) == len(own) + len(ident_rows)
    seen = set()
    owner_ripe = next(r[4] for r in ident_rows if r[0] == PUBKEY_V4 and r[1]['name'] == 'valid')
    for i, (kind, e, _obj, _plain, _expect) in enumerate(rows):
        rec = res.recs[i]
        seen.add((kind, int(rec['status'])))
        ok = int(rec['status']) == receive.OBJ_OK
        if 'record' in e:  # rxobj_kats.json
            check_row_against_fixture(kind, e, res, i, final=True)
            assert int(rec['digest']) == e['digest'], e['name']
            if e['result'] is not None:
                assert (res.fromAddress(i), res.ripe(i).hex()) == (e['result']['fromAddress'], e['result']['ripe']), e['name']
                if kind == BROADCAST:
                    assert res.sigHash(i).hex() == e['result']['sigHash'], e['name']
                else:
                    assert res.storedData(i).hex() == e['result']['storedData'] and res.sigHash(i) == bytes(32), e['name']
        elif kind == BROADCAST:  # ident_kats.json
            assert int(rec['status']) == LINE_STATUS[kind][e['line']], e['name']
            if e['result'] is not None:
                got = {'fromAddress': res.fromAddress(i), 'ripe': res.ripe(i).hex(), 'sigHash': res.sigHash(i).hex()}
                assert got == e['result'] and res.signedData(i).hex() == e['parts']['signedData'], e['name']
        else:
            # what decides before the decryption is the wrapper's; here every row has its plaintext and the ripe of
            # the address given, so those rows go by their signature and keys
            line = e['line']
            if line in (423, 428, 442, 457):  # these rows carry the keys and the signature of the `valid` row's owner
                line = None if _expect == owner_ripe else 497
            assert int(rec['status']) == LINE_STATUS[kind][line], e['name']
            if ok:
                assert res.storedData(i).hex() == e['parts']['storedData'], e['name']
        if not ok:
            assert rec['ripe'].tobytes() == bytes(20) and rec['sig_hash'].tobytes() == bytes(32) and rec['addr_len'] == 0
            assert int(rec['digest']) == 0
    # every status of every kind the device can set
    assert seen == {(k, s) for k in (BROADCAST, PUBKEY_V4, PUBKEY) for s in receive.OBJ_STATUS_LINES[k] if s < 14}



def test_wrappers_on_their_own_fixture(gpulib, kats):
    """Objects alone, with the subscriptions and the needed pubkeys: a status for every object, the fixture's."""
    from pybitmessage_amd import receive
    objs = [bytes.fromhex(e['obj']) for e in kats['broadcasts']]
    res = receive.open_broadcasts(objs, kats['subscriptions'])
    old = receive.process_broadcasts(objs, kats['subscriptions'])
    for i, e in enumerate(kats['broadcasts']):
        assert int(res.status[i]) == LINE_STATUS[BROADCAST][e['line']], e['name']
        assert (old[i] is None) == (e['line'] is not None), e['name']
        if e['plaintext'] is not None:
            assert res.plaintexts[i].hex() == e['plaintext']
            check_row_against_fixture(BROADCAST, e, res, i, final=True)
        if old[i] is not None:
            assert_same_broadcast(res, i, old[i])
    pk = kats['pubkeys_v4'] + kats['pubkeys']
    objs = [bytes.fromhex(e['obj']) for e in pk]
    needed = {bytes.fromhex(t): a for t, a in kats['needed'].items()}
    res = receive.open_pubkeys(objs, needed)
    n4 = len(kats['pubkeys_v4'])
    old = receive.check_pubkeys_v4(objs[:n4], [e['address'] or kats['pubkeys_v4'][0]['address'] for e in kats['pubkeys_v4']])
    for i, e in enumerate(pk):
        kind = PUBKEY_V4 if i < n4 else PUBKEY
        line = e['line']
        if kind == PUBKEY and line == 410:
            line, kind = 411, PUBKEY_V4  # the wrapper routes it: a clear pubkey's 233 bytes are below :411's floor
        if e['record'] is None:
            kind = PUBKEY  # a header varint raises before the version is known
        assert int(res.status[i]) == LINE_STATUS[kind][line] and int(res.kind[i]) == kind, e['name']
        if e['result'] is not None:
            assert (res.fromAddress(i), res.ripe(i).hex(), res.storedData(i).hex()) == \
                (e['result']['fromAddress'], e['result']['ripe'], e['result']['storedData']), e['name']
        if i < n4:
            assert (old[i] is None) == (e['line'] is not None), e['name']
            if old[i] is not None:
                assert res.storedData(i) == old[i]
    assert res.accepted() == [i for i, e in enumerate(pk) if e['line'] is None]


def assert_same_broadcast(res, i, old):
    assert (res.signedData(i), res.signature(i), res.message(i), res.pubkeyData(i)) == \
        (old.signedData, old.signature, old.message, old.pubkeyData)
    assert (int(res.senderVersion[i]), int(res.senderStream[i]), int(res.encoding[i])) == \
        (old.senderVersion, old.senderStream, old.encoding)
    assert (res.fromAddress(i), res.ripe(i), res.sigHash(i)) == (old.fromAddress, old.ripe, old.sigHash)
    assert old.pubSigningKey64 + old.pubEncryptionKey64 in res.pubkeyData(i)


def test_wrappers_equal_the_old_functions_on_the_identification_fixture(gpulib, ident_kats):
    """``None`` <=> status != OK, the fields equal where accepted, and the status the fixture's line."""
    from pybitmessage_amd import receive, signatures
    subs = [s['address'] for s in ident_kats['subscriptions']]
    objs = [bytes.fromhex(b['obj']) for b in ident_kats['broadcasts']]
    res, old = receive.open_broadcasts(objs, subs), receive.process_broadcasts(objs, subs)
    assert len(res) == len(old) == 50
    for i, b in enumerate(ident_kats['broadcasts']):
        assert (old[i] is None) == (res.status[i] != receive.OBJ_OK), b['name']
        assert int(res.status[i]) == LINE_STATUS[BROADCAST][b['line']], b['name']
        if old[i] is not None:
            assert_same_broadcast(res, i, old[i])
    # one call per address asked for: its rows' tags are what neededPubkeys holds for it
    by_address = {}
    for k in ident_kats['pubkeys_v4']:
        by_address.setdefault(k['address'], []).append(k)
    for address, group in by_address.items():
        objs = [bytes.fromhex(k['obj']) for k in group]
        needed = {}
        for k, o in zip(group, objs):
            head = signatures.pubkey_v4_header(o)
            if head is not None:
                needed[head[2]] = address
        res, old = receive.open_pubkeys(objs, needed), receive.check_pubkeys_v4(objs, [address] * len(objs))
        for i, k in enumerate(group):
            assert (old[i] is None) == (res.status[i] != receive.OBJ_OK), k['name']
            # :442: the entry under the object's tag is for another address.  An object that says version 5 never
            # gets to decryptAndCheckPubkeyPayload's :423: processpubkey returns at :287
            want = receive.OBJ_ADDRESS_VERSION if k['name'] == 'object_version_5' else LINE_STATUS[PUBKEY_V4][k['line']]
            if len(objs[i]) < 350 and k['name'] != 'version_varint_not_minimal':  # the cut plaintexts: below processpubkey's :411
                want = receive.OBJ_V4_TOO_SHORT
            assert int(res.status[i]) == want, k['name']
            if old[i] is not None:
                assert res.storedData(i) == old[i] == bytes.fromhex(k['storedData']) and res.fromAddress(i) == address


def test_padding_boundary_under_every_prefix_length(gpulib, senders):
    """Signed lengths congruent to 55, 56, 63, 0 and 1 mod 64 -- either side of the byte that takes one more
    block for the padding, and of the block edge -- under each prefix length: 14, 16, 18, 22 (v4 broadcasts),
    46, 48, 50, 54 (v5 broadcasts and encrypted pubkeys) and 0 with the source read from byte 8 (clear
    pubkeys).  A broadcast's message sets its length freely.  A pubkey's signed data has no free field: its
    length is 177 (encrypted) or 145 (clear) plus three minimal varints of 1, 3, 5 or 9 bytes, an even number,
    so of the five residues 56 and 0 can be met (184 and 192 bytes) and only by an encrypted one; for clear
    pubkeys every reachable length 148 .. 172 is taken instead."""
    from pybitmessage_amd import receive
    value = {1: 7, 3: 300, 5: 70000, 9: 2 ** 32}
    rows, want_len = [], []
    for bv, fixed in ((4, 12 + 1 + 1 + 4 + 128 + 3 + 3 + 1), (5, 12 + 1 + 32 + 1 + 4 + 128 + 3 + 3 + 1)):
        for stream in STREAMS:
            width = {7: 1, 300: 3, 70000: 5, 2 ** 32: 9}[stream]
            for length in (247, 248, 255, 256, 257, 311, 312, 319, 320, 321):
                m = length - fixed - 2 * width
                m -= 1 if m - 1 < 253 else 3  # the message length's own varint
                rows.append(row(len(rows), BROADCAST, bv=bv, stream=stream, message=bytes((length + k) & 0xff for k in range(m)),
                                alg='sha1' if len(rows) % 2 else 'sha256'))
                want_len.append(length)
    for s, n, e in ((1, 1, 5), (1, 3, 3), (3, 3, 1), (5, 1, 1), (1, 5, 9), (3, 9, 3), (9, 3, 3), (5, 5, 5), (9, 9, 9)):
        rows.append(row(len(rows), PUBKEY_V4, stream=value[s], ntpb=value[n], extra=value[e], alg='sha1' if n == 3 else 'sha256'))
        want_len.append(177 + s + n + e)
    for s in (1, 3, 5, 9):
        for n in (1, 3, 5, 9):
            for e in (1, 9):
                rows.append(row(len(rows), PUBKEY, stream=value[s], ntpb=value[n], extra=value[e], alg='sha1' if n == 5 else 'sha256'))
                want_len.append(145 + s + n + e)
    made, signed = compose(rows, senders)
    assert [len(s) for s in signed] == want_len
    assert {184, 192} <= {n for n, r in zip(want_len, rows) if r['kind'] == PUBKEY_V4}
    assert {n for n, r in zip(want_len, rows) if r['kind'] == PUBKEY} == set(range(148, 173, 2)) - {170}
    res = open_rows(made)
    assert res.status.tolist() == [receive.OBJ_OK] * len(rows)
    assert res.digest.tolist() == [1 if r['alg'] == 'sha1' else 2 for r in rows]
    assert [int(res.recs[i]['prefix_len']) + int(res.recs[i]['bottom']) for i in range(len(rows))] == want_len
    assert [res.signedData(i) for i in range(len(rows))] == signed
    assert {int(res.recs[i]['prefix_len']) for i in range(len(rows))} == {0, 14, 16, 18, 22, 46, 48, 50, 54}
    # the last signed byte decides too
    flipped = []
    for (kind, obj, plain, expect), s in zip(made, signed):
        if kind == PUBKEY:
            at = 8 + len(s) - 1
            flipped.append((kind, obj[:at] + bytes([obj[at] ^ 0x40]) + obj[at + 1:], None, None))
        else:
            at = len(s) - (len(obj) - len(b'encrypted payload') - 8) - 1
            flipped.append((kind, obj, plain[:at] + bytes([plain[at] ^ 0x40]) + plain[at + 1:], expect))
    res = open_rows(flipped)
    assert res.status.tolist() == [receive.OBJ_BAD_SIGNATURE] * len(rows)
    assert res.digest.tolist() == [0] * len(rows)


@pytest.fixture(scope='module')
def alone(gpulib, kats):
    """Every device row of the fixture, and its record when it is submitted by itself."""
    from pybitmessage_amd import receive
    rows = device_rows(kats)
    return rows, [receive.open_objects([k], [o], [p], [x]).recs.tobytes() for k, _e, o, p, x in rows]


@pytest.mark.parametrize('n', [1, 63, 64, 65, 129])
def test_row_counts_and_interleaved_rejects(gpulib, alone, n):
    """Rejected rows of every status and kind sit between accepted ones inside one wave; each row's record is
    what the row gives alone, so neither the dummy rows, nor the lanes past n, nor the stride's rounding leak."""
    from pybitmessage_amd import receive
    rows, records = alone
    ok = [i for i, r in enumerate(rows) if r[1]['line'] is None]
    bad = [i for i, r in enumerate(rows) if r[1]['line'] is not None]
    assert {(rows[i][0], LINE_STATUS[rows[i][0]][rows[i][1]['line']]) for i in bad} == \
        {(k, s) for k in (BROADCAST, PUBKEY_V4, PUBKEY) for s in receive.OBJ_STATUS_LINES[k] if 0 < s < 14}
    pick = [(ok[(k // 2) % len(ok)] if k % 2 == 0 else bad[(k // 2) % len(bad)]) for k in range(n)]
    res = receive.open_objects([rows[i][0] for i in pick], [rows[i][2] for i in pick], [rows[i][3] for i in pick],
                               [rows[i][4] for i in pick])
    for k, i in enumerate(pick):
        assert res.recs[k].tobytes() == records[i], (k, rows[i][1]['name'])


def mixed_rows(count, seed, senders, spoil, sizes=(0, 1, 7, 60, 200, 200, 2000, None)):
    rng = random.Random(seed)
    rows = []
    for k in range(count):
        kind = rng.choice((BROADCAST, BROADCAST, PUBKEY_V4, PUBKEY))
        size = rng.choice(sizes)
        size = rng.randrange(20000) if size is None else size
        rows.append(row(k, kind, bv=rng.choice((4, 5)), stream=rng.choice((1, 1, 300, 70000, 2 ** 33)),
                        message=bytes([k & 0xff]) * size, ntpb=rng.choice((1, 1000, 70000)), extra=rng.choice((1, 1000, 2 ** 32)),
                        alg=rng.choice(('sha1', 'sha256'))))
    made, _signed = compose(rows, senders)
    spoiled = 0
    for k in range(count):
        if rng.random() >= spoil:
            continue
        spoiled += 1
        kind, obj, plain, expect = made[k]
        src, how = bytearray(obj if kind == PUBKEY else plain), rng.randrange(5)
        if how == 0:
            # a clear pubkey's version byte is left alone: as version 2 it is accepted, and has no extractor to compare with
            src[rng.randrange(21 if kind == PUBKEY else 0, len(src))] ^= 1 << rng.randrange(8)
        elif how == 1:
            src[rng.randrange(130, min(len(src), 185))] = rng.choice((0, 253, 254, 255))
        elif how == 2:
            del src[rng.randrange(len(src)):]
        elif how == 3 and kind != PUBKEY:
            expect = bytes(20)
        elif kind != PUBKEY:
            obj = obj[:22] + bytes([obj[22] ^ 1]) + obj[23:]  # the stream number, or the tag behind it
        if kind == PUBKEY:
            obj = bytes(src)
        else:
            plain = bytes(src)
        made[k] = (kind, obj, plain, expect)
    return made, spoiled


def test_equals_the_composition_on_mixed_rows(gpulib, senders):
    """2,000 seeded rows of the three kinds, 150 B to 20 KB, about one in ten spoiled at a random field, against
    the extractors -> verify_batch_digest -> derive_batch -> comparisons and hashlib on the same device."""
    made, spoiled = mixed_rows(2000, 20251024, senders, 0.1)
    assert 150 < spoiled < 260
    res = open_rows(made)
    want, bad_signature = assert_equals_composition(res, made)
    assert sum(w is not None for w in want) > 1700 and len(bad_signature) > 20
    assert {int(k) for k in res.kind[res.accepted()]} == {BROADCAST, PUBKEY_V4, PUBKEY}
    assert len(set(res.status.tolist())) >= 6


@pytest.fixture(scope='module')
def distinct(gpulib, senders):
    """128 distinct signed rows of the three kinds, a few of them spoiled, and what one call gives them."""
    from pybitmessage_amd import receive
    made, _ = mixed_rows(128, 7, senders, 0.15, sizes=(0, 1, 7, 60, 200))
    res = open_rows(made)
    assert_equals_composition(res, made)
    status = np.stack([res.status, res.digest, res.kind], axis=1)
    assert receive.OBJ_OK in res.status and len(set(res.status.tolist())) >= 3 and sorted(set(res.digest.tolist())) == [0, 1, 2]
    return made, status, res.recs.tobytes()


def test_two_sets(gpulib, distinct):
    from pybitmessage_amd import receive
    made, status, _ = distinct
    n = SET + 65
    idx = np.arange(n) % 128
    receive.obj_reset_stats()
    receive.reset_stats()
    res = open_rows([made[i] for i in idx])
    st = receive.obj_stats()
    assert (st['calls'], st['rows'], st['sets'], st['launches']) == (1, n, 2, 18)
    assert np.array_equal(np.stack([res.status, res.digest, res.kind], axis=1), status[idx])
    assert all(st[k] > 0 for k in ('walk_ms', 'hash_ms', 'scalar_ms', 'curve_ms', 'ident_ms', 'finish_ms', 'host_ms'))
    msgs = receive.stats()  # the msgs' counters are theirs alone
    assert (msgs['calls'], msgs['rows'], msgs['sets'], msgs['launches']) == (0, 0, 0, 0)


def test_abort_and_empty_input(gpulib, distinct):
    from pybitmessage_amd import _lib, receive
    made, status, records = distinct
    idx = np.arange(SET + 1) % 128
    rows = [made[i] for i in idx]
    gpulib.bmpow_abort()
    try:
        with pytest.raises(_lib.BmpowError) as e:
            open_rows(rows)
        assert e.value.code == _lib.E_ABORTED
    finally:
        gpulib.bmpow_clear_abort()
    assert open_rows(made).recs.tobytes() == records
    receive.obj_reset_stats()
    assert len(receive.open_objects([], [], [], [])) == 0
    rec = np.zeros(1, dtype=receive.OBJ_REC)
    assert gpulib.bmpow_rx_objects(0, None, None, None, None, None, None, rec.ctypes.data) == 0
    st = receive.obj_stats()
    assert (st['calls'], st['rows'], st['sets'], st['launches']) == (0, 0, 0, 0)


def test_msgs_are_unchanged_in_the_same_process(gpulib, distinct):
    """After object calls in this process ``open_msgs`` still gives its own fixture, and each side counts its own."""
    from pybitmessage_amd import receive
    from tests.test_rx import LINE_STATUS as MSG_LINE_STATUS
    made, _status, records = distinct
    assert open_rows(made).recs.tobytes() == records
    msgs = [m for m in load_golden('rx_kats.json')['msgs'] if m['line'] != 478]
    receive.reset_stats()
    receive.obj_reset_stats()
    res = receive.open_msgs([bytes.fromhex(m['obj']) for m in msgs], [bytes.fromhex(m['plaintext']) for m in msgs],
                            [bytes.fromhex(m['toRipe']) for m in msgs])
    assert res.status.tolist() == [MSG_LINE_STATUS[m['line']] for m in msgs]
    for i, m in enumerate(msgs):
        assert int(res.digest[i]) == m['digest'], m['name']
        if m['result'] is not None:
            assert {'fromAddress': res.fromAddress(i), 'ripe': res.ripe(i).hex(), 'sigHash': res.sigHash(i).hex()} == m['result']
    assert receive.stats()['rows'] == len(msgs) and receive.obj_stats()['rows'] == 0
    assert open_rows(made).recs.tobytes() == records
