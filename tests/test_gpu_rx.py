"""Msg processing on the GPU (include/bmpow_rx.h, pybitmessage_amd/receive.py: open_msgs, process_msgs) against
tests/golden/rx_kats.json, which tests/test_rx.py pins to the reference, and against the composition the
library offered before (``signatures.msg_signed_parts`` per object, ``verify_batch_digest``,
``receive.identify``, hashlib).  Everything is bit-exact."""
import hashlib
import random

import numpy as np
import pytest

from tests.conftest import load_golden
from tests.test_rx import LINE_STATUS, check_row_against_fixture

pytestmark = pytest.mark.gpu

SET = 1 << 18  # rows of one launch set


@pytest.fixture(scope='module')
def kats():
    return load_golden('rx_kats.json')


@pytest.fixture(scope='module')
def fixture_rows(kats):
    """(fixture entry, obj, plaintext, toRipe) of every msg some key decrypts or the header refuses."""
    return [(m, bytes.fromhex(m['obj']), bytes.fromhex(m['plaintext']), bytes.fromhex(m['toRipe']))
            for m in kats['msgs'] if m['line'] != 478]


@pytest.fixture(scope='module')
def senders(gpulib):
    """Eight key pairs: (priv_signing, pub_signing64, pub_encryption64)."""
    from pybitmessage_amd import sender
    rng = random.Random(11)
    privs = [bytes(rng.randrange(1, 256) for _ in range(32)) for _ in range(16)]
    pubs = sender.priv_to_pub(privs)
    return [(privs[2 * i], pubs[2 * i][1:], pubs[2 * i + 1][1:]) for i in range(8)]


def compose(rows, senders):
    """Signed msgs made on the device.  rows: dicts with claimed, version, inner, sender (index), to_ripe,
    message, ack, alg, seed; gives (obj, plaintext) per row."""
    from pybitmessage_amd import sender
    from pybitmessage_amd.addressgen import encodeVarint as ev
    heads, bodies = [], []
    for r in rows:
        rng = random.Random(r['seed'])
        head = bytes(rng.randrange(256) for _ in range(16)) + b'\x00\x00\x00\x02' + ev(1) + ev(r['claimed'])
        _, pub_s, pub_e = senders[r['sender']]
        body = ev(r['version']) + ev(r['inner']) + b'\x00\x00\x00\x01' + pub_s + pub_e
        if r['version'] >= 3:
            body += ev(1000) + ev(1000)
        body += r['to_ripe'] + ev(2) + ev(len(r['message'])) + r['message'] + ev(len(r['ack'])) + r['ack']
        heads.append(head)
        bodies.append(body)
    signed = [h[8:20] + ev(1) + ev(r['claimed']) + b for h, r, b in zip(heads, rows, bodies)]
    sigs = [None] * len(rows)
    for alg in ('sha1', 'sha256'):
        idx = [i for i, r in enumerate(rows) if r['alg'] == alg]
        for i, s in zip(idx, sender.sign_batch([signed[i] for i in idx], [senders[rows[i]['sender']][0] for i in idx], alg)):
            assert s is not None
            sigs[i] = s
    return [(h + b'encrypted payload', b + ev(len(s)) + s) for h, b, s in zip(heads, bodies, sigs)], signed


def row(seed, **kw):
    r = {'claimed': 1, 'version': 4, 'inner': 1, 'sender': seed % 8, 'to_ripe': hashlib.sha1(b'me').digest(),
         'message': b'Subject:s\nBody:b', 'ack': b'', 'alg': 'sha256', 'seed': seed}
    r.update(kw)
    return r


def test_fixture_in_one_call(gpulib, kats, fixture_rows):
    from pybitmessage_amd import receive
    res = receive.open_msgs([r[1] for r in fixture_rows], [r[2] for r in fixture_rows], [r[3] for r in fixture_rows])
    assert len(res) == len(fixture_rows)
    for i, (m, _obj, _plain, _ripe) in enumerate(fixture_rows):
        check_row_against_fixture(m, res, i, final=True)
        assert int(res.digest[i]) == m['digest'], m['name']
        if m['result'] is not None:
            got = {'fromAddress': res.fromAddress(i), 'ripe': res.ripe(i).hex(), 'sigHash': res.sigHash(i).hex()}
            assert got == m['result'], m['name']
        else:
            assert res.recs[i]['ripe'].tobytes() == bytes(20) and res.recs[i]['sig_hash'].tobytes() == bytes(32)
    assert res.accepted() == [i for i, r in enumerate(fixture_rows) if r[0]['line'] is None]
    # ... and from the objects alone, with the recipients' keys
    keys = {bytes.fromhex(k['ripe']): bytes.fromhex(k['privkey']) for k in kats['recipients']}
    out = receive.process_msgs([bytes.fromhex(m['obj']) for m in kats['msgs']], keys)
    for m, got in zip(kats['msgs'], out):
        assert (got is None) == (m['line'] is not None), m['name']
        if got is None:
            continue
        assert got.toRipe.hex() == m['toRipe'] and got.digest == m['digest']
        assert {'fromAddress': got.fromAddress, 'ripe': got.ripe.hex(), 'sigHash': got.sigHash.hex()} == m['result']
        rec = m['record']
        assert (got.senderVersion, got.senderStream, got.encoding) == (rec['senderVersion'], rec['senderStream'], rec['encoding'])
        assert (got.message.hex(), got.ackData.hex(), got.signature.hex()) == (rec['message'], rec['ackData'], rec['signature'])
        assert got.pubkeyData.hex() == m['plaintext'][:2 * rec['endOfThePublicKeyPosition']]
        assert (got.behaviour.hex(), got.nonceTrialsPerByte, got.extraBytes) == (rec['behaviour'], rec['nonceTrialsPerByte'], rec['extraBytes'])


def test_padding_boundary_under_every_prefix_width(gpulib, senders):
    """Signed lengths 236 .. 260 cross the 247 / 248 edge where the padding takes one more block, under each of
    the four misalignments of the plaintext against the block pool."""
    from pybitmessage_amd import receive
    rows, want_len = [], []
    for claimed, prefix in ((7, 14), (300, 16), (70000, 18), (2 ** 32, 22)):
        for length in range(236, 261):
            m = length - prefix - 164  # a v4 sender's fields take 163 bytes, the one-byte ackData one more
            rows.append(row(len(rows), claimed=claimed, message=bytes((length + k) & 0xff for k in range(m)), ack=b'\xa5',
                            alg='sha1' if len(rows) % 2 else 'sha256'))
            want_len.append(length)
    assert len(rows) == 100
    msgs, signed = compose(rows, senders)
    assert [len(s) for s in signed] == want_len
    ripes = [r['to_ripe'] for r in rows]
    res = receive.open_msgs([o for o, _ in msgs], [p for _, p in msgs], ripes)
    assert res.status.tolist() == [receive.OK] * 100
    assert res.digest.tolist() == [1 if r['alg'] == 'sha1' else 2 for r in rows]
    assert [int(res.recs[i]['prefix_len']) + int(res.recs[i]['bottom']) for i in range(100)] == want_len
    flipped = []
    for (o, p), s in zip(msgs, signed):
        at = len(s) - (13 + _varint_len(o)) - 1  # the last signed byte of the plaintext: the ackData byte
        assert p[at] == 0xa5
        flipped.append(p[:at] + b'\x5a' + p[at + 1:])
    res = receive.open_msgs([o for o, _ in msgs], flipped, ripes)
    assert res.status.tolist() == [receive.BAD_SIGNATURE] * 100
    assert res.digest.tolist() == [0] * 100


def _varint_len(obj):
    from pybitmessage_amd.ecies import _varint
    return _varint(obj[21:30])[1]


@pytest.fixture(scope='module')
def alone(gpulib, fixture_rows):
    """Every fixture row's record when it is submitted by itself."""
    from pybitmessage_amd import receive
    return [receive.open_msgs([o], [p], [r]).recs.tobytes() for _m, o, p, r in fixture_rows]


@pytest.mark.parametrize('n', [1, 63, 64, 65, 129])
def test_row_counts_and_interleaved_rejects(gpulib, fixture_rows, alone, n):
    """Rejected rows of every kind sit between accepted ones inside one wave; each row's record is what the
    row gives alone, so neither the dummy rows, nor the lanes past n, nor the stride's rounding leak."""
    from pybitmessage_amd import receive
    ok = [i for i, r in enumerate(fixture_rows) if r[0]['line'] is None]
    bad = [i for i, r in enumerate(fixture_rows) if r[0]['line'] is not None]
    assert {LINE_STATUS[fixture_rows[i][0]['line']] for i in bad} == {1, 3, 4, 5, 6, 7, 8, 9}
    pick = [(ok[(k // 2) % len(ok)] if k % 2 == 0 else bad[(k // 2) % len(bad)]) for k in range(n)]
    res = receive.open_msgs([fixture_rows[i][1] for i in pick], [fixture_rows[i][2] for i in pick],
                            [fixture_rows[i][3] for i in pick])
    for k, i in enumerate(pick):
        assert res.recs[k].tobytes() == alone[i], (k, fixture_rows[i][0]['name'])


def _end_of_pubkey(plain):
    from pybitmessage_amd.ecies import _varint
    ver = _varint(plain[:10])
    pos = ver[1] + _varint(plain[ver[1]:ver[1] + 10])[1] + 4 + 128
    if ver[0] >= 3:
        for _ in range(2):
            pos += _varint(plain[pos:pos + 10])[1]
    return pos


def test_equals_the_composition_on_mixed_rows(gpulib, senders):
    """2,000 seeded msgs of 170 B to 20 KB, about one in ten mutated, against msg_signed_parts ->
    verify_batch_digest -> identify -> hashlib on the same device."""
    from pybitmessage_amd import receive, signatures
    rng = random.Random(20251023)
    rows = []
    for k in range(2000):
        size = rng.choice((0, 1, 7, 60, 200, 200, 200, 2000, 2000, rng.randrange(20000)))
        rows.append(row(k, claimed=rng.choice((1, 1, 300, 70000, 2 ** 33)), version=rng.choice((2, 3, 4, 4)),
                        inner=rng.choice((1, 1, 9, 65536)), message=bytes([k & 0xff]) * size,
                        ack=bytes(rng.randrange(256) for _ in range(rng.choice((0, 0, 32, 300)))),
                        alg=rng.choice(('sha1', 'sha256'))))
    msgs, _signed = compose(rows, senders)
    objs, plains, ripes = [o for o, _ in msgs], [p for _, p in msgs], [r['to_ripe'] for r in rows]
    mutated = 0
    for k in range(2000):
        if rng.random() >= 0.1:
            continue
        mutated += 1
        p, kind = bytearray(plains[k]), rng.randrange(5)
        if kind == 0:
            p[rng.randrange(len(p))] ^= 1 << rng.randrange(8)
        elif kind == 1:
            p[rng.randrange(130, 175)] = rng.choice((0, 253, 254, 255))
        elif kind == 2:
            del p[rng.randrange(len(p)):]
        elif kind == 3:
            ripes[k] = bytes(20)
        else:
            objs[k] = objs[k][:20] + b'\x02' + objs[k][21:]
        plains[k] = bytes(p)
    assert 150 < mutated < 260
    res = receive.open_msgs(objs, plains, ripes)
    parts = [signatures.msg_signed_parts(o, p) for o, p in zip(objs, plains)]
    live = [k for k, p in enumerate(parts) if p is not None and len(p[2]) == 64
            and plains[k][_end_of_pubkey(plains[k]):][:20] == ripes[k]]
    verdicts = signatures.verify_batch_digest([parts[k][0] for k in live], [parts[k][1] for k in live], [parts[k][2] for k in live])
    good = [k for k, v in zip(live, verdicts) if v]
    who = receive.identify([parts[k] for k in good], [rows[k]['version'] for k in good], [rows[k]['inner'] for k in good])
    assert res.accepted() == good and len(good) > 1700
    digest = dict(zip(live, verdicts))
    for k, (address, ripe) in zip(good, who):
        assert (res.fromAddress(k), res.ripe(k)) == (address, ripe), k
        assert res.sigHash(k) == hashlib.sha512(hashlib.sha512(parts[k][1]).digest()).digest()[32:], k
        assert int(res.digest[k]) == digest[k] and res.signature(k) == parts[k][1]
        assert res.message(k) == rows[k]['message'] and res.ackData(k) == rows[k]['ack']
    bad_sig = [k for k in live if not digest[k]]
    assert [k for k in range(2000) if res.status[k] == receive.BAD_SIGNATURE] == bad_sig and bad_sig
    assert all(res.status[k] not in (receive.OK, receive.BAD_SIGNATURE) for k in range(2000) if k not in set(live))


@pytest.fixture(scope='module')
def distinct(gpulib, senders):
    """128 distinct signed msgs, a few of them spoiled, and their statuses one call gives them."""
    from pybitmessage_amd import receive
    rows = [row(k, claimed=(1, 300)[k % 2], message=bytes([k]) * (3 * k), alg=('sha1', 'sha256')[k % 2]) for k in range(128)]
    msgs, _ = compose(rows, senders)
    objs, plains = [o for o, _ in msgs], [p for _, p in msgs]
    for k in range(0, 128, 9):
        plains[k] = plains[k][:-2] + bytes([plains[k][-2] ^ 4]) + plains[k][-1:]
    ripes = [r['to_ripe'] for r in rows]
    ripes[5] = bytes(20)
    res = receive.open_msgs(objs, plains, ripes)
    status = np.stack([res.status, res.digest], axis=1)  # per row: the status and the digest it verified under
    assert sorted(set(res.status.tolist())) == [receive.OK, receive.WRONG_TO_RIPE, receive.BAD_SIGNATURE]
    assert sorted(set(res.digest.tolist())) == [0, 1, 2]
    return objs, plains, ripes, status


def test_two_sets(gpulib, distinct):
    from pybitmessage_amd import receive
    objs, plains, ripes, status = distinct
    n = SET + 65
    idx = np.arange(n) % 128
    receive.reset_stats()
    res = receive.open_msgs([objs[i] for i in idx], [plains[i] for i in idx], [ripes[i] for i in idx])
    st = receive.stats()
    assert (st['calls'], st['rows'], st['sets'], st['launches']) == (1, n, 2, 18)
    assert np.array_equal(np.stack([res.status, res.digest], axis=1), status[idx])
    assert all(st[k] > 0 for k in ('walk_ms', 'hash_ms', 'scalar_ms', 'curve_ms', 'ident_ms', 'finish_ms', 'host_ms'))


def test_abort_and_empty_input(gpulib, distinct):
    from pybitmessage_amd import _lib, receive
    objs, plains, ripes, status = distinct
    idx = np.arange(SET + 1) % 128
    args = ([objs[i] for i in idx], [plains[i] for i in idx], [ripes[i] for i in idx])
    gpulib.bmpow_abort()
    try:
        with pytest.raises(_lib.BmpowError) as e:
            receive.open_msgs(*args)
        assert e.value.code == _lib.E_ABORTED
    finally:
        gpulib.bmpow_clear_abort()
    res = receive.open_msgs(objs, plains, ripes)
    assert np.array_equal(np.stack([res.status, res.digest], axis=1), status)
    receive.reset_stats()
    assert len(receive.open_msgs([], [], [])) == 0
    rec = np.zeros(1, dtype=receive.MSG_REC)
    assert gpulib.bmpow_rx_msgs(0, None, None, None, None, None, rec.ctypes.data) == 0
    st = receive.stats()
    assert (st['calls'], st['rows'], st['sets'], st['launches']) == (0, 0, 0, 0)


def test_neighbours_are_unchanged_in_the_same_process(gpulib, distinct):
    """The signature unit's buffers and set limits moved into a header this unit shares; after msg calls in this
    process its answers and the identification's are still the fixtures'."""
    from pybitmessage_amd import addresses, receive, signatures
    objs, plains, ripes, status = distinct
    assert np.array_equal(receive.open_msgs(objs, plains, ripes).status, status[:, 0])
    cases = load_golden('sig_kats.json')['cases']
    got = signatures.verify_batch_digest([bytes.fromhex(c['msg']) for c in cases], [bytes.fromhex(c['sig']) for c in cases],
                                         [bytes.fromhex(c['key']) for c in cases])
    assert got == [c['code'] for c in cases]
    assert signatures.verify_batch([bytes.fromhex(c['msg']) for c in cases], [bytes.fromhex(c['sig']) for c in cases],
                                   [bytes.fromhex(c['key']) for c in cases]) == [c['verdict'] for c in cases]
    keys = load_golden('ident_kats.json')['keys']
    ident = addresses.derive_batch([bytes.fromhex(k['pub_signing']) for k in keys],
                                   [bytes.fromhex(k['pub_encryption']) for k in keys], [4] * len(keys), [1] * len(keys))
    for i, k in enumerate(keys):
        assert ident.ripe[i].tobytes().hex() == k['ripe']
        assert ident.address(i) == addresses.encodeAddress(4, 1, bytes.fromhex(k['ripe']))
    assert np.array_equal(receive.open_msgs(objs, plains, ripes).status, status[:, 0])
