"""The one-call opening of received msgs on the GPU (include/bmpow_rxopen.h, pybitmessage_amd/receive.py:
open_sealed_msgs, process_sealed_msgs) against tests/golden/rx_kats.json, which tests/test_rx.py pins to the
reference, and against the composition of calls it replaces (``ecies.process_msgs``: ``bmpow_ecies_match`` and
``bmpow_aes256_cbc``; then ``receive.open_msgs``: ``bmpow_rx_msgs``).  Everything is bit-exact."""
import ctypes
import hashlib
import hmac
import random

import numpy as np
import pytest

from tests.conftest import load_golden
from tests.test_gpu_rx import compose, row
from tests.test_rx import LINE_STATUS, check_row_against_fixture
from tests.test_rxobj import BROADCAST

pytestmark = pytest.mark.gpu

SET = 1 << 18  # objects of one ECIES set
TAIL = len(b'encrypted payload')  # what compose() puts where the payload goes
ROW_UP, ROW_DOWN = 80 + 16, 208 + 4  # a matched row's descriptors (rx_row, rxs_row); its record and opened[]


@pytest.fixture(scope='module')
def kats():
    return load_golden('rx_kats.json')


@pytest.fixture(scope='module')
def senders(gpulib):
    from pybitmessage_amd import sender
    rng = random.Random(11)
    privs = [bytes(rng.randrange(1, 256) for _ in range(32)) for _ in range(16)]
    pubs = sender.priv_to_pub(privs)
    return [(privs[2 * i], pubs[2 * i][1:], pubs[2 * i + 1][1:]) for i in range(8)]


@pytest.fixture(scope='module')
def user(gpulib):
    """Three encryption key pairs and the ripes they go by: (privs, pubs64, ripes).  The tests hold the first
    two; the third is somebody else's."""
    from pybitmessage_amd import sender
    rng = random.Random(5)
    privs = [bytes(rng.randrange(1, 256) for _ in range(32)) for _ in range(3)]
    pubs = [p[1:] for p in sender.priv_to_pub(privs)]
    return privs, pubs, [hashlib.sha1(b'ripe of key %d' % i).digest() for i in range(3)]


def seal(msgs, pubkeys, seed, ephemeral=None):
    """compose()'s (obj, plaintext) pairs as wire objects: each plaintext sealed to its key, fixed ephemerals."""
    from pybitmessage_amd import sender
    rng = random.Random(seed)
    eph = ephemeral or [bytes(rng.randrange(1, 256) for _ in range(32)) for _ in msgs]
    ivs = [bytes(rng.randrange(256) for _ in range(16)) for _ in msgs]
    blobs = sender.encrypt_batch([p for _, p in msgs], pubkeys, ephemeral=eph, ivs=ivs)
    assert all(b is not None for b in blobs)
    return [o[:-TAIL] + b for (o, _), b in zip(msgs, blobs)]


def split_blob(blob):
    """(iv || curve, X, Y, ciphertext, mac) of an ECIES blob."""
    xl = int.from_bytes(blob[18:20], 'big')
    yl = int.from_bytes(blob[20 + xl:22 + xl], 'big')
    return blob[:18], blob[20:20 + xl], blob[22 + xl:22 + xl + yl], blob[22 + xl + yl:-32], blob[-32:]


def keys_of(priv, X, Y):
    """(key_e, key_m) of ``ECC.decrypt``: SHA-512 of the shared x."""
    from pybitmessage_amd import ecies
    h = hashlib.sha512(ecies.ecdh([priv], [(X, Y)])[0]).digest()
    return h[:32], h[32:]


def blob_of(front, X, Y, cipher, priv, zx=0, zy=0):
    """A blob whose coordinates carry zx / zy extra leading zero bytes, MACed for the holder of priv."""
    body = (front + (len(X) + zx).to_bytes(2, 'big') + bytes(zx) + X + (len(Y) + zy).to_bytes(2, 'big') + bytes(zy) + Y +
            cipher)
    return body + hmac.new(keys_of(priv, X, Y)[1], body, hashlib.sha256).digest()


def composition(objs, ripes, privs):
    """What the library offered before: (opened, live, records of the live rows)."""
    from pybitmessage_amd import ecies, receive
    opened = ecies.process_msgs(objs, dict(zip(ripes, privs)))
    live = [i for i, r in enumerate(opened) if r is not None]
    res = receive.open_msgs([objs[i] for i in live], [opened[i][1] for i in live], [opened[i][0] for i in live])
    return opened, live, res


def assert_equals_composition(objs, ripes, privs):
    """Every row of open_sealed_msgs against ecies.process_msgs + open_msgs, byte for byte; gives the batch."""
    from pybitmessage_amd import ecies, receive
    got = receive.open_sealed_msgs(objs, (ripes, privs))
    assert len(got) == len(objs)
    opened, live, res = composition(objs, ripes, privs)
    payloads = [ecies.msg_payload(o) for o in objs]
    matches = ecies.match_keys([p or b'' for p in payloads], privs) if privs else [None] * len(objs)
    for j, i in enumerate(live):
        assert got.recs[i].tobytes() == res.recs[j].tobytes(), i
        assert got.plaintexts[i] == opened[i][1], i
        assert got.toRipe(i) == opened[i][0] and int(got.match[i]) == ripes.index(opened[i][0]), i
    alive = set(live)
    for i in range(len(objs)):
        if i in alive:
            continue
        assert got.plaintexts[i] == b'' and not got.recs[i]['ripe'].any() and not got.recs[i]['addr_len'], i
        if payloads[i] is None:
            assert int(got.status[i]) == receive.MSG_VERSION and int(got.match[i]) == -1, i
            assert got.recs[i].tobytes() == receive.walk_msg(objs[i], b'', bytes(20))[0].recs.tobytes(), i
        else:
            assert int(got.status[i]) == receive.NOT_MINE, i
            assert int(got.match[i]) == (-1 if matches[i] is None else matches[i]), i
            assert got.toRipe(i) == (None if matches[i] is None else ripes[matches[i]])
            only = np.zeros(1, dtype=receive.MSG_REC)
            only['status'], only['claimed_stream'], only['prefix_len'] = receive.NOT_MINE, got.claimedStream[i], got.recs[i]['prefix_len']
            assert got.recs[i].tobytes() == only.tobytes() and int(got.recs[i]['prefix_len']) in (14, 16, 18, 22), i
    return got


def check_msg_result(m, res, i):
    """Row i of a msg batch against the fixture's final record, digest and result."""
    check_row_against_fixture(m, res, i, final=True)
    assert int(res.digest[i]) == m['digest'], m['name']
    if m['result'] is not None:
        got = {'fromAddress': res.fromAddress(i), 'ripe': res.ripe(i).hex(), 'sigHash': res.sigHash(i).hex()}
        assert got == m['result'], m['name']
    else:
        assert res.recs[i]['ripe'].tobytes() == bytes(20) and res.recs[i]['sig_hash'].tobytes() == bytes(32)


def check_sealed_row(m, res, i):
    """Row i of open_sealed_msgs against the fixture: the record, and whose key opened it to what."""
    if m['line'] in (444, 478):
        check_row_against_fixture(m, res, i, final=True)
        assert int(res.digest[i]) == m['digest'], m['name']
        assert int(res.status[i]) == LINE_STATUS[m['line']] and int(res.match[i]) == -1, m['name']
        assert res.toRipe(i) is None and res.plaintexts[i] == b''
        return
    assert res.toRipe(i).hex() == m['toRipe'] and res.plaintexts[i].hex() == m['plaintext'], m['name']
    check_msg_result(m, res, i)


# ------------------------------------------------------------------ 1. the fixture
def test_fixture_in_one_call(gpulib, kats):
    from pybitmessage_amd import receive
    keys = {bytes.fromhex(k['ripe']): bytes.fromhex(k['privkey']) for k in kats['recipients']}
    objs = [bytes.fromhex(m['obj']) for m in kats['msgs']]
    res = receive.open_sealed_msgs(objs, keys)
    assert len(res) == len(objs)
    for i, m in enumerate(kats['msgs']):
        check_sealed_row(m, res, i)
    assert [m['name'] for m, s in zip(kats['msgs'], res.status) if s == receive.NOT_MINE] == ['not_mine']
    assert res.accepted() == [i for i, m in enumerate(kats['msgs']) if m['line'] is None]
    assert receive.process_sealed_msgs(objs, keys) == receive.process_msgs(objs, keys)
    assert_equals_composition(objs, list(keys), list(keys.values()))


# ------------------------------------------------------------------ 2. equals the composition
def test_equals_the_composition_on_mixed_rows(gpulib, senders, user):
    from pybitmessage_amd import receive
    privs, pubs, ripes = user
    rows, to = [], []
    for k, (version, alg, size) in enumerate((v, a, s) for v in (2, 3, 4) for a in ('sha1', 'sha256') for s in (0, 1, 200, 2000)):
        rows.append(row(k, version=version, alg=alg, message=bytes([k]) * size, to_ripe=ripes[k % 2],
                        claimed=(1, 300, 70000)[k % 3], ack=bytes(range(k % 5))))
        to.append(k % 2)
    base = len(rows)
    rows += [row(100, to_ripe=ripes[0], message=b'spoiled below'), row(101, to_ripe=ripes[1], message=b'for my other address'),
             row(102, to_ripe=ripes[2], message=b'for somebody else' * 9), row(103, to_ripe=ripes[2], alg='sha1')]
    to += [0, 0, 2, 2]
    msgs, _ = compose(rows, senders)
    spoiled = bytearray(msgs[base][1])
    spoiled[spoiled.index(b'spoiled below')] ^= 0x20
    msgs[base] = (msgs[base][0], bytes(spoiled))
    objs = seal(msgs, [pubs[t] for t in to], seed=1)
    got = assert_equals_composition(objs, ripes[:2], privs[:2])
    assert got.status[:base].tolist() == [receive.OK] * base
    assert got.status[base:].tolist() == [receive.BAD_SIGNATURE, receive.WRONG_TO_RIPE, receive.NOT_MINE, receive.NOT_MINE]
    assert got.match.tolist() == to[:base] + [0, 0, -1, -1]
    assert got.digest[:base].tolist() == [1 if r['alg'] == 'sha1' else 2 for r in rows[:base]]
    assert [got.message(i) for i in range(base)] == [r['message'] for r in rows[:base]]
    assert receive.process_sealed_msgs(objs, dict(zip(ripes[:2], privs[:2]))) == \
        receive.process_msgs(objs, dict(zip(ripes[:2], privs[:2])))


# ------------------------------------------------------------------ 3. every ciphertext alignment
def test_every_ciphertext_alignment(gpulib, senders, user):
    """One msg under heads of every length mod 16: the coordinates re-encoded with leading zero bytes (legal:
    they are reduced mod p) and MACed again, and ephemeral points whose X or Y has 31 bytes as the sender's own
    seal writes them."""
    from pybitmessage_amd import receive, sender
    privs, pubs, ripes = user
    msgs, _ = compose([row(7, to_ripe=ripes[0], message=b'aligned ' * 30)], senders)
    rng = random.Random(31)
    cands = [bytes(rng.randrange(1, 256) for _ in range(32)) for _ in range(4096)]
    points = sender.priv_to_pub(cands)
    short_x = next(c for c, p in zip(cands, points) if p[1] == 0 and p[33] != 0)
    short_y = next(c for c, p in zip(cands, points) if p[33] == 0 and p[1] != 0)
    base = seal(msgs, [pubs[0]], seed=2)[0]
    head, blob = base[:22], base[22:]  # nonce, time, type, version 1, stream 1
    front, X, Y, cipher, mac = split_blob(blob)
    assert (len(X), len(Y)) == (32, 32) and blob_of(front, X, Y, cipher, privs[0]) == blob  # the MAC is restated right
    objs = [head + blob_of(front, X, Y, cipher, privs[0], zx=z) for z in range(16)]
    objs += [head + blob_of(front, X, Y, cipher, privs[0], zx=3, zy=z) for z in (1, 6)]
    objs += seal(msgs * 2, [pubs[0]] * 2, seed=3, ephemeral=[short_x, short_y])
    plans = [receive.sealed_plan(o) for o in objs]
    assert all(p[0] for p in plans)
    assert {p[3] % 16 for p in plans[:16]} == set(range(16)) and [p[3] for p in plans[-2:]] == [85, 85]
    assert [len(split_blob(o[22:])[1]) for o in objs[-2:]] == [31, 32] and [len(split_blob(o[22:])[2]) for o in objs[-2:]] == [32, 31]
    got = assert_equals_composition(objs, ripes[:2], privs[:2])
    assert got.status.tolist() == [receive.OK] * len(objs)
    for i in range(len(objs)):
        assert got.recs[i].tobytes() == got.recs[0].tobytes() and got.plaintexts[i] == msgs[0][1], i


# ------------------------------------------------------------------ 4. padding
def crafted(user, seed, key=0):
    """(make, key_e, iv): make(cipher) is an object whose payload carries `cipher` as it stands under a MAC that
    verifies for user key `key`; key_e and iv are what that payload is opened with."""
    from pybitmessage_amd import sender
    privs, _pubs, _ripes = user
    rng = random.Random(seed)
    eph = bytes(rng.randrange(1, 256) for _ in range(32))
    iv = bytes(rng.randrange(256) for _ in range(16))
    R = sender.priv_to_pub([eph])[0][1:]
    X, Y = R[:32].lstrip(b'\x00'), R[32:].lstrip(b'\x00')
    head = bytes(rng.randrange(256) for _ in range(16)) + b'\x00\x00\x00\x02\x01\x01'
    make = lambda c: head + blob_of(iv + b'\x02\xca', X, Y, c, privs[key])  # noqa: E731
    return make, keys_of(privs[key], X, Y)[0], iv


def test_padding_on_both_sides_of_a_block(gpulib, senders, user):
    from pybitmessage_amd import ecies, receive
    privs, pubs, ripes = user
    msgs, _ = compose([row(9, to_ripe=ripes[1], version=3)], senders)
    whole = msgs[0][1]
    cut = [(msgs[0][0], whole[:n]) for n in range(170, 187)]  # 170 .. 186 bytes: pads of 6 .. 1, 16 .. 6
    objs = seal(cut, [pubs[1]] * len(cut), seed=4)
    assert sorted({receive.sealed_plan(o)[4] for o in objs}) == [176, 192]
    got = assert_equals_composition(objs, ripes[:2], privs[:2])
    assert [len(got.plaintexts[i]) for i in range(len(objs))] == list(range(170, 187))
    assert got.match.tolist() == [1] * len(objs)

    # a MAC that verifies over a ciphertext the cipher refuses: bad padding, 8 bytes, none
    make, key_e, iv = crafted(user, seed=5, key=1)
    two_blocks = bytes(range(31)) + b'\x00'
    enc = ecies.aes_cbc_batch([key_e], [iv], [two_blocks])[0]
    assert len(enc) == 48 and ecies.aes_cbc_batch([key_e], [iv], [enc[:32]], decrypt=True) == [None]
    well = ecies.aes_cbc_batch([key_e], [iv], [bytes(range(31))])[0]  # the same way, with padding that holds
    bad = [make(enc[:32]), make(enc[:8]), make(b''), make(well)]
    got = assert_equals_composition(bad + objs[:3], ripes[:2], privs[:2])
    assert got.match.tolist() == [1] * 7
    assert got.status[:3].tolist() == [receive.NOT_MINE] * 3 and got.status[3] != receive.NOT_MINE
    assert [got.plaintexts[i] for i in range(4)] == [b'', b'', b'', bytes(range(31))]
    assert [got.toRipe(i) for i in range(4)] == [ripes[1]] * 4
    assert receive.process_sealed_msgs(bad, dict(zip(ripes[:2], privs[:2]))) == [None] * 4


# ------------------------------------------------------------------ 5. row counts
@pytest.fixture(scope='module')
def handful(gpulib, senders, user):
    """Distinct objects: six for the second of the user's keys (one spoiled), four for nobody, one whose head
    refuses; all of about one size."""
    privs, pubs, ripes = user
    rows = [row(20 + k, to_ripe=ripes[1], message=bytes([k]) * (40 + k), alg=('sha1', 'sha256')[k % 2], version=(3, 4)[k % 2])
            for k in range(6)]
    rows += [row(30 + k, to_ripe=ripes[2], message=bytes([k]) * 44) for k in range(4)]
    msgs, _ = compose(rows, senders)
    msgs[5] = (msgs[5][0], msgs[5][1][:-1] + bytes([msgs[5][1][-1] ^ 1]))
    objs = seal(msgs, [pubs[1]] * 6 + [pubs[2]] * 4, seed=6)
    mine, others = objs[:6], objs[6:]
    refused = mine[0][:20] + b'\x02' + mine[0][21:]
    return mine, others, refused


@pytest.mark.parametrize('n', [1, 63, 64, 65, 129])
def test_row_counts_and_interleaved_matches(gpulib, user, handful, n):
    from pybitmessage_amd import receive
    privs, _pubs, ripes = user
    mine, others, refused = handful
    objs = [mine[(k // 2) % 6] if k % 2 == 0 else (others + [refused])[(k // 2) % 5] for k in range(n)]
    receive.sealed_reset_stats()
    got = assert_equals_composition(objs, ripes[:2], privs[:2])
    st = receive.sealed_stats()
    assert (st['calls'], st['rows'], st['sets'], st['matched']) == (1, n, 1, (n + 1) // 2)
    assert (st['launches'], st['rx_launches']) == (14, 10)
    assert got.match.tolist() == [1 if k % 2 == 0 else -1 for k in range(n)]
    assert sorted(set(got.status.tolist())) == sorted({receive.OK} | ({receive.NOT_MINE} if n > 1 else set()) |
                                                      ({receive.BAD_SIGNATURE} if n > 10 else set()) |
                                                      ({receive.MSG_VERSION} if n > 9 else set()))


def test_no_match_at_all_and_every_row_matches(gpulib, user, handful):
    from pybitmessage_amd import receive
    privs, _pubs, ripes = user
    mine, others, refused = handful
    receive.sealed_reset_stats()
    got = assert_equals_composition(others * 20 + [refused], ripes[:2], privs[:2])
    st = receive.sealed_stats()
    assert got.status.tolist() == [receive.NOT_MINE] * 80 + [receive.MSG_VERSION]
    assert (st['calls'], st['sets'], st['matched'], st['rx_launches'], st['launches']) == (1, 1, 0, 0, 4)
    assert st['open_ms'] == 0 and st['walk_ms'] == 0 and st['curve_ms'] == 0 and st['match_ms'] > 0
    receive.sealed_reset_stats()
    got = assert_equals_composition(mine * 11, ripes[:2], privs[:2])
    st = receive.sealed_stats()
    assert got.match.tolist() == [1] * 66 and (st['matched'], st['rx_launches'], st['launches']) == (66, 10, 14)
    assert all(st[k] > 0 for k in ('match_ms', 'open_ms', 'walk_ms', 'hash_ms', 'scalar_ms', 'curve_ms', 'ident_ms',
                                   'finish_ms', 'host_ms'))


# ------------------------------------------------------------------ 6. two sets
def test_two_sets(gpulib, user, handful):
    """2^18 + 1 objects of one MAC block count, so the sets split in input order: a few matches on either side."""
    from pybitmessage_amd import ecies, receive
    privs, _pubs, ripes = user
    mine, others, _refused = handful
    same = [o for o in mine if (len(o) - 22 - 32 + 9 + 63) // 64 == (len(others[0]) - 22 - 32 + 9 + 63) // 64]
    assert len(same) >= 3
    n = SET + 1
    hits = {0: same[0], 77: same[1], SET - 1: same[2], SET: same[0]}
    objs = [hits.get(i, others[i % 4]) for i in range(n)]
    small = receive.open_sealed_msgs(same[:3] + others, ([ripes[1]], [privs[1]]))
    record = {o: small.recs[k].tobytes() for k, o in enumerate(same[:3] + others)}
    receive.sealed_reset_stats()
    got = receive.open_sealed_msgs(objs, ([ripes[1]], [privs[1]]))
    st = receive.sealed_stats()
    assert (st['calls'], st['rows'], st['sets'], st['matched'], st['rx_launches'], st['launches']) == (1, n, 2, 4, 20, 28)
    assert np.flatnonzero(got.match >= 0).tolist() == sorted(hits)
    assert np.flatnonzero(got.status != receive.NOT_MINE).tolist() == sorted(hits)
    for i, o in hits.items():
        assert got.recs[i].tobytes() == record[o] and got.toRipe(i) == ripes[1]
        assert got.plaintexts[i] == ecies.process_msgs([o], {ripes[1]: privs[1]})[0][1]
    for i in (1, 2, 3, 4, SET - 2, SET + 0 - 3):
        assert got.recs[i].tobytes() == record[objs[i]] and got.plaintexts[i] == b''


# ------------------------------------------------------------------ 7. abort, empty input, no keys, the arena
def test_abort_empty_input_no_keys_and_a_small_arena(gpulib, user, handful):
    from pybitmessage_amd import _lib, receive
    privs, _pubs, ripes = user
    mine, others, refused = handful
    objs = mine + others + [refused]
    gpulib.bmpow_abort()
    try:
        with pytest.raises(_lib.BmpowError) as e:
            receive.open_sealed_msgs(objs, (ripes[:2], privs[:2]))
        assert e.value.code == _lib.E_ABORTED
    finally:
        gpulib.bmpow_clear_abort()
    assert_equals_composition(objs, ripes[:2], privs[:2])
    receive.sealed_reset_stats()
    assert len(receive.open_sealed_msgs([], (ripes[:2], privs[:2]))) == 0
    assert receive.process_sealed_msgs([], {}) == []
    got = receive.open_sealed_msgs(objs, {})
    assert got.status.tolist() == [receive.NOT_MINE] * 10 + [receive.MSG_VERSION] and got.match.tolist() == [-1] * 11
    assert receive.process_sealed_msgs(objs, {}) == [None] * 11
    # the arena one byte too small, by the raw call
    n = len(objs)
    recs = np.zeros(n, dtype=receive.MSG_REC)
    match = np.zeros(n, dtype=np.int32)
    off, ln = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    lens = np.array([len(o) for o in objs], dtype=np.uint64)
    arena = np.zeros(int(lens.sum()), dtype=np.uint8)
    ptrs = (ctypes.c_char_p * n)(*objs)

    def call(cap):
        return gpulib.bmpow_rx_sealed_msgs(n, ctypes.cast(ptrs, ctypes.c_void_p), lens.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                           2, b''.join(privs[:2]), b''.join(ripes[:2]), recs.ctypes.data, match.ctypes.data,
                                           arena.ctypes.data, cap, off.ctypes.data, ln.ctypes.data)

    assert call(arena.size - 1) == _lib.E_ARG
    st = receive.sealed_stats()
    assert (st['calls'], st['sets'], st['launches'], st['bytes_up'], st['bytes_down']) == (0, 0, 0, 0, 0)
    assert call(arena.size) == 0
    want = receive.open_sealed_msgs(objs, (ripes[:2], privs[:2]))
    assert recs.tobytes() == want.recs.tobytes() and match.tolist() == want.match.tolist()
    for i in range(n):  # each plaintext lies in its own object's share of the arena
        assert arena[int(off[i]):int(off[i]) + int(ln[i])].tobytes() == want.plaintexts[i]
        assert ln[i] == 0 or int(lens[:i].sum()) <= off[i] and off[i] + ln[i] <= int(lens[:i + 1].sum())


# ------------------------------------------------------------------ 8. the neighbours
def test_neighbours_are_unchanged_in_the_same_process(gpulib, user, handful, kats):
    """bmpow_ecies_match and bmpow_rx_msgs now share their set's body with the sealed call: their answers are
    the same before and after one, and their counters do not move across it."""
    from pybitmessage_amd import _lib, ecies, receive, sender
    privs, _pubs, ripes = user
    mine, others, refused = handful
    objs = mine + others
    payloads = [ecies.msg_payload(o) for o in objs]
    key, iv = bytes(range(32)), bytes(range(16))

    def neighbours():
        match, key_e, _ = ecies._match(payloads, privs[:2], True)
        opened = ecies.decrypt_batch(payloads, privs[:2])
        cbc = ecies.aes_cbc_batch([key] * 3, [iv] * 3, [b'', b'x' * 16, b'y' * 100])
        back = ecies.aes_cbc_batch([key] * 3, [iv] * 3, cbc, decrypt=True)
        res = receive.open_msgs(mine, [o[1] for o in opened[:6]], [ripes[1]] * 6)
        return match, key_e.tobytes(), opened, cbc, back, res.recs.tobytes()

    def counters():
        st = _lib.BmpowEciesStats()
        assert gpulib.bmpow_ecies_get_stats(ctypes.byref(st)) == 0
        return ([getattr(st, f) for f, _ in st._fields_], receive.stats(), sender.seal_stats(), receive.obj_stats())

    before = neighbours()
    assert before[0] == [1] * 6 + [None] * 4 and before[4] == [b'', b'x' * 16, b'y' * 100]
    quiet = counters()
    receive.open_sealed_msgs(objs + [refused], (ripes[:2], privs[:2]))
    assert counters() == quiet
    assert neighbours() == before
    # ... and the fixture through the old door still gives the fixture
    keys = {bytes.fromhex(k['ripe']): bytes.fromhex(k['privkey']) for k in kats['recipients']}
    out = receive.process_msgs([bytes.fromhex(m['obj']) for m in kats['msgs']], keys)
    assert [o is not None for o in out] == [m['line'] is None for m in kats['msgs']]


# ------------------------------------------------------------------ 9. what crosses the bus
def test_byte_counters(gpulib, user, handful):
    from pybitmessage_amd import ecies, receive
    privs, _pubs, ripes = user
    mine, others, refused = handful
    objs = (mine + others) * 3 + [refused, mine[0][:60]]  # the last: a payload cut inside its header, never tried
    tried = [ecies.msg_payload(o) for o in objs[:-2]]
    pool = sum((len(p) - 32 + 9 + 63) // 64 * 64 for p in tried)
    opened = [receive.sealed_plan(o)[4] for o in mine * 3]
    receive.sealed_reset_stats()
    got = receive.open_sealed_msgs(objs, (ripes[:2], privs[:2]))
    st = receive.sealed_stats()
    assert int((got.match >= 0).sum()) == st['matched'] == 18
    # up: the padded MAC pool, a point (64 B) and an ec_obj (40 B) per tried object, 64 digits of 4 B per key, and
    # the matched rows' descriptors; nothing per byte of plaintext or ciphertext beyond the pool
    assert st['bytes_up'] == pool + len(tried) * (64 + 40) + 2 * 64 * 4 + 18 * ROW_UP
    # down: match[] of the tried objects; per matched row its record, opened[] and its plaintext slot (the
    # ciphertext's length) -- not a byte for a row that did not match
    assert st['bytes_down'] == 4 * len(tried) + 18 * ROW_DOWN + sum(opened)
    assert sum(len(got.plaintexts[i]) for i in range(len(objs))) < sum(opened) <= sum(len(p) for p, o in zip(tried, objs) if o in mine)


# ------------------------------------------------------------------ 10. the four receive-side calls, alternating
def test_four_entry_points_alternate_in_one_process(gpulib, kats):
    """bmpow_rx_objects, bmpow_rx_sealed_msgs, bmpow_rx_msgs and bmpow_sig_verify share one set planner, one
    verification chain and one rows driver, and the object rows (120 bytes) and the opening kernel's rows
    (16 bytes) are two types in one library.  Here they take turns in one process, every call growing its own
    buffers afresh, at 1, 65 and 129 rows -- stride above n each time, the larger two across a wave and an
    SG_BLOCK boundary -- over the golden fixtures tiled to that size; every row of every call is its
    fixture's."""
    from pybitmessage_amd import receive, signatures
    from tests.test_rxobj import check_row_against_fixture as check_obj_row, device_rows

    def tile(rows, first, n):  # n rows from rows[first] on, round and round
        return [rows[(first + k) % len(rows)] for k in range(n)]

    obj_rows = device_rows(load_golden('rxobj_kats.json'))
    obj_first = next(i for i, r in enumerate(obj_rows) if r[1]['result'] is not None)
    msgs = kats['msgs']
    msg_first = next(i for i, m in enumerate(msgs) if m['name'] == 'ok_v4')
    opened = [m for m in msgs if m['line'] != 478]  # bmpow_rx_msgs takes the rows some key decrypts
    opened_first = next(i for i, m in enumerate(opened) if m['name'] == 'ok_v4')
    keys = {bytes.fromhex(k['ripe']): bytes.fromhex(k['privkey']) for k in kats['recipients']}
    sig_kats = load_golden('sig_kats.json')
    sigs = [(k['name'], bytes.fromhex(k['msg']), bytes.fromhex(k['sig']), bytes.fromhex(k['key']), k['code'])
            for k in sig_kats['cases']]
    sig_first = next(i for i, c in enumerate(sigs) if c[4] == 2)

    for n in (1, 65, 129):
        receive.obj_reset_stats(), receive.sealed_reset_stats(), receive.reset_stats()
        rows = tile(obj_rows, obj_first, n)
        res = receive.open_objects([r[0] for r in rows], [r[2] for r in rows], [r[3] for r in rows], [r[4] for r in rows])
        assert len(res) == n
        for i, (kind, e, _obj, _plain, _expect) in enumerate(rows):
            check_obj_row(kind, e, res, i, final=True)
            assert int(res.recs[i]['digest']) == e['digest'], (n, e['name'])
            if e['result'] is not None:
                assert (res.fromAddress(i), res.ripe(i).hex()) == (e['result']['fromAddress'], e['result']['ripe']), (n, e['name'])
                if kind == BROADCAST:
                    assert res.sigHash(i).hex() == e['result']['sigHash'], (n, e['name'])
                else:
                    assert res.storedData(i).hex() == e['result']['storedData'] and res.sigHash(i) == bytes(32), (n, e['name'])

        rows = tile(msgs, msg_first, n)
        res = receive.open_sealed_msgs([bytes.fromhex(m['obj']) for m in rows], keys)
        assert len(res) == n
        for i, m in enumerate(rows):
            check_sealed_row(m, res, i)

        rows = tile(opened, opened_first, n)
        res = receive.open_msgs([bytes.fromhex(m['obj']) for m in rows], [bytes.fromhex(m['plaintext']) for m in rows],
                                [bytes.fromhex(m['toRipe']) for m in rows])
        assert len(res) == n
        for i, m in enumerate(rows):
            check_msg_result(m, res, i)

        rows = tile(sigs, sig_first, n)
        got = signatures.verify_batch_digest([c[1] for c in rows], [c[2] for c in rows], [c[3] for c in rows])
        assert [(c[0], c[4], g) for c, g in zip(rows, got) if c[4] != g] == [], n

        # one set each, of the family's nine launches (ten behind the opening kernel, four in front for one key group)
        assert (receive.obj_stats()['sets'], receive.obj_stats()['launches']) == (1, 9), n
        assert (receive.stats()['sets'], receive.stats()['launches']) == (1, 9), n
        st = receive.sealed_stats()
        assert (st['sets'], st['rx_launches']) == (1, 10) and st['matched'] > 0, n
