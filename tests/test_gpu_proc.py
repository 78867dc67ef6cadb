"""The object processor's dispatch on the GPU (``pybitmessage_amd.processor``) against the reference-made fixture
``tests/golden/proc_kats.json`` (tests/golden/make_proc_golden.py) and against dicts written here: the whole fixture
as one queue under several launch sizes, empty tables, one key under a wave and a lane of its acks, constructed tag
and start-slot collisions, tails at every alignment, a long tail that differs in its last byte, and a dispatcher's
life across a re-selection, an abort and a live PoW service.  Every malformed input here is a defined status:
nothing provokes a fault."""
import random
import threading

import numpy as np
import pytest

from pybitmessage_amd import _lib, processor as P, worker
from tests.proc_expect import address_table, check_verdict, expected_acks, objects

pytestmark = pytest.mark.gpu

SEED = 20251021


@pytest.fixture(scope='module')
def kats(golden):
    return golden('proc_kats.json')


def ack_object(tail, object_type=P.OBJECT_MSG):
    """An object whose data[16:] is tail (tail[:4] is where the type would stand: never read)."""
    return bytes(16) + bytes(tail)


def ack_columns(res):
    return list(zip(res.ack.tolist(), res.ack_aux.tolist(), res.ack_first.tolist()))


def fixture_dispatcher(kats, seed=SEED):
    d = P.Dispatcher(seed=seed)
    keys = [bytes.fromhex(k) for k in kats['watch']]
    assert d.watch(keys, aux=range(len(keys))).all()
    d.set_addresses(address_table(kats))
    return d


def check_fixture(kats, d, res):
    objs, _ = objects(kats)
    table = address_table(kats)
    for row, rec, data in zip(kats['rows'], res.records, objs):
        check_verdict(kats, row, rec, data, table)
    assert ack_columns(res) == expected_acks(kats)
    left = [k for k in kats['watch'] if d.watching(bytes.fromhex(k))]
    assert sorted(left) == kats['watch_left'] and len(d) == len(left)


# ---- 1. the fixture as one queue ----

@pytest.mark.parametrize('rows_per_launch', [0, 1, 3, 64])
def test_the_whole_fixture_in_one_call(gpulib, kats, rows_per_launch):
    objs, types = objects(kats)
    assert len(objs) > 64
    with fixture_dispatcher(kats) as d:
        res = d.dispatch(objs, types, now=kats['now'], rows_per_launch=rows_per_launch)
        check_fixture(kats, d, res)
        st = d.stats()
        assert st['calls'] == 1 and st['rows'] == len(objs) and st['found'] == len(kats['watch']) - len(kats['watch_left'])
        assert 0 < st['rows_uploaded'] <= st['rows'] + st['ack_rows']
        per = rows_per_launch or st['rows_uploaded']
        assert st['launches'] == -(-st['rows_uploaded'] // per) + 1  # the rows launches and the finish
        # the helpers, against the fixture
        assert res.acks().tolist() == [i for i, r in enumerate(kats['rows']) if r['ack_left']]
        assert all(res.ack_key(i).hex() in kats['watch'] for i in res.acks())
        want = [(i, r['command'][0], r['command'][1]) for i, r in enumerate(kats['rows']) if r['command']]
        got = [(i, c, kats['addresses'][a]['address'] if isinstance(a, int) else a.hex()) for i, c, a in res.pubkey_requests()]
        assert got == want
        want = [(i, r['peer'][0], r['peer'][2]) for i, r in enumerate(kats['rows']) if r['peer']]
        assert [(i, s, port) for i, s, _, _, port in res.peers()] == want
        for route, idx in ((P.MSG, res.msgs()), (P.BROADCAST, res.broadcasts()), (P.PUBKEY, res.pubkeys())):
            assert idx.tolist() == [i for i, t in enumerate(types) if t == route]
        # the same queue again: every key found then is gone now
        again = d.dispatch(objs, types, now=kats['now'], rows_per_launch=rows_per_launch)
        assert not np.isin(again.ack, [P.FOUND, P.FOUND_EARLIER]).any()
        assert again.status.tolist() == res.status.tolist()


def test_the_fixture_reversed_and_doubled(gpulib, kats):
    """FOUND / FOUND_EARLIER pairs in the other direction across launches, against a dict run here."""
    objs, types = objects(kats)
    objs, types = (objs + objs)[::-1], (types + types)[::-1]
    aux = {bytes.fromhex(k): i for i, k in enumerate(kats['watch'])}
    want, found = [], {}
    for i, o in enumerate(objs):
        tail = o[16:]
        if len(o) < 32:
            want.append((P.NOT_CHECKED, 0, P.NO_ROW))
        elif tail in found:
            want.append((P.FOUND_EARLIER, aux[tail], found[tail]))
        elif tail in aux:
            found[tail] = i
            want.append((P.FOUND, aux[tail], i))
        else:
            want.append((P.NOT_WATCHED, 0, P.NO_ROW))
    for rows_per_launch in (5, 64):
        with fixture_dispatcher(kats, seed=3) as d:
            res = d.dispatch(objs, types, now=kats['now'], rows_per_launch=rows_per_launch)
            assert ack_columns(res) == want
            assert len(d) == len(aux) - len(found)
            half = len(objs) // 2
            assert res.status[:half].tolist() == res.status[half:].tolist()  # two accepted requests both say SEND_*


# ---- 2. empty tables, n = 0, n = 1 ----

def test_empty_tables_and_tiny_batches(gpulib, kats):
    objs, types = objects(kats)
    with P.Dispatcher(seed=SEED) as d:
        assert len(d.dispatch([], [])) == 0 and d.stats()['calls'] == 0
        res = d.dispatch(objs, types, now=kats['now'])
        assert res.ack.tolist() == [P.NOT_CHECKED if len(o) < 32 else P.NOT_WATCHED for o in objs]
        assert (res.ack_first == P.NO_ROW).all() and (res.address == P.NO_ROW).all()
        for rec, o, t in zip(res.records, objs, types):
            want = P.walk(t, o, None, now=kats['now'])
            assert rec['status'] == want['status'] and rec['route'] == want['route']
        assert d.stats()['ack_rows'] == 0 and d.stats()['table_uploads'] == 0
        one = d.dispatch([objs[0]], types[0])
        assert len(one) == 1 and one.ack[0] == P.NOT_WATCHED and one.route[0] == P.MSG
        d.watch([objs[0][16:]], aux=9)
        one = d.dispatch([objs[0]], types[0])
        assert ack_columns(one) == [(P.FOUND, 9, 0)] and len(d) == 0
        # a watch set whose keys are all shorter than any tail, and one with the empty key alone
        d.watch([b'', b'short'])
        res = d.dispatch([bytes(16), bytes(32), bytes(21)], P.OBJECT_MSG)
        assert res.ack.tolist() == [P.NOT_CHECKED, P.NOT_WATCHED, P.NOT_CHECKED] and len(d) == 2


# ---- 3. one key, a wave and a lane of its acks ----

def test_one_key_under_65_copies_of_its_ack(gpulib):
    key = bytes(range(100, 138))
    with P.Dispatcher(seed=SEED) as d:
        d.watch([key], aux=4242)
        res = d.dispatch([ack_object(key)] * 65, P.OBJECT_MSG)
        assert ack_columns(res) == [(P.FOUND, 4242, 0)] + [(P.FOUND_EARLIER, 4242, 0)] * 64
        assert len(d) == 0 and not d.watching(key)
        res = d.dispatch([ack_object(key)] * 65, P.OBJECT_MSG)
        assert ack_columns(res) == [(P.NOT_WATCHED, 0, P.NO_ROW)] * 65 and len(d) == 0


# ---- 4. constructed collisions ----

def test_equal_tags_and_one_start_slot(gpulib):
    rng = random.Random(SEED)
    # four keys of one length and one first 16 bytes: one tag, one start slot
    head = rng.randbytes(16)
    four = [head + rng.randbytes(22) for _ in range(4)]
    assert len({P.watch_slot(SEED, 4, k) for k in four}) == 1
    stranger = head + rng.randbytes(22)
    longer = four[0] + b'\x00'
    with P.Dispatcher(seed=SEED) as d:
        d.watch(four, aux=[10, 11, 12, 13])
        assert d.stats()['watch_slots'] == 8
        order = [3, 1, 0, 2]
        res = d.dispatch([ack_object(stranger), ack_object(longer)] + [ack_object(four[i]) for i in order], P.OBJECT_MSG)
        assert ack_columns(res) == [(P.NOT_WATCHED, 0, P.NO_ROW)] * 2 + [(P.FOUND, 10 + i, 2 + j) for j, i in enumerate(order)]
        assert len(d) == 0
    # three keys that start at the last slot of an 8-slot index: they lie in slots 7, 0 and 1, and a probe for a
    # fourth walks round the table's end to the empty slot 2
    at_7 = []
    while len(at_7) < 4:
        k = rng.randbytes(38)
        if P.watch_slot(SEED, 3, k) == 7 and all(k[:16] != o[:16] for o in at_7):
            at_7.append(k)
    three, fourth = at_7[:3], at_7[3]
    for absent in (None, 0, 1, 2):
        with P.Dispatcher(seed=SEED) as d:
            present = [k for i, k in enumerate(three) if i != absent]
            d.watch(present, aux=[three.index(k) for k in present])
            assert d.stats()['watch_slots'] == 8
            res = d.dispatch([ack_object(fourth)] + [ack_object(k) for k in three], P.OBJECT_MSG)
            want = [(P.NOT_WATCHED, 0, P.NO_ROW)] + [(P.NOT_WATCHED, 0, P.NO_ROW) if i == absent else (P.FOUND, i, 1 + i)
                                                    for i in range(3)]
            assert ack_columns(res) == want, absent
            assert len(d) == 0


# ---- 5. alignment ----

def test_tails_at_every_residue_and_the_pool_s_last_byte(gpulib):
    rng = random.Random(SEED + 5)
    objs = [rng.randbytes(n) for n in range(38, 54)]  # tails of 22 .. 37 bytes, uploaded back to back
    starts = np.cumsum([0] + [len(o) - 16 for o in objs[:-1]])
    assert sorted(set(int(s) % 8 for s in starts)) == list(range(8))
    total = sum(len(o) - 16 for o in objs)
    with P.Dispatcher(seed=SEED) as d:
        d.watch([o[16:] for o in objs], aux=range(16))
        # the last byte of each flipped: uploaded and compared, none found (the last row ends on the pool's last byte)
        near = [o[:-1] + bytes([o[-1] ^ 0x80]) for o in objs]
        res = d.dispatch(near, P.OBJECT_MSG)
        assert ack_columns(res) == [(P.NOT_WATCHED, 0, P.NO_ROW)] * 16 and len(d) == 16
        assert d.stats()['bytes_uploaded'] == total and d.stats()['ack_rows'] == 16
        # the first byte of each tail flipped
        near = [o[:16] + bytes([o[16] ^ 1]) + o[17:] for o in objs]
        assert d.dispatch(near, P.OBJECT_MSG).ack.tolist() == [P.NOT_WATCHED] * 16
        res = d.dispatch(objs, P.OBJECT_MSG)
        assert ack_columns(res) == [(P.FOUND, i, i) for i in range(16)] and len(d) == 0
        assert d.stats()['bytes_uploaded'] == 3 * total


def test_a_long_tail_that_differs_in_its_last_byte(gpulib):
    rng = random.Random(SEED + 6)
    obj = rng.randbytes(1 << 18)
    key = obj[16:-1] + bytes([obj[-1] ^ 1])
    with P.Dispatcher(seed=SEED) as d:
        d.watch([key, bytes(38)])
        res = d.dispatch([obj], P.OBJECT_MSG)
        assert ack_columns(res) == [(P.NOT_WATCHED, 0, P.NO_ROW)] and len(d) == 2
        st = d.stats()
        assert st['rows_uploaded'] == 1 and st['bytes_uploaded'] == (1 << 18) - 16  # uploaded: a key has its length
        d.unwatch([key])
        assert d.dispatch([obj], P.OBJECT_MSG).ack[0] == P.NOT_WATCHED
        st = d.stats()
        assert st['rows_uploaded'] == 1 and st['bytes_uploaded'] == (1 << 18) - 16  # not uploaded: no key of that length
        d.watch([obj[16:]], aux=77)
        assert ack_columns(d.dispatch([obj], P.OBJECT_MSG)) == [(P.FOUND, 77, 0)]


# ---- 6. lifecycle ----

def test_a_dispatcher_across_a_reselection_and_an_abort(gpulib, kats):
    objs, types = objects(kats)
    d = fixture_dispatcher(kats)
    n = len(d)
    gpulib.bmpow_abort()
    try:
        with pytest.raises(_lib.BmpowError) as err:
            d.dispatch(objs, types, now=kats['now'])
        assert err.value.code == _lib.E_ABORTED
    finally:
        gpulib.bmpow_clear_abort()
    assert len(d) == n and all(d.watching(bytes.fromhex(k)) for k in kats['watch'])  # nothing changed
    check_fixture(kats, d, d.dispatch(objs, types, now=kats['now']))
    _lib.reset()
    _lib.get()
    try:
        for call in (lambda: len(d), lambda: d.watch([b'k']), lambda: d.unwatch([b'k']), lambda: d.watching(b'k'), d.clear,
                     d.stats, d.reset_stats, lambda: d.set_addresses(address_table(kats)),
                     lambda: d.dispatch(objs, types), lambda: d.dispatch([], [])):
            with pytest.raises(_lib.BmpowError) as err:
                call()
            assert err.value.code == _lib.E_STATE
    finally:
        d.close()
    d.close()  # twice is fine
    with fixture_dispatcher(kats) as e:  # and a dispatcher of the new selection works
        check_fixture(kats, e, e.dispatch(objs, types, now=kats['now']))


def test_dispatch_beside_a_live_pow_service(gpulib, kats, coracle):
    objs, types = objects(kats)
    with fixture_dispatcher(kats) as d:
        quiet = d.dispatch(objs, types, now=kats['now']).records.copy()
    u64 = (1 << 64) - 1
    rng = random.Random(SEED + 7)
    easy = [(u64 // 100000, rng.randbytes(64)) for _ in range(4)]
    results, errors = [], []

    def work():
        try:
            for _ in range(20):
                with fixture_dispatcher(kats) as d:
                    results.append(d.dispatch(objs, types, now=kats['now'], rows_per_launch=16).records.copy())
        except Exception as e:  # noqa: BLE001 -- reported by the main thread
            errors.append(e)

    svc = worker.PowService().start()
    try:
        futures = svc.submit_many(easy)
        t = threading.Thread(target=work)
        t.start()
        answers = [list(f.result(60)) for f in futures]
        t.join()
    finally:
        svc.stop(30)
    assert not errors, errors
    assert len(results) == 20 and all(r.tobytes() == quiet.tobytes() for r in results)
    assert answers == [list(coracle.search(ih, target)) for target, ih in easy]


# ---- 7. behind the packets and the intake ----

def test_dispatch_packets_takes_the_accepted_objects_with_their_types(gpulib, golden):
    import hashlib
    import struct
    from pybitmessage_amd import intake, packets
    from tests.golden.make_intake_golden import regen as regen_object
    kats = golden('intake_kats.json')
    now = kats['now']
    by_name = {k['name']: regen_object(k) for k in kats['kats']}
    objs = [by_name[n] for n in ('msg_ok', 'pubkey_ok', 'broadcast_ok')]

    def packet(command, payload):
        return struct.pack('!L12sL4s', 0xE9BEB4D9, command, len(payload), hashlib.sha512(payload).digest()[:4]) + payload
    bufs = [packet(b'object', objs[0]) + packet(b'ping', b'x' * 5) + packet(b'object', objs[1]),
            packet(b'object', objs[2]) + packet(b'object', objs[0][:-1] + bytes([objs[0][-1] ^ 1])) + packet(b'object', objs[0])]
    res = packets.check_buffers(bufs, now=now)
    index = res.objects()
    assert [bytes(res.payload(int(i))) for i in index] == [objs[0], objs[1], objs[2], objs[0]]  # the spoilt one fails its POW
    with P.Dispatcher(seed=SEED) as d:
        d.watch([objs[0][16:], objs[2][16:], b'other'], aux=[5, 6, 7])
        got = d.dispatch_packets(res)
        assert got.source_index.tolist() == index.tolist()
        assert got.route.tolist() == [P.MSG, P.PUBKEY, P.BROADCAST, P.MSG]
        assert ack_columns(got) == [(P.FOUND, 5, 0), (P.NOT_WATCHED, 0, P.NO_ROW), (P.FOUND, 6, 2), (P.FOUND_EARLIER, 5, 0)]
        assert len(d) == 1
        # the same from an intake result
        d.watch([objs[1][16:]], aux=8)
        checked = intake.check_objects(objs + [objs[1][:-1] + b'\x00' if objs[1][-1] else objs[1][:-1] + b'\x01'], now=now)
        got = d.dispatch_packets(checked)
        assert got.source_index.tolist() == checked.accepted().tolist() == [0, 1, 2]
        assert got.route.tolist() == [P.MSG, P.PUBKEY, P.BROADCAST]
        assert ack_columns(got) == [(P.NOT_WATCHED, 0, P.NO_ROW), (P.FOUND, 8, 1), (P.NOT_WATCHED, 0, P.NO_ROW)]
