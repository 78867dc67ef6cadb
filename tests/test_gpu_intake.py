"""Object intake on the GPU: ``intake.inventory_hashes`` against hashlib, the two launch shapes against
each other and against ``verify.pow_values``, and ``intake.check_objects`` against the reference-made
fixture ``tests/golden/intake_kats.json`` (tests/golden/make_intake_golden.py)."""
import hashlib
import random
import struct

import numpy as np
import pytest

from pybitmessage_amd import _lib, intake, verify
from tests.golden.make_intake_golden import regen

pytestmark = pytest.mark.gpu


def inv_hash(obj):
    return hashlib.sha512(hashlib.sha512(obj).digest()).digest()[:32]


@pytest.fixture(scope='module')
def kats(golden):
    return golden('intake_kats.json')


@pytest.fixture(scope='module')
def ragged():
    """4000 objects, 8 B to 20 KB, in no order: several waves per size class, lanes of unlike length."""
    rng = random.Random(4000)
    data = rng.randbytes(1 << 20)
    sizes = [rng.choice([8, 9, 54, 119, 120, 121, 247, 248, 249, rng.randrange(8, 600), rng.randrange(8, 3000)])
             for _ in range(3990)] + [20000, 16384, 12000, 8191, 5000, 4097, 4096, 3000, 2999, 2048]
    rng.shuffle(sizes)
    objs = []
    for L in sizes:
        at = rng.randrange(0, len(data) - L)
        objs.append(data[at:at + L])
    return objs, [inv_hash(o) for o in objs]


def test_every_length_across_the_block_edges(gpulib):
    """L = 8 .. 441 crosses nblk's edges (L - 8 = 111 | 112, 239 | 240) and nblk2's (L = 111 | 112, 239 | 240)."""
    rng = random.Random(441)
    objs = [rng.randbytes(L) for L in range(8, 442)]
    got = intake.inventory_hashes(objs)
    for o, g in zip(objs, got):
        assert g == inv_hash(o), len(o)


def test_long_objects_and_one_long_lane_among_short_ones(gpulib):
    rng = random.Random(300000)
    objs = [rng.randbytes(rng.randrange(8, 400)) for _ in range(3000)]
    objs.insert(1234, rng.randbytes(300000))
    objs.append(rng.randbytes(262152))
    got = intake.inventory_hashes(objs)
    assert len(got) == len(objs)
    for i, (o, g) in enumerate(zip(objs, got)):
        assert g == inv_hash(o), (i, len(o))


def test_the_nonce_is_part_of_the_hash(gpulib):
    payload = random.Random(2).randbytes(200)
    a, b = struct.pack('>Q', 1) + payload, struct.pack('>Q', 2) + payload
    ha, hb = intake.inventory_hashes([a, b])
    assert ha != hb and ha == inv_hash(a) and hb == inv_hash(b)
    assert verify.pow_values([a, b]) != verify.pow_values([a, a])


@pytest.mark.parametrize('ids', [[0], [0, 0, 0]])
def test_sorted_and_binned_launches_agree(gpulib, shards, monkeypatch, ragged, ids):
    objs, want = ragged
    shards(ids)
    pows = verify.pow_values(objs)
    for binned in ('0', '1'):
        monkeypatch.setenv('BMPOW_VBINNED', binned)
        intake.reset_stats()
        assert intake.inventory_hashes(objs) == want, binned
        res = intake.check_objects(objs, now=1700000000)
        for i, w in enumerate(want):  # random bytes: most headers decode, objects under 20 B never
            assert res.inventory_hash(i) == (bytes(32) if res.status[i] == intake.MALFORMED else w), (binned, i)
        ok = res.status != intake.MALFORMED
        assert ok.sum() > 2500
        assert res.pow[ok].tolist() == [p for p, k in zip(pows, ok) if k], binned
        st = intake.stats()
        assert st['calls'] == 2 and st['launches'] == 2 * len(ids) and st['objects'] == len(objs) + int(ok.sum())
        assert st['kernel_ms'] > 0


def test_a_flood_under_the_default_rule(gpulib):
    """140 000 objects of 54 - 208 B: above the binned kernel's threshold on any device up to 273 CUs."""
    n = 140000
    rng = np.random.default_rng(140000)
    raw = rng.bytes(n * 208)
    lens = rng.integers(54, 209, size=n)
    objs = [raw[208 * i:208 * i + int(L)] for i, L in enumerate(lens)]
    got = intake.inventory_hashes(objs)
    assert len(got) == n
    for i in range(0, n, 97):
        assert got[i] == inv_hash(objs[i]), i


def test_check_objects_reproduces_the_fixture(gpulib, kats):
    groups = {}
    for k in kats['kats']:
        for c in k['checks']:
            groups.setdefault((c['now'], tuple(c['streams'])), []).append((k, c))
    assert len(groups) >= 8
    seen = set()
    for (now, streams), items in groups.items():
        objs = [regen(k) for k, _ in items]
        res = intake.check_objects(objs, streams=streams, now=now)
        assert len(res) == len(objs)
        for i, (k, c) in enumerate(items):
            assert res.status[i] == c['status'], (k['name'], c)
            seen.add(c['status'])
            f = k['fields']
            if f is None:
                assert res.inventory_hash(i) == bytes(32) and res.pow[i] == 0
                continue
            assert (int(res.expiresTime[i]), int(res.objectType[i]), int(res.version[i]), int(res.streamNumber[i]),
                    int(res.payloadOffset[i])) == (f['expires'], f['type'], f['version'], f['stream'],
                                                   f['payloadOffset']), k['name']
            assert int(res.records['nonce'][i]) == f['nonce']
            assert res.tag(i).hex() == f['tag'], k['name']
            if c['status'] == intake.TOO_LARGE:  # never uploaded
                assert res.inventory_hash(i) == bytes(32) and res.pow[i] == 0
            else:
                assert res.inventory_hash(i).hex() == f['inv'], k['name']
    assert seen == set(range(9))
    # the hashes alone, for everything long enough to have one
    objs = [regen(k) for k in kats['kats'] if k['L'] >= 8]
    assert intake.inventory_hashes(objs) == [inv_hash(o) for o in objs]


def test_ok_agrees_with_the_pow_batch_plus_the_host_checks(gpulib, kats):
    now = kats['now']
    objs = [regen(k) for k in kats['kats'] if k['fields'] is not None]
    pow_ok = verify.isProofOfWorkSufficient_batch(objs, recvTime=now)
    res = intake.check_objects(objs, now=now)
    want = [intake.status_of(intake.header(o), len(o), p, now) for o, p in zip(objs, pow_ok)]
    assert res.status.tolist() == want
    assert (res.status == intake.OK).sum() >= 12
    assert res.accepted().tolist() == [i for i, s in enumerate(want) if s == intake.OK]
    assert res.pow[res.status != intake.TOO_LARGE].tolist() == \
        verify.pow_values([o for o, s in zip(objs, want) if s != intake.TOO_LARGE])


def test_parameters_and_edges(gpulib, kats):
    assert intake.inventory_hashes([]) == []
    empty = intake.check_objects([])
    assert len(empty) == 0 and empty.status.shape == (0,) and empty.inventoryHash.shape == (0, 32)
    with pytest.raises(_lib.BmpowError) as e:
        intake.inventory_hashes([bytes(100), bytes(7)])
    assert e.value.code == _lib.E_ARG
    assert intake.inventory_hashes([bytearray(8), memoryview(bytes(9))]) == [inv_hash(bytes(8)), inv_hash(bytes(9))]
    by_name = {k['name']: k for k in kats['kats']}
    now = kats['now']
    msg = regen(by_name['msg_ok'])
    # difficulty and recvTime are the call's: the network minimum passes, a demand 2^40 times it does not,
    # and recvTime moves the TTL the target is computed from
    assert intake.check_objects([msg], now=now).status.tolist() == [intake.OK]
    assert intake.check_objects([msg], now=now, nonceTrialsPerByte=1000, payloadLengthExtraBytes=1000).status[0] == intake.OK
    assert intake.check_objects([msg], now=now, nonceTrialsPerByte=1000 << 40).status[0] == intake.INSUFFICIENT_POW
    assert intake.check_objects([msg], now=now, payloadLengthExtraBytes=1 << 50).status[0] == intake.INSUFFICIENT_POW
    assert intake.check_objects([msg], now=now, recvTime=now - (1 << 40)).status[0] == intake.INSUFFICIENT_POW
    assert intake.check_objects([msg], now=now, recvTime=now).status[0] == intake.OK
    assert intake.check_objects([msg], now=now, streams=[2]).status[0] == intake.UNWANTED_STREAM
    assert intake.check_objects([msg], now=now, streams=np.array([7, 1])).status[0] == intake.OK
    # now = 0 is the clock: a 2023 object expired long ago
    assert intake.check_objects([msg]).status[0] == intake.EXPIRED_PAST
    with pytest.raises(_lib.BmpowError):
        intake.check_objects([msg], nonceTrialsPerByte=1 << 62)
