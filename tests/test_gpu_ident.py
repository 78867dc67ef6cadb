"""Sender identification on the GPU (include/bmpow_ident.h, pybitmessage_amd/addresses.py and receive.py)
against tests/golden/ident_kats.json, hashlib and the host restatement of encodeAddress, which
tests/test_ident.py pins to the reference.  Everything is bit-exact."""
import hashlib
import random

import numpy as np
import pytest

from tests.conftest import load_golden

pytestmark = pytest.mark.gpu

U64 = 2 ** 64 - 1
COLUMNS = ('ripe', 'key_v3', 'tag_key', 'tag')


@pytest.fixture(scope='module')
def kats():
    return load_golden('ident_kats.json')


@pytest.fixture(scope='module')
def keyrows(kats):
    """(pub_signing65, pub_encryption65, ripe) of every fixture key."""
    return [(bytes.fromhex(k['pub_signing']), bytes.fromhex(k['pub_encryption']), bytes.fromhex(k['ripe']))
            for k in kats['keys']]


def expected(version, stream, ripe):
    """One row from hashlib and the host encodeAddress."""
    from pybitmessage_amd import addresses
    data = addresses.encodeVarint(version) + addresses.encodeVarint(stream) + ripe
    d1 = hashlib.sha512(data).digest()
    d2 = hashlib.sha512(d1).digest()
    return {'ripe': ripe, 'key_v3': d1[:32], 'tag_key': d2[:32], 'tag': d2[32:],
            'address': addresses.encodeAddress(version, stream, ripe)}


def check(res, rows):
    """rows: (version, stream, ripe) per record of res."""
    assert len(res) == len(rows)
    addrs = res.addresses()
    for i, (version, stream, ripe) in enumerate(rows):
        want = expected(version, stream, ripe)
        for c in COLUMNS:
            assert getattr(res, c)[i].tobytes() == want[c], (c, i, version, stream, ripe.hex())
        assert addrs[i] == want['address'] == res.address(i), (i, version, stream, ripe.hex())


def test_fixture_keys_through_derive_batch(gpulib, keyrows):
    from pybitmessage_amd import addresses
    versions = [(2, 3, 4, 1, 5)[i % 5] for i in range(len(keyrows))]
    streams = [(1, 2, 300, 70000, 2 ** 40)[i % 5] for i in range(len(keyrows))]
    res = addresses.derive_batch([k[0] for k in keyrows], [k[1] for k in keyrows], versions, streams)
    check(res, [(v, s, k[2]) for v, s, k in zip(versions, streams, keyrows)])
    # 64-byte keys and an array of them are the same rows
    again = addresses.derive_batch(np.frombuffer(b''.join(k[0][1:] for k in keyrows), dtype=np.uint8).reshape(-1, 64),
                                   [k[1][1:] for k in keyrows], np.array(versions, dtype=np.uint64), streams)
    assert again.recs.tobytes() == res.recs.tobytes()


def test_encode_batch_over_the_cross_product(gpulib):
    from pybitmessage_amd import addresses
    rng = random.Random(7)
    rows = []
    for zeros in (0, 1, 2, 3, 19, 20):
        for version in (0, 1, 2, 3, 4, 5, 252, 253, U64):
            for stream in (0, 1, 252, 253, 65535, 65536, 2 ** 32 - 1, 2 ** 32, U64):
                rows.append((version, stream, bytes(zeros) + bytes(rng.randrange(1, 256) for _ in range(20 - zeros))))
    assert len(rows) == 486
    res = addresses.encode_batch([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows])
    check(res, rows)
    by = {(r[0], r[1], len(r[2]) - len(r[2].lstrip(b'\x00'))): a for r, a in zip(rows, res.addresses())}
    # version 4 with a zero ripe: nothing but the two varints and the checksum
    assert len(by[(4, 1, 20)]) < 14 and addresses.decodeAddress(by[(4, 1, 20)])[0] == 'ripetooshort'
    assert max(len(a) for a in res.addresses()) <= 3 + 58


def test_edge_addresses_are_the_references(gpulib, kats):
    """Version 0 (the data's leading zero byte vanishes in the integer), stream 0 and 2^64 - 1 against strings
    the reference's encodeAddress made."""
    from pybitmessage_amd import addresses
    rows = kats['edge_addresses']
    assert any(r['version'] == 0 for r in rows)
    res = addresses.encode_batch([r['version'] for r in rows], [r['stream'] for r in rows],
                                 [bytes.fromhex(r['ripe']) for r in rows])
    assert res.addresses() == [r['address'] for r in rows]


def test_both_entry_points_share_their_code(gpulib, keyrows):
    from pybitmessage_amd import addresses
    n = 3 * len(keyrows)
    versions = [(0, 1, 2, 3, 4, 5, 253, U64)[i % 8] for i in range(n)]
    streams = [(1, 252, 253, 65536, 2 ** 32, U64, 0)[i % 7] for i in range(n)]
    first = addresses.derive_batch([keyrows[i % len(keyrows)][0] for i in range(n)],
                                   [keyrows[i % len(keyrows)][1] for i in range(n)], versions, streams)
    second = addresses.encode_batch(versions, streams, first.ripe)
    assert first.recs.tobytes() == second.recs.tobytes()
    assert first.ripe.tobytes() == b''.join(keyrows[i % len(keyrows)][2] for i in range(n))


@pytest.mark.parametrize('n', [1, 63, 64, 65, 129])
def test_wave_edges(gpulib, keyrows, n):
    from pybitmessage_amd import addresses
    idx = [(5 * i + n) % len(keyrows) for i in range(n)]
    versions = [(4, 3, 2)[i % 3] for i in range(n)]
    streams = [1 + i for i in range(n)]
    check(addresses.derive_batch([keyrows[j][0] for j in idx], [keyrows[j][1] for j in idx], versions, streams),
          [(v, s, keyrows[j][2]) for v, s, j in zip(versions, streams, idx)])
    check(addresses.encode_batch(versions, streams, [keyrows[j][2] for j in idx]),
          [(v, s, keyrows[j][2]) for v, s, j in zip(versions, streams, idx)])


def test_set_split(gpulib):
    """2^18 + 1 rows repeating a 1,000-row pattern: two sets; the pattern rows against the oracle once."""
    from oracle import addrgen_oracle
    from pybitmessage_amd import addresses
    rng = np.random.default_rng(11)
    period, n = 1000, (1 << 18) + 1
    ks = rng.integers(0, 256, size=(period, 64), dtype=np.uint8)
    ke = rng.integers(0, 256, size=(period, 64), dtype=np.uint8)
    versions = np.array([(4, 3, 2, 1)[i % 4] for i in range(period)], dtype=np.uint64)
    streams = rng.integers(1, 2 ** 63, size=period, dtype=np.uint64) >> rng.integers(0, 63, size=period, dtype=np.uint64)
    rep = np.arange(n) % period
    addresses.reset_stats()
    res = addresses.derive_batch(ks[rep], ke[rep], versions[rep], streams[rep])
    st = addresses.stats()
    assert (st['calls'], st['rows'], st['sets'], st['launches']) == (1, n, 2, 2)
    raw = res.recs.view(np.uint8).reshape(n, 180)
    assert np.array_equal(raw, raw[:period][rep])
    ripes = [addrgen_oracle.ripemd160(hashlib.sha512(b'\x04' + ks[i].tobytes() + b'\x04' + ke[i].tobytes()).digest())
             for i in range(period)]
    check(addresses.Identified(res.recs[:period]), [(int(versions[i]), int(streams[i]), ripes[i]) for i in range(period)])
    # the row behind the split is a pattern row too
    assert res.address(n - 1) == res.address((n - 1) % period)


def test_no_rows_launch_nothing(gpulib):
    from pybitmessage_amd import addresses
    addresses.reset_stats()
    assert len(addresses.derive_batch([], [], [], [])) == 0
    assert len(addresses.encode_batch([], [], [])) == 0
    assert addresses.address_keys([]) == []
    st = addresses.stats()
    assert (st['calls'], st['rows'], st['sets'], st['launches']) == (0, 0, 0, 0)
    assert gpulib.bmpow_ident_derive(0, None, None, None, None) == 0


def test_argument_errors(gpulib):
    from pybitmessage_amd import _lib, addresses
    with pytest.raises(ValueError):
        addresses.derive_batch([bytes(63)], [bytes(64)], [4], [1])
    with pytest.raises(ValueError):
        addresses.derive_batch([bytes(64)], [bytes(63)], [4], [1])
    with pytest.raises(ValueError):
        addresses.encode_batch([4], [1], [bytes(19)])
    assert gpulib.bmpow_ident_derive(1, None, None, None, None) == _lib.E_ARG


def _broadcast_result(r):
    if r is None:
        return None
    return {k: (v.hex() if isinstance(v, bytes) else v) for k, v in r._asdict().items()}


def test_process_broadcasts(gpulib, kats):
    from pybitmessage_amd import receive
    subs = [s['address'] for s in kats['subscriptions']]
    cases = kats['broadcasts']
    objs = [bytes.fromhex(b['obj']) for b in cases]
    got = receive.process_broadcasts(objs, subs)
    for b, g in zip(cases, got):
        want = None if b['result'] is None else dict(b['parts'], **b['result'])
        assert _broadcast_result(g) == want, b['name']
        assert (g is None) == (b['line'] is not None), b['name']
    accepted = [g for g in got if g is not None]
    assert len(accepted) >= 6 and all(g.fromAddress.startswith('BM-') and len(g.sigHash) == 32 for g in accepted)
    # the same batch in another order, the subscriptions too, and one that does not decode among them
    order = list(range(len(objs)))
    random.Random(3).shuffle(order)
    again = receive.process_broadcasts([objs[i] for i in order], ['BM-notanaddress'] + subs[::-1])
    for j, i in enumerate(order):
        assert again[j] == got[i], cases[i]['name']
    assert receive.process_broadcasts(objs, []) == [None] * len(objs)
    assert receive.process_broadcasts([], subs) == []


def test_check_pubkeys_v4(gpulib, kats):
    from pybitmessage_amd import receive
    cases = kats['pubkeys_v4']
    got = receive.check_pubkeys_v4([bytes.fromhex(p['obj']) for p in cases], [p['address'] for p in cases])
    for p, g in zip(cases, got):
        assert (None if g is None else g.hex()) == p['storedData'], p['name']
        assert (g is None) == (p['line'] is not None), p['name']
    assert sum(g is not None for g in got) >= 3


def test_address_keys(gpulib, kats):
    from pybitmessage_amd import addresses
    subs = kats['subscriptions']
    bad = [m['address'] for m in kats['malformed'] if m['decoded'][0] != 'success']
    got = addresses.address_keys([s['address'] for s in subs] + bad)
    for s, g in zip(subs, got):
        assert g == ('success', s['version'], s['stream'], bytes.fromhex(s['ripe']), bytes.fromhex(s['lookup_key']),
                     bytes.fromhex(s['privkey'])), s['address']
    assert {s['version'] for s in subs} == {2, 3, 4}
    for a, g in zip(bad, got[len(subs):]):
        assert g == (addresses.decodeAddress(a)[0], 0, 0, b'', None, None) and g[0] != 'success'


def test_identify_msgs_and_pubkeys(gpulib):
    """receive.identify over the signature fixture's v3 pubkeys and msgs: the encryption key is found
    behind the signing key, the ripe is the oracle's."""
    from oracle import addrgen_oracle
    from pybitmessage_amd import addresses, receive, signatures
    from pybitmessage_amd.ecies import _varint
    sig = load_golden('sig_kats.json')
    parts, versions, streams = [], [], []
    for e in sig['pubkey_objects']:
        obj = bytes.fromhex(e['obj'])
        p = signatures.pubkey_v3_signed_parts(obj)
        if p is not None:
            parts.append(p), versions.append(3), streams.append(_varint(obj[21:31])[0])
    for e in sig['msg_objects']:
        p = signatures.msg_signed_parts(bytes.fromhex(e['obj']), bytes.fromhex(e['plaintext']))
        if p is not None:
            plain = bytes.fromhex(e['plaintext'])
            parts.append(p), versions.append(plain[0]), streams.append(plain[1])
    assert len(parts) >= 4
    got = receive.identify(parts, versions, streams)
    for p, v, s, (addr, ripe) in zip(parts, versions, streams, got):
        at = p[0].index(p[2])
        want = addrgen_oracle.ripemd160(hashlib.sha512(b'\x04' + p[2] + b'\x04' + p[0][at + 64:at + 128]).digest())
        assert ripe == want and addr == addresses.encodeAddress(v, s, want)
