"""Sender identification without a GPU: the host restatements of ``src/addresses.py`` and the broadcast / v4
pubkey extractors against tests/golden/ident_kats.json (made by running the reference's primitives,
tests/golden/make_ident_golden.py), the fixture's ripes against the oracle's RIPEMD-160, and the
byte-oriented code the kernel shares with the host (pybitmessage_amd/csrc/bmpow_ident_fmt.h) as a stand-alone
program under AddressSanitizer + UBSan (tests/native/ident_sim.cpp, against libcrypto)."""
import hashlib
import os
import subprocess

import pytest

from tests.conftest import ROOT, load_golden

CSRC = os.path.join(ROOT, 'pybitmessage_amd', 'csrc')


@pytest.fixture(scope='module')
def kats():
    return load_golden('ident_kats.json')


def test_fixture_covers_what_it_claims(kats):
    rows = kats['addresses']
    assert {r['version'] for r in rows} == {1, 2, 3, 4, 5, 252, 253}
    assert {r['stream'] for r in rows} == {1, 252, 253, 65535, 65536, 2 ** 32, 2 ** 64 - 1}
    zeros = {len(r['ripe']) // 2 - len(bytes.fromhex(r['ripe']).lstrip(b'\x00')) for r in rows}
    assert zeros == {0, 1, 2, 3, 19, 20}
    assert {m['decoded'][0] for m in kats['malformed']} == {
        'success', 'invalidcharacters', 'checksumfailed', 'varintmalformed', 'versiontoohigh', 'ripetooshort',
        'ripetoolong', 'encodingproblem'}
    lines = {b['line'] for b in kats['broadcasts']}
    assert {None, 760, 801, 810, 820, 830, 838, 848, 882, 893, 901, 916, 'varint'} <= lines
    assert {None, 423, 428, 442, 457, 484, 497, 'varint'} <= {p['line'] for p in kats['pubkeys_v4']}
    assert len(kats['keys']) >= 40


def test_encode_address_matches_the_reference(kats):
    from pybitmessage_amd import addresses
    for r in kats['addresses'] + kats['edge_addresses']:
        assert addresses.encodeAddress(r['version'], r['stream'], bytes.fromhex(r['ripe'])) == r['address'], r
    assert {(r['version'], r['stream']) for r in kats['edge_addresses']} >= {(0, 1), (0, 0), (4, 0), (2 ** 64 - 1, 2 ** 64 - 1)}


def _decoded(res):
    return [res[0], res[1], res[2], res[3].hex()]


def test_decode_address_matches_the_reference(kats):
    from pybitmessage_amd import addresses
    for r in kats['addresses'] + kats['malformed']:
        want = r['decoded'] or ['success', r['version'], r['stream'], r['ripe']]  # null: it decodes to itself
        assert _decoded(addresses.decodeAddress(r['address'])) == want, r
    # what encodes decodes to itself wherever the reference can decode it at all
    for r in kats['addresses']:
        if r['version'] > 4:
            assert r['decoded'][0] == 'versiontoohigh', r
        elif r['decoded'] is not None:  # only a version-4 ripe stripped to fewer than 4 bytes does not come back
            assert r['version'] == 4 and r['decoded'][0] == 'ripetooshort' and r['ripe'].startswith('00' * 17), r
    assert addresses.decodeAddress(kats['addresses'][0]['address'].encode()) == \
        addresses.decodeAddress(kats['addresses'][0]['address'])


def test_varints_and_base58_round_trip():
    from pybitmessage_amd import addresses
    for v in (0, 1, 252, 253, 254, 65535, 65536, 2 ** 32 - 1, 2 ** 32, 2 ** 64 - 1):
        enc = addresses.encodeVarint(v)
        assert addresses.decodeVarint(enc) == (v, len(enc))
        assert addresses.decodeVarint(enc + b'tail') == (v, len(enc))
    assert addresses.decodeVarint(b'') == (0, 0)
    for bad in (b'\xfd\x00\xfc', b'\xfd\x01', b'\xfe\x00\x00\xff\xff', b'\xfe\x00\x01\x00', b'\xff' + bytes(4) + b'\xff' * 4,
                b'\xff' + bytes(7)):
        with pytest.raises(addresses.varintDecodeError):
            addresses.decodeVarint(bad)
    for n in (0, 1, 57, 58, 58 ** 5 - 1, 58 ** 5, 2 ** 336 - 1):
        assert addresses.decodeBase58(addresses.encodeBase58(n)) == n
    assert addresses.decodeBase58('0') == 0 and addresses.decodeBase58('2 2') == 0
    data = b'an object'
    assert addresses.calculateInventoryHash(data) == hashlib.sha512(hashlib.sha512(data).digest()).digest()[:32]


def test_fixture_ripes_equal_the_oracle(kats):
    from oracle import addrgen_oracle
    for k in kats['keys']:
        pub = bytes.fromhex(k['pub_signing']) + bytes.fromhex(k['pub_encryption'])
        assert addrgen_oracle.ripemd160(hashlib.sha512(pub).digest()).hex() == k['ripe']
    assert sum(k['ripe'].startswith('0000') for k in kats['keys']) >= 1
    assert sum(k['ripe'].startswith('00') and not k['ripe'].startswith('0000') for k in kats['keys']) >= 1


def _parts_dict(p):
    if p is None:
        return None
    return {k: (v.hex() if isinstance(v, bytes) else v) for k, v in p._asdict().items()}


def test_broadcast_extractors_match_every_fixture_object(kats):
    from pybitmessage_amd import signatures
    seen = 0
    for b in kats['broadcasts']:
        obj = bytes.fromhex(b['obj'])
        head = signatures.broadcast_header(obj)
        if b['line'] in (760,) or (b['line'] == 'varint' and b['plaintext'] is None):
            assert head is None, b['name']
            continue
        assert head is not None and head[0] in (4, 5), b['name']
        assert (head[2] is None) == (head[0] == 4)
        if b['plaintext'] is None:
            continue
        got = _parts_dict(signatures.broadcast_signed_parts(obj, bytes.fromhex(b['plaintext'])))
        assert got == b['parts'], b['name']
        if got is not None:
            assert got['signedData'].startswith(obj[8:head[3]].hex())
            seen += 1
        if b['result'] is not None:
            assert got is not None and sorted(b['result']) == ['fromAddress', 'ripe', 'sigHash']
    assert seen >= 20


def test_pubkey_v4_extractor_matches_every_fixture_object(kats):
    from pybitmessage_amd import signatures
    for p in kats['pubkeys_v4']:
        obj = bytes.fromhex(p['obj'])
        got = _parts_dict(signatures.pubkey_v4_signed_parts(obj, bytes.fromhex(p['plaintext'])))
        assert got == p['parts'], p['name']
        own = signatures.pubkey_v4_header(obj)
        if p['parts'] is not None:
            assert (own[0], own[1], own[2].hex()) == (got['addressVersion'], got['stream'], got['tag'])
            assert got['signedData'].startswith(obj[8:own[3]].hex())
            if p['storedData'] is not None:
                assert got['storedData'] == p['storedData']


def test_subscription_keys_are_the_references_statements(kats):
    """The generator's keys against hashlib (src/shared.py:169-184), so the GPU test compares with values
    that two sources agree on."""
    from pybitmessage_amd import addresses
    for s in kats['subscriptions']:
        assert _decoded(addresses.decodeAddress(s['address'])) == ['success', s['version'], s['stream'], s['ripe']]
        data = addresses.encodeVarint(s['version']) + addresses.encodeVarint(s['stream']) + bytes.fromhex(s['ripe'])
        d1 = hashlib.sha512(data).digest()
        d2 = hashlib.sha512(d1).digest()
        want = (s['ripe'], d1[:32].hex()) if s['version'] <= 3 else (d2[32:].hex(), d2[:32].hex())
        assert (s['lookup_key'], s['privkey']) == want


def test_argument_errors_before_any_device():
    from pybitmessage_amd import addresses
    with pytest.raises(ValueError):
        addresses.derive_batch([bytes(63)], [bytes(64)], [4], [1])
    with pytest.raises(ValueError):
        addresses.derive_batch([bytes(64)], [bytes(64), bytes(64)], [4, 4], [1, 1])
    with pytest.raises(ValueError):
        addresses.encode_batch([4], [1], [bytes(19)])
    with pytest.raises(ValueError):
        addresses.encode_batch([1 << 64], [1], [bytes(20)])
    with pytest.raises(ValueError):
        addresses.encode_batch([4, 4], [1], [bytes(20)])


def test_ident_rec_layout():
    import ctypes

    from pybitmessage_amd import _lib, addresses
    assert ctypes.sizeof(_lib.BmpowIdentRec) == 180 == addresses.REC.itemsize
    for name in ('ripe', 'key_v3', 'tag_key', 'tag', 'addr_len', 'addr'):
        assert getattr(_lib.BmpowIdentRec, name).offset == addresses.REC.fields[name][1]
    lib = _lib.load()  # binds every symbol of include/bmpow_ident.h; no device
    assert lib.bmpow_ident_derive and lib.bmpow_ident_from_ripe


def test_ident_sim_under_sanitizers(tmp_path, kats):
    """A program of its own (its own main, the sanitizer runtimes linked in), never loaded into this
    process: the fixture's address rows and varints through the header the kernel is built from, then its
    own sweep of every string length against a byte-wise long division."""
    from pybitmessage_amd import addresses
    rows = ['A %d %d %s %s' % (r['version'], r['stream'], r['ripe'], r['address'][3:])
            for r in kats['addresses'] + kats['edge_addresses']]
    rows += ['V %d %s' % (v, addresses.encodeVarint(v).hex())
             for v in (0, 1, 252, 253, 65535, 65536, 2 ** 32 - 1, 2 ** 32, 2 ** 64 - 1)]
    (tmp_path / 'rows.txt').write_text('\n'.join(rows) + '\n')
    exe = tmp_path / 'ident_sim'
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-Werror', '-Wno-unknown-pragmas',
                           '-fsanitize=undefined,address', '-fno-sanitize-recover=all', '-static-libasan',
                           '-static-libubsan', '-I', CSRC, os.path.join(ROOT, 'tests', 'native', 'ident_sim.cpp'),
                           '-o', str(exe), '-lcrypto'])
    env = dict(os.environ)
    env['ASAN_OPTIONS'] = 'halt_on_error=1 detect_leaks=1'
    env['UBSAN_OPTIONS'] = 'halt_on_error=1 print_stacktrace=1'
    r = subprocess.run([str(exe), str(tmp_path / 'rows.txt')], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    assert 'all ident checks passed (%d rows)' % len(rows) in r.stderr
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr
