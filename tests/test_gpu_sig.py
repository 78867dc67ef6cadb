"""Signature verification on the GPU (``bmpow_sig_verify``, ``bmpow_ecdsa_verify_digest``,
``pybitmessage_amd.signatures``) against the reference-made fixture ``tests/golden/sig_kats.json``
(pyelliptic and highlevelcrypto.verify over OpenSSL, tests/golden/make_sig_golden.py): every verdict is
the reference's, 1 under SHA-1, 2 under SHA-256 only, 0 invalid."""
import random

import pytest

from pybitmessage_amd import signatures

pytestmark = pytest.mark.gpu

P = 2 ** 256 - 2 ** 32 - 977
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141


@pytest.fixture(scope='module')
def kats(golden):
    return golden('sig_kats.json')


@pytest.fixture(scope='module')
def triples(kats):
    """Every case as (name, msg, sig, key, code), the objects' signed parts included."""
    out = [(k['name'], bytes.fromhex(k['msg']), bytes.fromhex(k['sig']), bytes.fromhex(k['key']), k['code'])
           for k in kats['cases']]
    for o in kats['pubkey_objects'] + kats['msg_objects']:
        if o['parts']:
            p = o['parts']
            code = 0
            if o['verdict']:
                code = 1 if o['name'].endswith('sha1') else 2
            out.append((o['name'], bytes.fromhex(p['signed']), bytes.fromhex(p['sig']), bytes.fromhex(p['key']), code))
    return out


def b32(v):
    return v.to_bytes(32, 'big')


def run(cases):
    return signatures.verify_batch_digest([c[1] for c in cases], [c[2] for c in cases], [c[3] for c in cases])


def mismatches(cases, got):
    return [(c[0], c[4], g) for c, g in zip(cases, got) if c[4] != g]


def test_every_fixture_case_in_one_call(gpulib, triples):
    got = run(triples)
    assert not mismatches(triples, got)
    names = {c[0]: g for c, g in zip(triples, got)}
    # the cases the final test and the complete additions exist for
    for alg, code in (('sha1', 1), ('sha256', 2)):
        assert names['xR_above_n_' + alg] == names['xR_twin_below_n_' + alg] == code
        assert names['valid_by_doubling_' + alg] == names['valid_by_doubling_small_u1_' + alg] == code
        assert names['R_infinity_' + alg] == names['equal_halves_wrong_' + alg] == 0
    assert sorted(set(got)) == [0, 1, 2]


@pytest.mark.parametrize('n', [1, 63, 64, 65])
def test_call_sizes(gpulib, triples, n):
    for start in (0, 24, len(triples) - n):  # 24: the first SHA-256 cases
        part = triples[start:start + n]
        assert not mismatches(part, run(part)), start


def test_shuffled_batch_of_mixed_lengths(gpulib, triples):
    rng = random.Random(5)
    batch = [rng.choice(triples) for _ in range(300)]
    assert len({len(c[1]) for c in batch}) > 10  # the block-count sort has something to sort
    assert not mismatches(batch, run(batch))


def test_verify_digest_kats(gpulib, kats):
    d = kats['digest_cases']
    assert {'e_zero', 'e_is_n', 'e_is_n_plus_1', 'e_all_ones'} <= {k['name'] for k in d if k['valid']}
    got = signatures.ecdsa_verify_digest([bytes.fromhex(k['key']) for k in d],
                                         [bytes.fromhex(k['r'] + k['s']) for k in d],
                                         [bytes.fromhex(k['e']) for k in d])
    assert got == [k['valid'] for k in d], [k['name'] for k, g in zip(d, got) if g != k['valid']]
    # e is taken mod n: e and e + n (where that is below 2^256) give one verdict
    small = next(k for k in d if k['name'] == 'e_zero')
    twice = signatures.ecdsa_verify_digest([bytes.fromhex(small['key'])] * 2, [bytes.fromhex(small['r'] + small['s'])] * 2,
                                           [b32(0), b32(N)])
    assert twice == [True, True]


def test_verify_digest_is_strict(gpulib, kats):
    k = next(k for k in kats['digest_cases'] if k['name'] == 'e_random')
    key, r, s, e = bytes.fromhex(k['key']), bytes.fromhex(k['r']), bytes.fromhex(k['s']), bytes.fromhex(k['e'])
    x, y = int.from_bytes(key[:32], 'big'), int.from_bytes(key[32:], 'big')
    rows = [
        (key, r + s, True),
        (b32(x) + b32((y + 1) % P), r + s, False),           # off the curve
        (b32(x) + b32(P - y), r + s, False),                 # the negated key: on the curve, wrong
        (b32(P) + b32(y), r + s, False),                     # coordinate = p
        (b32(x) + b32(2 ** 256 - 1), r + s, False),          # coordinate >= p
        (bytes(64), r + s, False),
        (key, b32(0) + s, False),
        (key, r + b32(0), False),
        (key, b32(N) + s, False),
        (key, r + b32(N), False),
        (key, r + b32(N - int.from_bytes(s, 'big')), True),  # the high-s twin
        (key, s + r, False),
    ]
    got = signatures.ecdsa_verify_digest([row[0] for row in rows], [row[1] for row in rows], [e] * len(rows))
    assert got == [row[2] for row in rows]


def test_one_ladder_per_parsable_signature(gpulib, triples, kats):
    der_ok = {k['name']: k['der_ok'] for k in kats['cases']}
    in_range = lambda key: int.from_bytes(key[:32], 'big') < P and int.from_bytes(key[32:], 'big') < P  # noqa: E731
    uploaded = [c for c in triples if der_ok.get(c[0], signatures.parse(c[2]) is not None) and in_range(c[3])]
    assert 0 < len(uploaded) < len(triples)
    signatures.reset_stats()
    run(triples)
    st = signatures.stats()
    assert st['calls'] == 1 and st['submitted'] == len(triples)
    assert st['uploaded'] == len(uploaded)  # unparsable signatures (and keys >= p) never reach the device
    assert st['ladders'] == len(uploaded)   # one u2 Q per signature serves both digests: never twice that
    assert st['launches'] == 5
    assert st['hash_ms'] > 0 and st['scalar_ms'] > 0 and st['curve_ms'] > 0 and st['host_ms'] > 0
    # nothing parsable: nothing launched
    signatures.reset_stats()
    bad = [c for c in triples if c[0].startswith('der_') and c[4] == 0]
    assert len(bad) >= 11 and run(bad) == [0] * len(bad)
    st = signatures.stats()
    assert st['calls'] == 0 and st['uploaded'] == 0 and st['ladders'] == 0 and st['submitted'] == len(bad)
    assert signatures.verify_batch_digest([], [], []) == []


def test_verify_end_to_end(gpulib, kats):
    by_name = {k['name']: k for k in kats['cases']}
    for name in ('valid_sha1_len65', 'valid_sha256_len3001'):
        k = by_name[name]
        msg, sig, key = bytes.fromhex(k['msg']), bytes.fromhex(k['sig']), bytes.fromhex(k['key'])
        hexkey = (b'\x04' + key).hex()
        assert signatures.verify(msg, sig, hexkey) is True
        assert signatures.verify(msg, sig, hexkey.encode()) is True
        assert signatures.verify(msg + b'\x00', sig, hexkey) is False
        assert signatures.verify(msg, sig, hexkey[:-4]) is False  # no key at all: the reference's except
    for o in kats['pubkey_objects']:
        parts = signatures.pubkey_v3_signed_parts(bytes.fromhex(o['obj']))
        assert (parts is None) == (o['verdict'] is None), o['name']
        if parts:
            assert signatures.verify(parts[0], parts[1], (b'\x04' + parts[2]).hex()) is o['verdict'], o['name']
    for o in kats['msg_objects']:
        parts = signatures.msg_signed_parts(bytes.fromhex(o['obj']), bytes.fromhex(o['plaintext']))
        assert (parts is None) == (o['verdict'] is None), o['name']
        if parts:
            assert signatures.verify(parts[0], parts[1], (b'\x04' + parts[2]).hex()) is o['verdict'], o['name']
    assert signatures.verify_batch([b'a', b'b'], [b'', b'\x30\x00'], [bytes(64), bytes(65)]) == [False, False]
