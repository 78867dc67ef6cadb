"""Signature verification on the GPU against constructed cases: signatures whose scalars are chosen so
that the kernels take the paths the reference-made fixture never reaches -- a doubling or a cancellation
at a chosen window of the comb (and the additions onto infinity after one), structured values of u2, s,
u1 and an unreduced digest through the device's arithmetic mod n, every message length through the
hashing pass, and more signatures than one set holds.  Every expectation is the oracle's
(``oracle/ecdsa_oracle.py``, pinned to the reference by ``tests/test_ecdsa_oracle.py``, which also shows
from integers that each case reaches its branch), never the library's."""
import collections
import random
import time

import pytest

from oracle import ecdsa_oracle as eo
from pybitmessage_amd import signatures

pytestmark = pytest.mark.gpu

N, P = eo.N, eo.P
SET = 1 << 18  # kSigSetObjects (bmpow_host_sig.hip)


def b32(v):
    return v.to_bytes(32, 'big')


def digest_rows(cases):
    """(keys, r || s, digests) of Case-like tuples with Q, r, s and e or digest."""
    return ([eo.xy_key(c.Q) for c in cases], [b32(c.r) + b32(c.s) for c in cases],
            [b32(c.digest if hasattr(c, 'digest') else c.e) for c in cases])


# ------------------------------------------------------------------ 1. comb collisions
@pytest.fixture(scope='module')
def comb():
    """Every comb case: 128 hits, and per hit the two siblings that miss by one and the scaled one that
    takes the same path to a wrong r."""
    return list(eo.comb_cases())


def wrong(cases, got):
    return [(c.name, c.case.valid, g) for c, g in zip(cases, got) if c.case.valid != g]


def test_comb_collisions_in_one_call(gpulib, comb):
    got = signatures.ecdsa_verify_digest(*digest_rows([c.case for c in comb]))
    assert not wrong(comb, got)
    verdicts = collections.Counter((c.role, c.kind, c.case.valid) for c in comb)
    assert verdicts == {('hit', 'double', True): 64, ('hit', 'cancel', True): 20, ('hit', 'cancel', False): 44,
                        ('miss_sum', 'double', True): 64, ('miss_sum', 'cancel', True): 64,
                        ('miss_window', 'double', True): 64, ('miss_window', 'cancel', True): 64,
                        ('scaled', 'double', False): 64, ('scaled', 'cancel', False): 64}


def test_comb_collisions_shuffled_and_across_a_wave_boundary(gpulib, comb):
    """Hit lanes and plain lanes in one wave: the whole set shuffled, and 65 of them (a wave and a lane)."""
    mixed = comb[:]
    random.Random(8).shuffle(mixed)
    assert not wrong(mixed, signatures.ecdsa_verify_digest(*digest_rows([c.case for c in mixed])))
    part = mixed[:65]
    assert {(c.role, c.kind) for c in part[:64]} >= {('hit', 'double'), ('hit', 'cancel'), ('miss_sum', 'double'),
                                                     ('miss_window', 'cancel')}
    assert not wrong(part, signatures.ecdsa_verify_digest(*digest_rows([c.case for c in part])))


def test_a_doubling_with_a_wrong_r_is_refused(gpulib):
    """The case a comb without the equal-points test would accept (Z = 0 makes X = r Z^2 hold for any r;
    tests/test_ecdsa_oracle.py): a doubling at each hit window, r not x(R)."""
    cases = [c for c in eo.comb_cases() if c.role == 'scaled' and c.kind == 'double']
    assert len(cases) == 64
    assert signatures.ecdsa_verify_digest(*digest_rows([c.case for c in cases])) == [False] * 64


# ------------------------------------------------------------------ 2. structured scalars
def test_structured_scalars(gpulib):
    cases = eo.scalar_cases()
    got = signatures.ecdsa_verify_digest(*digest_rows(cases))
    bad = [(c.name, c.valid, g) for c, g in zip(cases, got) if c.valid != g]
    assert not bad, (len(bad), bad[:5])
    count = collections.Counter((c.family, c.valid) for c in cases)
    assert count == {('u2', True): 735, ('s', True): 735, ('u1', True): 736, ('e_plus_n', True): 64,
                     ('u2_mutant', False): 441, ('s_mutant', False): 441, ('u1_mutant', False): 444,
                     ('e_plus_n_mutant', False): 36}
    # an unreduced digest and its reduced twin give one verdict
    twins = [c._replace(digest=c.digest - N) for c in cases if c.family == 'e_plus_n']
    assert signatures.ecdsa_verify_digest(*digest_rows(twins)) == [True] * 64


# ------------------------------------------------------------------ 3. hash lengths
def test_every_message_length(gpulib):
    cases = list(eo.hash_cases())
    assert {len(c.msg) for c in cases} >= set(range(261)) | {4095, 4096, 4097}
    random.Random(9).shuffle(cases)
    got = signatures.verify_batch_digest([c.msg for c in cases], [c.sig for c in cases], [c.key for c in cases])
    bad = [(c.name, c.code, g) for c, g in zip(cases, got) if c.code != g]
    assert not bad, (len(bad), bad[:5])
    assert collections.Counter(c.code for c in cases) == {0: 264, 1: 132, 2: 132}


# ------------------------------------------------------------------ 4. more than one set per call
def uploads(sig, key):
    """Whether the host sends the row to the device: a canonical DER signature with 1 <= r, s < n and a
    64-byte key with both coordinates below p."""
    rs = eo.der_decode(sig)
    return rs is not None and 1 <= rs[0] < N and 1 <= rs[1] < N and len(key) == 64 and max(eo.key_xy(key)) < P


def test_two_sets_in_one_message_call(gpulib):
    """2^18 + 65 rows that reach the device, in one call: the second pass of the set loop, its new
    stride, and the scatter through ``orig`` with rows in between that never go up."""
    rng = random.Random(10)
    cases = eo.hash_cases()[:2 * 261]  # lengths 0 .. 260: 1 to 5 blocks
    rows = [(c.msg, c.sig, c.key, c.code) for c in cases[::6]]   # valid, both digests
    rows += [(c.msg, c.sig, c.key, c.code) for c in cases[1::16]]  # parsable, wrong message
    g = cases[200]
    r, s = eo.der_decode(g.sig)
    x, y = eo.key_xy(g.key)
    for sig in (b'', g.sig[:-1], g.sig + b'\x00', eo.der_encode(0, s), eo.der_encode(r, N), b'\x30\x00'):
        rows.append((g.msg, sig, g.key, None))                               # no signature: never uploaded
    rows.append((g.msg, g.sig, b32(P) + b32(y), None))                       # coordinate = p: never uploaded
    rows.append((g.msg, g.sig, b32(x) + b32(2 ** 256 - 1), None))
    rows.append((g.msg, g.sig, g.key[:63], None))                            # no key: never submitted
    rows.append((g.msg, g.sig, b32(x) + b32((y + 1) % P), None))             # off the curve: uploaded, refused there
    rows.append((g.msg, g.sig, b32(x) + b32(P - y), None))                   # the negated key
    rows = [(m, sg, k, eo.verify(m, sg, k) if code is None else code) for m, sg, k, code in rows]
    assert 120 <= len(rows) <= 140 and {row[3] for row in rows} == {0, 1, 2}
    rng.shuffle(rows)
    up = [uploads(row[1], row[2]) for row in rows]
    assert 7 <= up.count(False) <= 9
    batch, sent = [], 0
    while sent < SET + 65:  # cycled until 2^18 + 65 rows go up
        j = len(batch) % len(rows)
        batch.append(rows[j])
        sent += up[j]
    assert len(batch) > sent == SET + 65
    signatures.reset_stats()
    t0 = time.perf_counter()
    got = signatures.verify_batch_digest([row[0] for row in batch], [row[1] for row in batch], [row[2] for row in batch])
    print('verify_batch_digest, %d rows (%d uploaded): %.2f s' % (len(batch), sent, time.perf_counter() - t0))
    bad = [(i, row[3], g) for i, (row, g) in enumerate(zip(batch, got)) if row[3] != g]
    assert not bad, (len(bad), bad[:5])
    st = signatures.stats()
    assert st['calls'] == 1 and st['submitted'] == sum(len(row[2]) == 64 for row in batch)
    assert st['uploaded'] == st['ladders'] == sent
    assert st['launches'] == 10  # five per set, two sets


def test_two_sets_in_one_digest_call(gpulib, comb):
    """2^18 + 1 digest rows: the last one is a set of its own."""
    keys, rs, digests = digest_rows([c.case for c in comb])
    idx = [j % len(comb) for j in range(SET + 1)]
    signatures.reset_stats()
    t0 = time.perf_counter()
    got = signatures.ecdsa_verify_digest([keys[j] for j in idx], [rs[j] for j in idx], [digests[j] for j in idx])
    print('ecdsa_verify_digest, %d rows: %.2f s' % (len(idx), time.perf_counter() - t0))
    bad = [(i, comb[j].name, g) for i, (j, g) in enumerate(zip(idx, got)) if comb[j].case.valid != g]
    assert not bad, (len(bad), bad[:5])
    st = signatures.stats()
    assert st['calls'] == 1 and st['submitted'] == st['uploaded'] == st['ladders'] == SET + 1
    assert st['launches'] == 8  # four per set, two sets
