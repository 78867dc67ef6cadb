"""The curve kernels on points chosen by their coordinates -- points with an unknown discrete logarithm, which
no scalar a test picks ever gives: x(R) in [n, p), where ``x_is_r`` (csrc/bmpow_sig.hip) needs its second
comparison X = (r + n) Z^2, and the two r that only its guards refuse; coordinates next to 0, next to p, in
[n, p) and with many leading zero bytes as the key Q, as a blob's ephemeral point and as the shared secret
itself; wire coordinates down to one byte.  Every expectation is the oracle's (``oracle/ecdsa_oracle.py``) or
the reference-made fixture's (``tests/golden/point_kats.json``), both pinned by ``tests/test_point_oracle.py``,
which also shows from integers that a kernel without the comparison or without a guard fails here."""
import collections
import ctypes
import hashlib
import hmac
import random
import struct

import pytest

from oracle import ecdsa_oracle as eo
from pybitmessage_amd import ecies, receive, sender, signatures
from tests.conftest import load_golden
from tests.test_gpu_sig_constructed import digest_rows, uploads
from tests.test_point_oracle import BELOW_P, NOT_BELOW_P

pytestmark = pytest.mark.gpu

N, P = eo.N, eo.P


def b32(v):
    return v.to_bytes(32, 'big')


def strip(v):
    """As ``BN_bn2bin`` leaves a number."""
    return b32(v).lstrip(b'\x00')


@pytest.fixture(scope='module')
def kats():
    return load_golden('point_kats.json')


@pytest.fixture(scope='module')
def rn():
    return list(eo.rn_cases())


def check(cases, got, want='valid'):
    """Every row decided as the oracle decides it; a failure names how many rows of which family are not."""
    bad = [(c, g) for c, g in zip(cases, got) if getattr(c, want) != g]
    families = sorted(collections.Counter(c.family for c, _ in bad).items())
    assert not bad, (len(bad), families, [(c.name, getattr(c, want), g) for c, g in bad[:5]])


def verify_all_uploaded(cases):
    """One ``ecdsa_verify_digest`` call in which every row reaches the device: the verdicts are the kernel's."""
    signatures.reset_stats()
    got = signatures.ecdsa_verify_digest(*digest_rows(cases))
    st = signatures.stats()
    assert st['calls'] == 1 and st['submitted'] == st['uploaded'] == st['ladders'] == len(cases)
    return got


# ------------------------------------------------------------------ 1. x(R) at and above n
def test_rn_cases_in_one_call(gpulib, rn):
    check(rn, verify_all_uploaded(rn))
    count = collections.Counter((c.family, c.role, c.valid) for c in rn)
    assert count == {('x_above_n', 'row', True): 24, ('x_above_n', 'mutant_r', False): 24, ('x_above_n', 'mutant_e', False): 24,
                     ('rn_reaches_p', 'row', False): 16, ('rn_reaches_p', 'sibling', True): 16,
                     ('rn_carries', 'row', False): 16, ('rn_carries', 'sibling', True): 16}


def test_rn_cases_shuffled_and_across_a_wave_boundary(gpulib, rn):
    """The whole set shuffled, and 65 rows (a wave and a lane): a dozen rows of each family among ordinary
    signatures and their mutants."""
    mixed = rn[:]
    random.Random(41).shuffle(mixed)
    check(mixed, verify_all_uploaded(mixed))
    part = [c for c in rn if c.role in ('row', 'sibling')][::2][:40]
    part += [c for c in eo.scalar_cases() if c.family in ('u2', 'u2_mutant')][:25]
    random.Random(42).shuffle(part)
    assert len(part) == 65
    count = collections.Counter((c.family, getattr(c, 'role', 'row')) for c in part[:64])
    assert min(count['x_above_n', 'row'], count['rn_reaches_p', 'row'], count['rn_carries', 'row'], count['u2', 'row']) >= 7
    check(part, verify_all_uploaded(part))


def test_rn_message_rows(gpulib, kats):
    """The message-level rows through the hashing pass and the DER parse (a one-byte r among them): the codes
    are the oracle's and the reference's own ``ECC.verify``."""
    cases = list(eo.rn_msg_cases())
    ref = [1 if v['sha1'] else 2 if v['sha256'] else 0 for v in kats['verify']]
    assert [c.code for c in cases] == ref and all(uploads(c.sig, c.key) for c in cases)
    assert collections.Counter((c.family, c.code) for c in cases) == {
        ('x_above_n', 1): 4, ('x_above_n', 2): 4, ('rn_reaches_p', 0): 8, ('rn_reaches_p', 1): 4, ('rn_reaches_p', 2): 4,
        ('rn_carries', 0): 8, ('rn_carries', 1): 4, ('rn_carries', 2): 4}
    for order in (list(range(len(cases))), random.Random(43).sample(range(len(cases)), len(cases))):
        rows = [cases[i] for i in order]
        signatures.reset_stats()
        got = signatures.verify_batch_digest([c.msg for c in rows], [c.sig for c in rows], [c.key for c in rows])
        check(rows, got, 'code')
        st = signatures.stats()
        assert st['submitted'] == st['uploaded'] == st['ladders'] == len(rows)
    assert min(len(c.sig) for c in cases) <= 40


# ------------------------------------------------------------------ 2. the key chosen by its coordinates
def test_keys_chosen_by_their_coordinates(gpulib):
    cases = list(eo.key_cases())
    check(cases, verify_all_uploaded(cases))
    assert collections.Counter((c.family, c.valid) for c in cases) == {('key', True): 75, ('key_mutant', False): 75}
    # a coordinate is compared with p, never with n: n - 1 .. p - 1 go up (and are refused there, being off the
    # curve), p .. 2^256 - 1 never do
    base = cases[0]
    edge = [base._replace(name='%s_%x' % ('xy'[i], v), Q=(v, base.Q[1]) if i == 0 else (base.Q[0], v), valid=False)
            for v in BELOW_P + NOT_BELOW_P for i in (0, 1)]
    assert not any(eo.verify_digest(c.Q, c.r, c.s, c.e) for c in edge)
    rows = cases[:40] + edge + cases[40:65]
    signatures.reset_stats()
    keys = [b32(c.Q[0]) + b32(c.Q[1]) for c in rows]
    got = signatures.ecdsa_verify_digest(keys, *digest_rows(rows)[1:])
    check(rows, got)
    st = signatures.stats()
    assert st['submitted'] == len(rows) == 81 and st['uploaded'] == 65 + 8 == sum(max(c.Q) < P for c in rows)


# ------------------------------------------------------------------ 3. ECDH
@pytest.fixture(scope='module')
def ecdh_rows():
    """(key, point, x or None): every point as R and as the shared point, the same with y negated, and the
    off-curve companions."""
    rows = [(c.k, c.R, c.x) for c in eo.ecdh_cases() + eo.shared_cases()]
    rows += [(k, eo.neg(R), x) for k, R, x in rows]
    V = eo.scalar_set()
    rows += [(V[j], pt, None) for _, pt in eo.off_curve_points() for j in (0, 3, 100, 700)]
    assert len(rows) == 1200 + 32
    return rows


def test_ecdh_full_width_and_stripped(gpulib, kats, ecdh_rows):
    want = [None if x is None else b32(x) for _, _, x in ecdh_rows]
    assert sum(w is not None and w[:8] == bytes(8) for w in want) >= 160 and sum(w is not None and w >= b32(N) for w in want) >= 64
    for enc in (b32, strip):
        got = ecies.ecdh([enc(k) for k, _, _ in ecdh_rows], [(enc(R[0]), enc(R[1])) for _, R, _ in ecdh_rows])
        assert got == want, [i for i, (g, w) in enumerate(zip(got, want)) if g != w][:10]
    assert min(len(strip(R[0])) for _, R, _ in ecdh_rows) == 1 and min(len(strip(R[1])) for _, R, _ in ecdh_rows) == 1
    # the reference's raw_get_ecdh_key on the stripped coordinates
    rows = kats['ecdh']
    got = ecies.ecdh([bytes.fromhex(r['key']) for r in rows], [(bytes.fromhex(r['x']), bytes.fromhex(r['y'])) for r in rows])
    assert got == [bytes.fromhex(r['shared_x']) for r in rows] and len(rows) == 150


def test_ecdh_ok_flags_of_the_raw_call(gpulib, ecdh_rows):
    rows = ecdh_rows[::7] + ecdh_rows[-32:]
    n = len(rows)
    out, ok = ctypes.create_string_buffer(32 * n), ctypes.create_string_buffer(n)
    u8 = ctypes.POINTER(ctypes.c_uint8)
    priv = b''.join(b32(k) for k, _, _ in rows)
    pub = b''.join(b32(R[0]) + b32(R[1]) for _, R, _ in rows)
    assert gpulib.bmpow_ecdh(n, priv, pub, ctypes.cast(out, u8), ctypes.cast(ok, u8)) == 0
    assert list(ok.raw) == [int(x is not None) for _, _, x in rows] and list(ok.raw).count(0) >= 32
    assert out.raw == b''.join(bytes(32) if x is None else b32(x) for _, _, x in rows)


# ------------------------------------------------------------------ 4. the fixture's blobs
def test_fixture_blobs_match_and_decrypt(gpulib, kats):
    keys = [bytes.fromhex(k) for k in kats['recipient_keys']]
    blobs = [bytes.fromhex(b['blob']) for b in kats['blobs']]
    want = [b['recipient'] if b['match'] else None for b in kats['blobs']]
    assert want.count(None) == 2 and [b['spoiled'] for b in kats['blobs'] if not b['match']] == ['mac', 'mac']
    assert ecies.match_keys(blobs, keys) == want
    assert ecies.match_keys(blobs, [k.lstrip(b'\x00') for k in keys]) == want
    plains = [(b['recipient'], bytes.fromhex(b['plaintext'])) if b['match'] else None for b in kats['blobs']]
    assert ecies.decrypt_batch(blobs, keys) == plains
    assert sorted(len(p[1]) for p in plains[:7]) == [0, 1, 15, 16, 17, 40, 100]


def test_fixture_blobs_among_ordinary_rows(gpulib, kats):
    """One launch with key headers of 55 to 87 bytes: the by-coordinate blobs shuffled among the reference's own."""
    old = load_golden('ecies_kats.json')
    keys = [bytes.fromhex(k) for k in old['recipient_keys']] + [bytes.fromhex(k) for k in kats['recipient_keys']]
    rows = [(bytes.fromhex(m['blob']), (m['recipient'], bytes.fromhex(m['plaintext']))) for m in old['msg_kats']]
    rows += [(bytes.fromhex(b['blob']), (3 + b['recipient'], bytes.fromhex(b['plaintext'])) if b['match'] else None)
             for b in kats['blobs']]
    random.Random(44).shuffle(rows)
    heads = {ecies.parse(blob)[2] for blob, _ in rows}
    assert {55, 56, 71, 85, 86, 87} <= heads and min(heads) == 55
    assert ecies.decrypt_batch([blob for blob, _ in rows], keys) == [w for _, w in rows]
    assert ecies.match_keys([blob for blob, _ in rows], keys) == [None if w is None else w[0] for _, w in rows]


# ------------------------------------------------------------------ 5. sealed objects under short ephemeral points
SHORT = ('x_small_0', 'x_below_edge_0', 'x_zero_bytes_24_0', 'x_zero_bytes_15_0', 'x_zero_bytes_1_0', 'y_small_0',
         'y_zero_bytes_16_0', 'y_zero_bytes_8_0')
SHORT_LENS = [(1, 32), (5, 32), (8, 32), (17, 32), (31, 32), (32, 1), (32, 16), (32, 24)]


def reseal(plain, priv, R, iv):
    """The ECIES blob of ``plain`` to the holder of ``priv`` under the ephemeral point R, its coordinates written
    as ``BN_bn2bin`` leaves them: the key from the oracle's shared x, AES by the library's raw CBC call, the
    MAC by hmac."""
    key = hashlib.sha512(b32(eo.mult(int.from_bytes(priv, 'big'), R)[0])).digest()
    X, Y = strip(R[0]), strip(R[1])
    body = iv + struct.pack('!HH', 714, len(X)) + X + struct.pack('!H', len(Y)) + Y
    body += ecies.aes_cbc_batch([key[:32]], [iv], [plain])[0]
    return body + hmac.new(key[32:], body, hashlib.sha256).digest()


def short_points():
    pts = dict(eo.coordinate_points())
    out = [pts[name] for name in SHORT]
    assert [(len(strip(x)), len(strip(y))) for x, y in out] == SHORT_LENS
    return out


def test_sealed_msgs_under_short_ephemeral_points(gpulib):
    from tests import test_gpu_rxopen as rxo
    from tests.test_gpu_rx import compose, row
    rng = random.Random(45)
    privs = [bytes(rng.randrange(1, 256) for _ in range(32)) for _ in range(16)]
    pubs = sender.priv_to_pub(privs)
    senders = [(privs[2 * i], pubs[2 * i][1:], pubs[2 * i + 1][1:]) for i in range(8)]
    mine = [bytes(rng.randrange(1, 256) for _ in range(32)) for _ in range(2)]
    ripes = [hashlib.sha1(b'ripe of key %d' % i).digest() for i in range(2)]
    rows = [row(600 + k, to_ripe=ripes[k % 2], message=bytes([k + 1]) * (0, 1, 15, 16, 17, 200, 31, 500)[k],
                alg=('sha1', 'sha256')[k % 2], version=(3, 4)[k // 4]) for k in range(8)]
    msgs, _ = compose(rows, senders)
    objs = [o[:-rxo.TAIL] + reseal(plain, mine[k % 2], R, bytes(rng.randrange(256) for _ in range(16)))
            for k, ((o, plain), R) in enumerate(zip(msgs, short_points()))]
    plans = [receive.sealed_plan(o) for o in objs]
    assert all(p[0] for p in plans) and [p[3] for p in plans] == [22 + xl + yl for xl, yl in SHORT_LENS]
    got = rxo.assert_equals_composition(objs, ripes, mine)
    assert got.status.tolist() == [receive.OK] * 8 and got.match.tolist() == [0, 1] * 4
    assert [got.plaintexts[i] for i in range(8)] == [p for _, p in msgs]
    assert [got.message(i) for i in range(8)] == [r['message'] for r in rows]


def test_sealed_broadcasts_under_short_ephemeral_points(gpulib):
    from tests import test_gpu_rxobjopen as roo
    rng = random.Random(46)
    privs = [bytes(rng.randrange(1, 256) for _ in range(32)) for _ in range(16)]
    pubs = sender.priv_to_pub(privs)
    senders = [(privs[2 * i], pubs[2 * i][1:], pubs[2 * i + 1][1:]) for i in range(8)]
    rows = [roo.row(700 + k, roo.BROADCAST, bv=5, stream=50 + k, message=bytes([k + 1]) * (0, 1, 15, 16, 17, 200, 31, 500)[k],
                    alg=('sha1', 'sha256')[k % 2]) for k in range(8)]
    kinds, sealed, addrs, keys = roo.sealed(rows, senders)
    made = roo.compose(rows, senders)
    assert [m[1][:-roo.TAIL] for m in made] == [o[:len(m[1]) - roo.TAIL] for m, o in zip(made, sealed)]  # the same heads
    objs = [m[1][:-roo.TAIL] + reseal(m[2], key, R, bytes(rng.randrange(256) for _ in range(16)))
            for m, key, R in zip(made, keys, short_points())]
    assert [ecies.parse(o[len(m[1]) - roo.TAIL:])[2] for m, o in zip(made, objs)] == [22 + xl + yl for xl, yl in SHORT_LENS]
    subs, _ = roo.tables_for(rows, addrs)
    got = roo.assert_equals_composition(kinds, objs, subs)
    assert got.status.tolist() == [receive.OBJ_OK] * 8 and got.accepted() == list(range(8))
    assert [got.plaintexts[i] for i in range(8)] == [m[2] for m in made]
    assert [got.message(i) for i in range(8)] == [r['message'] for r in rows]
    assert receive.open_sealed_broadcasts(objs, subs).recs.tobytes() == got.recs.tobytes()


# ------------------------------------------------------------------ 6. sealing to keys chosen by their coordinates
@pytest.mark.parametrize('mode', [1, 0], ids=['device_seal', 'host_seal'])
def test_encrypt_to_keys_chosen_by_their_coordinates(gpulib, mode):
    rng = random.Random(47)
    V = eo.scalar_set()
    keys = [pt for _, pt in eo.coordinate_points()] + [pt for _, pt in eo.off_curve_points()]
    n = len(keys)
    eph = [V[rng.randrange(len(V))] for _ in range(n)]
    ivs = [bytes(rng.randrange(256) for _ in range(16)) for _ in range(n)]
    plains = [bytes(rng.randrange(256) for _ in range(j % 50)) for j in range(n)]
    prev = sender.set_seal(mode)
    try:
        blobs = sender.encrypt_batch(plains, [eo.xy_key(q) for q in keys], ephemeral=[b32(k) for k in eph], ivs=ivs)
    finally:
        sender.set_seal(prev)
    assert [b is None for b in blobs] == [False] * 75 + [True] * 8
    key_e, bodies = [], []
    for j in range(75):
        R = eo.mult_g(eph[j])
        X, Y = strip(R[0]), strip(R[1])
        head = ivs[j] + struct.pack('!HH', 714, len(X)) + X + struct.pack('!H', len(Y)) + Y
        blob = blobs[j]
        assert blob[:len(head)] == head, j
        key = hashlib.sha512(b32(eo.mult(eph[j], keys[j])[0])).digest()
        assert hmac.new(key[32:], blob[:-32], hashlib.sha256).digest() == blob[-32:], j
        key_e.append(key[:32])
        bodies.append(blob[len(head):-32])
    assert ecies.aes_cbc_batch(key_e, ivs[:75], bodies, decrypt=True) == plains[:75]
