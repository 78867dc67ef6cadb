"""Points chosen by their coordinates (no device): the constructors of ``oracle/ecdsa_oracle.py`` that
``tests/test_gpu_points.py`` runs on the device are pinned here to the reference-made fixture
``tests/golden/point_kats.json`` (tests/golden/make_point_golden.py), every family is shown from integers to be
what it says, the integer model of ``sg_comb_kernel`` with the second comparison of ``x_is_r`` or one of its two
guards taken out gets exactly one family wrong, and the host-only entry points are tried at the coordinate
boundaries n and p."""
import collections
import functools
import hashlib
import hmac
import struct

import pytest

from oracle import ecdsa_oracle as eo
from tests.test_ecdsa_oracle import HAS_RN, kernel_decide, kernel_point
from tests.test_gpu_sig_constructed import uploads

N, P = eo.N, eo.P
X_EDGE = 2 ** 32 + 977
# key coordinates at the two moduli: the first four are below p (n is no bound for a coordinate), the rest not
BELOW_P = (N - 1, N, N + 1, P - 1)
NOT_BELOW_P = (P, P + 1, 2 ** 256 - 2 ** 32, 2 ** 256 - 1)


def b32(v):
    return v.to_bytes(32, 'big')


@pytest.fixture(scope='module')
def kats(golden):
    return golden('point_kats.json')


# ------------------------------------------------------------------ the constructors
def test_lift_nearest_and_key_for():
    # what the curve has next to 0 and next to p
    assert [x for x in range(1, 14) if eo.lift_x(x)] == [1, 2, 3, 4, 6, 8, 12, 13]
    assert [d for d in range(1, 13) if eo.lift_x(P - d)] == [3, 4, 10, 12]
    assert [y for y in range(1, 18) if eo.lift_y(y)] == [1, 6, 11, 13, 17]
    assert eo.lift_x(0) is None and eo.lift_y(0) is None and eo.lift_x(P) is None and eo.lift_x(-1) is None
    assert eo.lift_x(5) is None and eo.lift_y(2) is None
    for v in (1, 2, 13, P - 3, N + 2, X_EDGE + 1):
        pt = eo.nearest(v)
        assert eo.on_curve(pt) and pt[0] >= v and pt[1] % 2 == 0 and all(eo.lift_x(x) is None for x in range(v, pt[0]))
        pt = eo.nearest(v, 1, 'y')
        assert eo.on_curve(pt) and pt[1] >= v and all(eo.lift_y(y) is None for y in range(v, pt[1]))
    assert eo.nearest(P - 1, -1)[0] == P - 3 and eo.nearest(5, -1)[0] == 4 and eo.nearest(2, -1, 'y')[1] == 1
    assert eo.lift_x(eo.GX) in (eo.G, eo.neg(eo.G)) and eo.lift_y(eo.GY)[1] == eo.GY
    # key_for: the verification computes exactly R
    R = eo.nearest(N + 1)
    r, s, e = R[0] - N, 12345, 2 ** 255 + 99
    Q = eo.key_for(R, r, s, e)
    w = pow(s, -1, N)
    assert eo.on_curve(Q) and eo.add(eo.mult_g(e * w % N), eo.mult(r * w % N, Q)) == R
    assert eo.verify_digest(Q, r, s, e) and not eo.verify_digest(Q, r, s, e + 1)


def test_coordinate_points_are_the_regions_they_name():
    pts = eo.coordinate_points()
    by = dict(pts)
    assert len(by) == len(pts) == 75 and len(set(by.values())) == 75 and all(eo.on_curve(pt) for pt in by.values())
    group = collections.Counter(name.rsplit('_', 2 if name.endswith('_neg') else 1)[0] for name in by)
    assert group == {'x_small': 10, 'x_large': 10, 'x_from_n': 5, 'x_in_n_p': 5, 'x_below_edge': 3, 'x_above_edge': 2,
                     'x_zero_bytes_1': 2, 'x_zero_bytes_2': 1, 'x_zero_bytes_4': 1, 'x_zero_bytes_8': 1, 'x_zero_bytes_15': 2,
                     'x_zero_bytes_16': 1, 'x_zero_bytes_24': 1, 'x_zero_bytes_31': 1, 'x_from_2_224': 2, 'x_from_2_255': 1,
                     'x_below_2_255': 1, 'y_small': 8, 'y_large': 8, 'y_from_n': 5, 'y_zero_bytes_1': 1, 'y_zero_bytes_8': 2,
                     'y_zero_bytes_16': 1, 'y_zero_bytes_31': 1}
    xs = lambda g: [by['%s_%d' % (g, j)][0] for j in range(8) if '%s_%d' % (g, j) in by]  # noqa: E731
    ys = lambda g: [by['%s_%d' % (g, j)][1] for j in range(8) if '%s_%d' % (g, j) in by]  # noqa: E731
    assert xs('x_small') == [1, 2, 3, 4, 6, 8, 12, 13] and xs('x_large')[:4] == [P - 3, P - 4, P - 10, P - 12]
    assert ys('y_small')[:5] == [1, 6, 11, 13, 17] and all(P - 64 < y < P for y in ys('y_large'))
    assert all(N < x < N + 64 for x in xs('x_from_n')) and all(N <= x < P for x in xs('x_in_n_p')) and len(xs('x_in_n_p')) == 4
    assert all(N <= y < N + 64 for y in ys('y_from_n')) and len(ys('y_from_n')) == 4
    assert all(X_EDGE - 64 < x < X_EDGE for x in xs('x_below_edge')) and all(X_EDGE <= x < X_EDGE + 64 for x in xs('x_above_edge'))
    for z in eo.X_ZERO_BYTES:
        assert len(b32(by['x_zero_bytes_%d_0' % z][0]).lstrip(b'\x00')) == 32 - z
    for z in eo.Y_ZERO_BYTES:
        assert len(b32(by['y_zero_bytes_%d_0' % z][1]).lstrip(b'\x00')) == 32 - z
    assert 0 <= by['x_from_2_224_0'][0] - 2 ** 224 < 64 and 0 <= by['x_from_2_255_0'][0] - 2 ** 255 < 64
    assert 0 < 2 ** 255 - by['x_below_2_255_0'][0] < 64
    negs = [name for name in by if name.endswith('_neg')]
    assert len(negs) == 12 and all(by[name] == eo.neg(by[name[:-4]]) for name in negs)
    off = eo.off_curve_points()
    assert len(off) == 8 and not any(eo.on_curve(pt) for _, pt in off) and all(max(pt) < P for _, pt in off)


def test_rn_families_are_what_they_say():
    cases = eo.rn_cases()
    count = collections.Counter((c.family, c.role, c.valid) for c in cases)
    assert count == {('x_above_n', 'row', True): 24, ('x_above_n', 'mutant_r', False): 24, ('x_above_n', 'mutant_e', False): 24,
                     ('rn_reaches_p', 'row', False): 16, ('rn_reaches_p', 'sibling', True): 16,
                     ('rn_carries', 'row', False): 16, ('rn_carries', 'sibling', True): 16}
    assert len({c.name for c in cases}) == len(cases) == 136
    rows = {c.name: c for c in cases}
    for c in cases:
        assert eo.on_curve(c.R) and eo.on_curve(c.Q) and 1 <= c.r < N and 1 <= c.s < N, c.name  # every row reaches the device
        assert c.valid == eo.verify_digest(c.Q, c.r, c.s, c.e), c.name
        x = c.R[0]
        if c.role in ('row', 'sibling'):  # the verification computes exactly R
            w = pow(c.s, -1, N)
            assert eo.add(eo.mult_g(c.e % N * w % N), eo.mult(c.r * w % N, c.Q)) == c.R, c.name
        if c.role == 'sibling':
            bad = rows[c.name[:-len('_sibling')]]
            assert (c.R, c.s, c.e, c.r) == (bad.R, bad.s, bad.e, x) and not bad.valid and c.valid
        elif c.role != 'row':
            good = rows[c.name[:c.name.index('_mutant')]]
            assert c.Q == good.Q and c.s == good.s and (c.r, c.e) in ((good.r + 1, good.e), (good.r, good.e ^ 1))
        elif c.family == 'x_above_n':
            assert N < x < P and c.r == x - N and c.r + N < P
        elif c.family == 'rn_reaches_p':
            assert x < X_EDGE and c.r == x + P - N and P <= c.r + N < 2 ** 256
        else:
            assert x < 2 * N - 2 ** 256 and c.r == x + 2 ** 256 - N and c.r + N >= 2 ** 256 and (c.r + N) % 2 ** 256 == x
    above = [c for c in cases if c.family == 'x_above_n' and c.role == 'row']
    assert [c.r for c in above[:8]] == [c.R[0] - N for c in above[:8]] and above[0].r == 2 and all(c.r < 64 for c in above[:8])
    assert all(P - c.R[0] < 64 for c in above[8:16])
    assert all(len(eo.der_encode(c.r, c.s)) <= 6 + 1 + 33 for c in above[:8])  # a 1-byte INTEGER r
    reach = [c.R[0] for c in cases if c.family == 'rn_reaches_p' and c.role == 'row']
    assert reach[:6] == [1, 2, 3, 4, 6, 8] and all(X_EDGE - 64 < x < X_EDGE for x in reach[6:11])
    carry = [c.R[0] for c in cases if c.family == 'rn_carries' and c.role == 'row']
    assert carry[:6] == [1, 2, 3, 4, 6, 8] and all(abs(x - X_EDGE) < 64 for x in carry[6:10])
    assert all(2 ** 254 <= x < 2 ** 255 for x in carry[10:])


def test_rn_message_rows_and_the_fixture(kats):
    """The oracle's code for every message-level row, the family's expectation (1, 2 and 0) and the reference's
    own ``ECC.verify`` under both digests."""
    cases = eo.rn_msg_cases()
    assert [v['name'] for v in kats['verify']] == [c.name for c in cases]
    count = collections.Counter()
    for c, v in zip(cases, kats['verify']):
        assert (c.msg.hex(), c.sig.hex(), c.key.hex()) == (v['msg'], v['sig'], v['key']), c.name
        ref = 1 if v['sha1'] else 2 if v['sha256'] else 0
        assert c.code == eo.verify(c.msg, c.sig, c.key) == ref, c.name
        honest = c.family == 'x_above_n' or c.name.endswith('_sibling')
        assert c.code == ((1 if c.alg == 'sha1' else 2) if honest else 0), c.name
        assert uploads(c.sig, c.key) and len(c.msg) <= 200, c.name
        count[c.family, c.name.endswith('_sibling'), c.code] += 1
    assert count == {('x_above_n', False, 1): 4, ('x_above_n', False, 2): 4,
                     ('rn_reaches_p', False, 0): 8, ('rn_reaches_p', True, 1): 4, ('rn_reaches_p', True, 2): 4,
                     ('rn_carries', False, 0): 8, ('rn_carries', True, 1): 4, ('rn_carries', True, 2): 4}
    # r = 2, ...: the shortest DER there is goes through the reference's parser and the oracle's
    assert min(len(c.sig) for c in cases if c.family == 'x_above_n') <= 40
    assert eo.der_decode(eo.der_encode(2, 1)) == (2, 1) and len(eo.der_encode(2, 1)) == 8


def test_key_ecdh_and_shared_cases(kats):
    pts = eo.coordinate_points()
    keys = eo.key_cases()
    assert collections.Counter((c.family, c.valid) for c in keys) == {('key', True): 75, ('key_mutant', False): 75}
    assert [c.Q for c in keys[::2]] == [pt for _, pt in pts] and all(1 <= c.r < N and 1 <= c.s < N for c in keys)
    assert all(a.Q == b.Q and (a.r, a.s, a.e + 1) == (b.r, b.s, b.e) for a, b in zip(keys[::2], keys[1::2]))
    ecdh, shared = eo.ecdh_cases(), eo.shared_cases()
    assert len(ecdh) == len(shared) == 4 * 75
    assert [c.R for c in ecdh[::4]] == [pt for _, pt in pts]
    assert [c.x for c in shared] == [pt[0] for _, pt in pts for _ in range(4)]
    V = set(eo.scalar_set())
    assert all(c.k in V and eo.on_curve(c.R) for c in ecdh + shared)
    assert sum(c.x < 2 ** 192 for c in shared) >= 4 * 20  # shared secrets with 8 or more leading zero bytes
    assert sum(c.x >= N for c in shared) >= 4 * 8         # and in [n, p)
    # the reference's raw_get_ecdh_key on stripped coordinates: the first key of every point
    rows = kats['ecdh']
    assert collections.Counter(r['family'] for r in rows) == {'ecdh': 75, 'shared': 75}
    for r, c in zip(rows, ecdh[::4] + shared[::4]):
        assert r['name'] == c.name and int(r['key'], 16) == c.k and (int(r['x'], 16), int(r['y'], 16)) == c.R
        assert bytes.fromhex(r['shared_x']) == b32(c.x), r['name']  # 32 bytes, leading zeros kept
        assert not r['x'].startswith('00') and not r['y'].startswith('00')
    assert min(len(r['x']) for r in rows) == 2 and min(len(r['y']) for r in rows) == 2
    for c in shared[1::4]:
        assert eo.mult(c.k, c.R)[0] == c.x, c.name


def test_fixture_blobs_against_the_oracle(kats):
    """Every blob of the fixture restated with hashlib / hmac from the oracle's shared x."""
    from pybitmessage_amd import ecies
    blobs = kats['blobs']
    keys = [int(k, 16) for k in kats['recipient_keys']]
    assert len(blobs) == 16 and [b['spoiled'] for b in blobs[12:]] == ['mac', 'mac', 'x_plus_p', 'x_plus_p']
    assert [tuple(b['coord_lens']) for b in blobs[:7]] == [(1, 32), (2, 32), (17, 32), (31, 32), (32, 1), (32, 16), (1, 32)]
    assert sum(b['shared_x'].startswith('00' * 8) for b in blobs[:12]) >= 4
    for b in blobs:
        blob = bytes.fromhex(b['blob'])
        xl, yl = b['coord_lens']
        x, y, off = ecies.parse(blob)
        assert off == 22 + xl + yl and (len(blob) - off - 32) % 16 == 0
        R = (int.from_bytes(x, 'big'), int.from_bytes(y, 'big'))
        assert eo.on_curve(R) and R[0] == int.from_bytes(blob[20:20 + xl], 'big') % P
        sx = eo.mult(keys[b['recipient']], R)[0]
        assert b32(sx).hex() == b['shared_x']
        mac = hmac.new(hashlib.sha512(b32(sx)).digest()[32:], blob[:-32], hashlib.sha256).digest()
        assert (mac == blob[-32:]) == b['match'] == (b['outcome'] == 'decrypted'), b['name']
        assert b['match'] == (b['spoiled'] != 'mac')  # the reference reduces a 33-byte x + p: that blob still opens
        if b['match']:
            assert b['plaintext'] == b['sent']
            assert ecies.decrypt(blob, hashlib.sha512(b32(sx)).digest()[:32]).hex() == b['sent'], b['name']


# ------------------------------------------------------------------ the GPU tests can fail
Row = collections.namedtuple('Row', 'name family u1 u2 case')


def as_row(c, family=None):
    w = pow(c.s, -1, N)
    return Row(c.name, family or c.family, c.e % N * w % N, c.r * w % N, c)


@functools.lru_cache(maxsize=None)
def modelled():
    """(row, verdict of the oracle, the kernel's point) for every new digest-level row and the comb's own."""
    rows = [as_row(c, c.family if c.role == 'row' else c.family + '_' + c.role) for c in eo.rn_cases()]
    rows += [as_row(c) for c in eo.key_cases()]
    rows += [Row(c.name, 'comb', c.u1, c.u2, c.case) for c in eo.comb_cases() if c.role in ('hit', 'scaled')]
    return [(row, row.case.valid, kernel_point(row)) for row in rows]


def test_a_kernel_without_the_second_comparison_or_a_guard_gets_its_family_wrong():
    wrong = {how: [row for row, valid, acc in modelled() if kernel_decide(acc, row.case.r, how) != valid] for how in HAS_RN}
    assert len(modelled()) == 136 + 150 + 256
    assert wrong['as_is'] == []  # the model of the kernel as it is decides every row as the oracle does
    for how, family, n in (('never', 'x_above_n', 24), ('no_carry_guard', 'rn_carries', 16),
                           ('no_canonical_guard', 'rn_reaches_p', 16)):
        assert [row.family for row in wrong[how]] == [family] * n, how  # the whole family, and nothing else
    assert not any(row.case.valid for row in wrong['no_carry_guard'] + wrong['no_canonical_guard'])  # accepted, wrongly
    assert all(row.case.valid for row in wrong['never'])  # refused, wrongly


# ------------------------------------------------------------------ host-only entry points at n and p
def test_upload_rule_and_the_walk_at_the_coordinate_boundaries(golden):
    """A key coordinate is compared with p, never with n: the host rule of ``signatures`` as the GPU tests
    restate it (``uploads``) and ``receive.walk_msg``'s ``verifiable`` (the same ``coord_in_range`` the
    upload of every receive path goes through)."""
    from pybitmessage_amd import receive
    from pybitmessage_amd.ecies import _varint
    m = next(m for m in golden('rx_kats.json')['msgs'] if m['line'] is None)
    obj, plain, ripe = bytes.fromhex(m['obj']), bytes.fromhex(m['plaintext']), bytes.fromhex(m['toRipe'])
    ver = _varint(plain[:10])
    at = ver[1] + _varint(plain[ver[1]:ver[1] + 10])[1] + 4  # the signing key's X || Y
    res, verifiable = receive.walk_msg(obj, plain, ripe)
    assert verifiable and int(res.status[0]) == receive.OK
    sig = res.signature(0)
    seen = collections.Counter()
    for v in BELOW_P + NOT_BELOW_P + (0, 1, 2 ** 255):
        for where in (0, 32):
            changed = plain[:at + where] + b32(v) + plain[at + where + 32:]
            res, verifiable = receive.walk_msg(obj, changed, ripe)
            assert int(res.status[0]) == receive.OK  # the walk reads no key
            assert verifiable == (v < P) == uploads(sig, changed[at:at + 64]), (hex(v), where)
            seen[verifiable] += 1
    assert seen == {True: 14, False: 8}


def payload(xb, yb, body=b'\x07' * 16):
    return b'\x24' * 16 + struct.pack('!HH', 714, len(xb)) + xb + struct.pack('!H', len(yb)) + yb + body + b'\x5a' * 32


def test_parse_reduces_coordinates_of_every_length():
    """``ecies.parse``: X and Y of 1 to 33 bytes, values at n, at p and at the top of each length; the
    coordinates come back mod p (as the reference opens the fixture's ``x_plus_p``) and the body starts at
    22 + len X + len Y."""
    from pybitmessage_amd import ecies
    values = set(BELOW_P + NOT_BELOW_P + (0, 1, 2 * P - 1, 2 * P, 2 * P + 1, 2 ** 264 - 1, 255 * P, 255 * P + 1))
    for ln in range(1, 34):
        values |= {2 ** (8 * ln) - 1, 2 ** (8 * ln - 1), 2 ** (8 * (ln - 1)), 2 ** (8 * ln) - 2 ** (8 * (ln - 1))}
    values = sorted(v for v in values if v < 2 ** 264)
    full = b32(eo.GY)
    n = 0
    for v in values:
        shortest = max(1, (v.bit_length() + 7) // 8)
        for ln in sorted({shortest, min(shortest + 1, 33), 32, 33}):
            if ln < shortest:
                continue
            vb = v.to_bytes(ln, 'big')
            for xb, yb in ((vb, full), (full, vb), (vb, vb)):
                got = ecies.parse(payload(xb, yb))
                want = (b32(int.from_bytes(xb, 'big') % P), b32(int.from_bytes(yb, 'big') % P), 22 + len(xb) + len(yb))
                assert got == want, (hex(v), ln)
                n += 1
    assert n >= 1000
    for v in BELOW_P:
        assert ecies.parse(payload(b32(v), full))[0] == b32(v)  # untouched: n is no bound for a coordinate
    for v in NOT_BELOW_P:
        assert ecies.parse(payload(b32(v), full))[0] == b32(v - P)
    for xl in range(1, 34):
        for yl in (1, 2, 31, 32, 33, xl):
            for body in (b'', b'\x01' * 16):
                xb, yb = b'\x81' * xl, b'\x7f' * yl
                assert ecies.parse(payload(xb, yb, body)) == (b32(int.from_bytes(xb, 'big') % P), b32(int.from_bytes(yb, 'big') % P),
                                                              22 + xl + yl)
            assert ecies.parse(payload(b'\x81' * xl, b'\x7f' * yl)[:22 + xl + yl + 31]) is None  # no room for the MAC
