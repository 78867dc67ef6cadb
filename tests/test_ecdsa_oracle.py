"""``oracle/ecdsa_oracle.py`` earns its trust (no device): against every reference-made row of
``tests/golden/sig_kats.json`` and ``ecies_kats.json``, against ``oracle/addrgen_oracle.py``, and against
itself -- every constructed family that ``tests/test_gpu_sig_constructed.py`` runs on the device is shown
here, from integers alone, to reach the branch of the kernel's comb it was built for, and a field-level
model of that comb with a branch taken out gets constructed cases wrong."""
import collections
import functools
import random

import pytest

from oracle import addrgen_oracle
from oracle import ecdsa_oracle as eo

N, P = eo.N, eo.P


@pytest.fixture(scope='module')
def kats(golden):
    return golden('sig_kats.json')


# ------------------------------------------------------------------ against the reference's fixtures
def test_verify_reproduces_every_fixture_case(kats):
    seen = collections.Counter()
    for k in kats['cases']:
        got = eo.verify(bytes.fromhex(k['msg']), bytes.fromhex(k['sig']), bytes.fromhex(k['key']))
        assert got == k['code'], k['name']
        seen[got] += 1
    assert seen[1] >= 12 and seen[2] >= 12 and seen[0] >= 20
    n = 0
    for o in kats['pubkey_objects'] + kats['msg_objects']:
        if o['parts']:
            p = o['parts']
            got = eo.verify(bytes.fromhex(p['signed']), bytes.fromhex(p['sig']), bytes.fromhex(p['key']))
            want = 0 if not o['verdict'] else 1 if o['name'].endswith('sha1') else 2
            assert got == want, o['name']
            n += 1
    assert n >= 6


def test_verify_digest_reproduces_every_digest_case(kats):
    for k in kats['digest_cases']:
        got = eo.verify_digest(eo.key_xy(bytes.fromhex(k['key'])), int(k['r'], 16), int(k['s'], 16), int(k['e'], 16))
        assert got == k['valid'], k['name']
    assert sum(k['valid'] for k in kats['digest_cases']) >= 6


def test_mult_reproduces_every_shared_x(golden):
    e = golden('ecies_kats.json')['ecdh_kats']
    n = 0
    for p, row in zip(e['points'], e['shared_x']):
        pt = (int(p['x'], 16), int(p['y'], 16))
        assert eo.on_curve(pt)
        for k, sx in zip(e['keys'], row):
            assert eo.mult(int(k, 16), pt)[0] == int(sx, 16)
            n += 1
    assert n == len(e['points']) * len(e['keys']) >= 150


def test_mult_g_against_the_address_oracle():
    rng = random.Random(3)
    V = eo.scalar_set()
    structured = V[:len(V) - 300]  # everything but V's own random tail
    assert len(structured) == 7 + 102 + 126 + 200
    for k in structured + [rng.randrange(1, N) for _ in range(50)]:
        assert eo.mult_g(k) == addrgen_oracle.point_mult_xy(k), hex(k)
    assert eo.mult_g(0) is None and eo.mult_g(N) is None and eo.mult(N, eo.G) is None
    assert eo.mult_g(N + 5) == eo.mult_g(5) == eo.mult(5, eo.G)
    for k in V[::40]:
        assert eo.mult(k, eo.G) == eo.mult_g(k)
        q = eo.mult_g(k)
        assert eo.on_curve(q) and not eo.on_curve((q[0], (q[1] + 1) % P)) and not eo.on_curve((q[0] + P, q[1]))
        assert eo.add(q, eo.neg(q)) is None and eo.add(q, q) == eo.mult_g(2 * k) and eo.add(q, None) == q


def test_der_and_the_constructors_agree_with_verify_digest():
    rng = random.Random(4)
    for _ in range(20):
        d, k, e = rng.randrange(1, N), rng.randrange(1, N), rng.getrandbits(256)
        r, s = eo.sign(d, k, e)
        assert eo.der_decode(eo.der_encode(r, s)) == (r, s)
        assert eo.verify_digest(eo.mult_g(d), r, s, e) and not eo.verify_digest(eo.mult_g(d), r, s, e ^ 1)
        c = eo.from_s(k, s, e)
        assert c.Q == eo.mult_g(d) and (c.r, c.s, c.e, c.valid) == (r, s, e, True)
    for r, s in ((1, 1), (0x7F, 0x80), (N - 1, N - 1), (2 ** 255, 2 ** 248 - 1)):
        enc = eo.der_encode(r, s)
        assert eo.der_decode(enc) == (r, s)
        assert eo.der_decode(enc + b'\x00') is None and eo.der_decode(enc[:-1]) is None
    Q = eo.mult_g(5)
    assert not eo.verify_digest(Q, 0, 1, 1) and not eo.verify_digest(Q, 1, 0, 1)
    assert not eo.verify_digest(Q, N, 1, 1) and not eo.verify_digest(Q, 1, N, 1)


# ------------------------------------------------------------------ the constructed families
def test_comb_cases_are_complete():
    cases = eo.comb_cases()
    hits = [c for c in cases if c.role == 'hit']
    # six windows, both kinds, every shape the window has, four window values: none dropped
    want = {(i, kind, shape) for i in eo.HIT_WINDOWS for kind in ('double', 'cancel')
            for shape in ('only', 'below', 'above') if not (i == 0 and shape == 'below') and not (i == 15 and shape == 'above')}
    got = collections.Counter((c.i, c.kind, c.shape) for c in hits)
    assert set(got) == want and set(got.values()) == {4} and len(hits) == 128
    for role in ('miss_sum', 'miss_window', 'scaled'):
        assert len([c for c in cases if c.role == role]) == len(hits)
    assert len({c.name for c in cases}) == len(cases) == 512
    for c in hits:
        assert {1, 0xFFFF, 0x8000} <= {h.u1 >> (16 * c.i) & 0xFFFF for h in hits if (h.i, h.kind, h.shape) == (c.i, c.kind, c.shape)}
    for c in cases:
        assert 0 <= c.u1 < N and c.u2 * c.d % N and 1 <= c.case.r < N and 1 <= c.case.s < N  # nothing degenerate


def test_every_comb_case_is_classified_as_intended():
    for c in eo.comb_cases():
        w = eo.comb_windows(c.u1)
        events, t = eo.comb_trace(c.u1, c.u2 * c.d)
        assert [i for i, _ in events] == [i for i, v in enumerate(w) if v], c.name
        special = [(i, k) for i, k in events if k != 'add']
        if c.role in ('hit', 'scaled'):
            above = [i for i, v in enumerate(w) if v and i > c.i]
            assert (c.shape == 'above') == bool(above), c.name
            assert (c.shape == 'below') == any(w[:c.i]), c.name
            # the hit falls at the intended window with the intended kind; after a cancellation in the
            # middle the next window is added onto infinity
            want = [(c.i, c.kind)] + ([(above[0], 'from_inf')] if c.kind == 'cancel' and above else [])
            assert special == want, c.name
            assert (t != 0) == (c.kind == 'double' or bool(above)), c.name
            # an addition without the special cases decides something else: undefined at the hit
            ev2, t2 = eo.comb_trace(c.u1, c.u2 * c.d, complete=False)
            assert t2 == 'undefined' and ev2[-1] == (c.i, c.kind) and t2 != t, c.name
        else:
            assert special == [], c.name  # the siblings miss: plain additions only
            assert eo.comb_trace(c.u1, c.u2 * c.d, complete=False) == (events, t), c.name
        # the constructor's verdict, the trace's and the equation's are one
        valid = c.case.valid
        assert valid == (t != 0 and c.role != 'scaled'), c.name
        assert eo.verify_digest(c.case.Q, c.case.r, c.case.s, c.case.e) == valid, c.name
        assert c.case.e * pow(c.case.s, -1, N) % N == c.u1 and c.case.r * pow(c.case.s, -1, N) % N == c.u2, c.name
    hits = [c for c in eo.comb_cases() if c.role == 'hit']
    assert sum(c.case.valid for c in hits if c.kind == 'double') == 64
    assert sum(c.case.valid for c in hits if c.kind == 'cancel') == 20  # the ones that run on from infinity
    assert sum(not c.case.valid for c in hits if c.kind == 'cancel') == 44


def test_scalar_cases_force_what_they_say():
    V = eo.scalar_set()
    assert len(V) == 735 and all(1 <= v < N for v in V)
    assert {1, 2, 3, N - 1, N - 2, (N + 1) // 2, (N - 1) // 2, 2 ** 251, N - 2 ** 251, 16 ** 63 + 1, 16 - 1} <= set(V)
    cases = eo.scalar_cases()
    by = collections.defaultdict(list)
    for c in cases:
        by[c.family].append(c)
    inv = lambda c: pow(c.s, -1, N)  # noqa: E731
    assert [c.r * inv(c) % N for c in by['u2']] == list(V)
    assert [c.s for c in by['s']] == list(V)
    assert [c.digest % N * inv(c) % N for c in by['u1']] == [0] + list(V)
    assert len(by['e_plus_n']) == 64 and all(N <= c.digest < 2 ** 256 for c in by['e_plus_n'])
    assert {c.digest for c in by['e_plus_n']} >= {N, N + 1, 2 ** 256 - 1}
    for fam in ('u2', 's', 'u1', 'e_plus_n'):
        assert all(c.valid for c in by[fam])
        muts = by[fam + '_mutant']
        assert len(muts) >= 3 * (len(by[fam]) // 5) and not any(m.valid for m in muts)  # the oracle's verdict: each False
        assert all(1 <= m.r < N and 1 <= m.s < N for m in muts)  # all reach the device
    rng = random.Random(6)
    for c in rng.sample([c for c in cases if c.valid], 150):  # valid by construction, and by the equation
        assert eo.verify_digest(c.Q, c.r, c.s, c.digest), c.name


def test_hash_cases():
    cases = eo.hash_cases()
    assert len(cases) == 2 * len(eo.HASH_LENGTHS) == 528
    assert [len(c.msg) for c in cases[::2]] == list(eo.HASH_LENGTHS)
    for good, bad in zip(cases[::2], cases[1::2]):
        assert good.code == (2 if len(good.msg) % 2 else 1), good.name
        assert bad.code == 0 and bad.sig == good.sig and bad.msg != good.msg, bad.name
        assert len(bad.msg) == max(len(good.msg), 1)


# ------------------------------------------------------------------ the GPU tests can fail
@functools.lru_cache(maxsize=None)
def comb_entry(i, v):
    return eo.mult_g(v << (16 * i))  # table[i << 16 | v] of the kernel's comb


def kernel_add(p, q, inf_branch, doubling):
    """``gej_add_ge_t`` (secp256k1_dev.h) over integers; p = (X, Y, Z, inf).  ``inf_branch=False`` takes
    out the ``p.inf`` branch (the stale coordinates go through the formulas); ``doubling`` is 'full',
    'absent' (the ``kDouble = false`` instantiation: the accumulator stays as it is) or 'formula' (no test
    for h = 0 with rr = 0 at all: the general formulas run and give Z = 0)."""
    x1, y1, z1, inf = p
    if inf and inf_branch:
        return q[0], q[1], 1, False
    zz = z1 * z1 % P
    h = (q[0] * zz - x1) % P
    rr = (q[1] * zz * z1 - y1) % P
    if h == 0 and rr != 0:
        return x1, y1, z1, True
    if h == 0 and doubling == 'full':
        d = eo.jac_double((x1, y1, z1))
        return d[0], d[1], d[2], False
    if h == 0 and doubling == 'absent':
        return x1, y1, z1, False
    hh = h * h % P
    hhh = h * hh % P
    v = x1 * hh % P
    x3 = (rr * rr - hhh - 2 * v) % P
    return x3, (rr * (v - x3) - y1 * hhh) % P, z1 * h % P, False


HAS_RN = ('as_is', 'never', 'no_carry_guard', 'no_canonical_guard')


def kernel_point(c, inf_branch=True, doubling='full'):
    """``sg_comb_kernel`` up to its comparison: T = u2 Q, then the comb over u1's windows; (X, Y, Z, inf)."""
    T = eo.mult(c.u2, c.case.Q)
    acc = (T[0], T[1], 1, False)
    for i, v in enumerate(eo.comb_windows(c.u1)):
        if v:
            acc = kernel_add(acc, comb_entry(i, v), inf_branch, doubling)
    return acc


def kernel_decide(acc, r, has_rn='as_is'):
    """``x_is_r`` and the guard in front of it: X = r Z^2, or X = (r + n) Z^2 with r + n as the kernel holds
    it, in 256 bits, which counts only when ``has_rn``: no carry out of 256 bits (``c == 0``) and already
    canonical (``same == 0``), that is r + n < p.  ``has_rn`` 'never' drops the second comparison,
    'no_carry_guard' and 'no_canonical_guard' one of its two guards."""
    x, _, z, inf = acc
    rn, carry = (r + N) % 2 ** 256, (r + N) >> 256
    canonical = rn < P  # fe_normalize leaves it as it is
    guard = {'as_is': not carry and canonical, 'never': False, 'no_carry_guard': canonical,
             'no_canonical_guard': not carry}[has_rn]
    return not inf and ((x - r * z * z) % P == 0 or (guard and (x - rn * z * z) % P == 0))


def kernel_verdict(c, inf_branch=True, doubling='full', has_rn='as_is'):
    """``sg_comb_kernel`` for one digest: T = u2 Q, the comb over u1's windows, then X = r Z^2 or
    (r + n) Z^2."""
    return kernel_decide(kernel_point(c, inf_branch, doubling), c.case.r, has_rn)


def test_a_comb_without_a_branch_gets_constructed_cases_wrong():
    cases = [c for c in eo.comb_cases() if c.role in ('hit', 'scaled')]
    wrong = lambda **kw: [c for c in cases if kernel_verdict(c, **kw) != c.case.valid]  # noqa: E731
    assert wrong() == []  # the model of the kernel as it is decides every case as the oracle does
    no_inf = wrong(inf_branch=False)
    assert no_inf and all(c.kind == 'cancel' and c.shape == 'above' and c.role == 'hit' for c in no_inf)
    assert len(no_inf) == 20  # every signature that runs on from infinity is refused without the branch
    no_double = wrong(doubling='absent')
    assert len(no_double) == 64 and all(c.kind == 'double' and c.role == 'hit' for c in no_double)
    # With no test for equal points at all the formulas give Z = 0 and X = 0, and X = r Z^2 holds for any r:
    # the valid doublings still pass, and only the 'scaled' siblings (the same path, a wrong r) show it.
    formula = wrong(doubling='formula')
    assert len(formula) == 64 and all(c.kind == 'double' and c.role == 'scaled' for c in formula)
