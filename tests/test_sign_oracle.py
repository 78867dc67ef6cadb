"""Signatures chosen by their r and s (no device): the signing families of ``oracle/ecdsa_oracle.py`` that
``tests/test_gpu_sign_constructed.py`` runs on the device.  Every row is shown from integers to verify and to
have the property its family names, the counts are literal, and integer and byte models of ``sd_sign_kernel``
(``scalar_dev.h``'s ``reduce512`` and ``add``) and of the device's DER writer (``bmpow_tx_fmt.h``) with one step
taken out are run over the same rows: the test prints and asserts by how many rows of which family each defect
is caught.

The models of ``reduce512`` split integers at 2^256 where the header folds limbs; the sums are the same ones
(``test_the_integer_folds_are_the_limb_folds`` compares them with a limb-by-limb transcription).  The inversion
is the header's whole chain with the same defect in every product, on every row.

Not reached, and not claimed: a ``reduce512`` without its fourth fold.  The third fold leaves a carry bit only
when it ends within 2^133 of 2^256, one product in about 2^123, and no family forces that: the model with the
fold taken out signs every row as it should (0 rows caught).  A ``reduce512`` without its conditional
subtraction is caught (590 rows).

Not observable, and not claimed: an ``add`` that leaves out the subtraction for a sum in [n, 2^256) (it still
subtracts on a carry).  Its result is a non-canonical residue below 2^256, and the product that follows reduces
any operand below 2^256: s comes out the same on every row, the row with the sum exactly n included (n times
anything is 0 mod n)."""
import collections
import functools
import random

from oracle import ecdsa_oracle as eo

N = eo.N
M = 2 ** 256
C = M - N


def b32(v):
    return v.to_bytes(32, 'big')


def cases():
    return eo.sign_cases()


def by_family(family):
    return [c for c in cases() if c.family == family]


# ------------------------------------------------------------------ the rows are what they say
FAMILY_COUNTS = {'k': 735, 'kinv': 735, 'd': 735, 't': 1470, 's': 735, 'sum': 39, 'len': 1067}


def test_family_counts():
    assert collections.Counter(c.family for c in cases()) == FAMILY_COUNTS
    assert len(cases()) == 5516 and len({c.name for c in cases()}) == 5516
    assert [c.name for c in cases() if c.s == 0] == ['sum_1']
    assert len(eo.scalar_set()) == 735 and len(eo.s_len_values()) == 97 and len(eo.SHORT_R_NONCES) == 11
    assert sum(c.e >= N for c in cases()) == 735 + 1  # unreduced digests: every t_plus_n row and one of 'sum'


def test_every_case_is_a_signature_that_verifies():
    for c in cases():
        assert 1 <= c.d < N and 1 <= c.k < N and 0 <= c.e < M and 1 <= c.r < N and 0 <= c.s < N, c.name
        assert c.r == eo.mult_g(c.k)[0] % N and c.s == (c.e + c.r * c.d) * pow(c.k, -1, N) % N, c.name
        if c.s:
            assert (c.r, c.s) == eo.sign(c.d, c.k, c.e % N), c.name
            assert eo.verify_digest(eo.mult_g(c.d), c.r, c.s, c.e), c.name
        else:
            assert not eo.verify_digest(eo.mult_g(c.d), c.r, c.s, c.e)


def test_scalar_families_force_what_they_name():
    V = eo.scalar_set()
    assert [c.k for c in by_family('k')] == V
    assert [pow(c.k, -1, N) for c in by_family('kinv')] == V
    assert [c.d for c in by_family('d')] == V
    assert [c.s for c in by_family('s')] == V
    t = by_family('t')
    assert [(c.e + c.r * c.d) % N for c in t[::2]] == V == [(c.e + c.r * c.d) % N for c in t[1::2]]
    assert all(c.e < N for c in t[::2]) and all(N <= c.e < M for c in t[1::2])
    assert [c.name.startswith('t_plus_n_') for c in t] == [False, True] * 735


def test_sum_family_reaches_every_sum():
    rows = by_family('sum')
    sums = [c.r * c.d % N + c.e % N for c in rows]
    assert tuple(sums[:7]) == eo.SUM_EDGES == (N - 1, N, N + 1, M - 1, M, M + 1, 2 * N - 2)
    assert all(N < T < M for T in sums[7:23]) and all(M < T < 2 * N - 2 for T in sums[23:])
    assert len(set(sums)) == 39
    assert collections.Counter(c.e for c in rows) == {5: 2, N + 5: 1, N - 1: 36}
    assert rows[6].e == N - 1 and rows[6].r * rows[6].d % N == N - 1  # 2 n - 2 is (n - 1) + (n - 1) alone
    assert [c.s == 0 for c in rows] == [T == N for T in sums]
    for c, T in zip(rows, sums):
        assert c.s == T % N * pow(c.k, -1, N) % N, c.name


def value_len(v):
    return (v.bit_length() + 7) // 8


def test_length_family_reaches_every_length():
    grid = eo.len_grid()
    rows = by_family('len')
    assert len(grid) == len(rows) == 11 * 97
    assert [(c.k, c.r, c.s) for c in rows] == [(n.k, r, s) for n, r, s in grid]
    for nonce in eo.SHORT_R_NONCES:
        r = eo.mult_g(nonce.k)[0]
        assert r < N and (value_len(r), r.bit_length() % 8 == 0) == (nonce.r_len, bool(nonce.top)), nonce.name
    assert [(n.name, n.r_len, n.top) for n in eo.SHORT_R_NONCES] == [
        ('half', 21, 0), ('z1_clear', 31, 0), ('z1_set', 31, 1), ('z2_clear', 30, 0), ('z2_set', 30, 1), ('full_set', 32, 1),
        ('full_clear', 32, 0), ('one', 32, 0), ('two', 32, 1), ('minus_one', 32, 0), ('minus_two', 32, 1)]
    assert eo.mult_g((N + 1) // 2)[0] == 0x3b78ce563f89a0ed9414f5aa28ad0d96d6795f9c63
    S = eo.s_len_values()
    assert S[-1] == N - 1 and all(1 <= s < N for s in S)
    assert S[:-1] == [v for ln in range(1, 33) for v in (2 ** (8 * ln - 1), 2 ** (8 * ln - 1) - 1, 2 ** (8 * (ln - 1)))]
    shape = collections.Counter((value_len(s), s.bit_length() % 8 == 0) for s in S)  # (bytes, needs the pad)
    assert shape == {**{(ln, True): 1 for ln in range(1, 32)}, **{(ln, False): 2 for ln in range(1, 33)}, (32, True): 2}
    ders = [eo.der_encode(r, s) for _, r, s in grid]
    assert {len(d) for d in ders} == set(range(28, 73))
    assert all(eo.der_decode(d) == (r, s) for d, (_, r, s) in zip(ders, grid))
    assert all(len(d) == 6 + value_len(r) + (r.bit_length() % 8 == 0) + value_len(s) + (s.bit_length() % 8 == 0)
               for d, (_, r, s) in zip(ders, grid))


# ------------------------------------------------------------------ models of scalar_dev.h
REDUCE_DEFECTS = ('no_last_fold', 'no_cond_sub')
ADD_DEFECTS = ('no_carry', 'no_sub_below_2_256')


def reduce512(p, defect=None):
    """``sn::reduce512``: three folds by 2^256 = c (mod n), one more for the carry bit, one conditional
    subtraction; 'no_last_fold' keeps 8 limbs of the third fold, 'no_cond_sub' returns what the folds leave."""
    t = (p % M) + (p >> 256) * C
    t = (t % M) + (t >> 256) * C
    t = (t % M) + (t >> 256) * C
    assert t >> 256 in (0, 1)
    if defect != 'no_last_fold':
        t = (t % M) + (t >> 256) * C
        assert t < M
    v = t % M
    return v - N if v >= N and defect != 'no_cond_sub' else v


def limbs(v, count):
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(count)]


def fold_limbs(lo, hi, on):
    """``sn::fold<HN, ON>`` limb by limb."""
    c = limbs(C, 5)
    o = [lo[i] if i < 8 else 0 for i in range(on)]
    for i, h in enumerate(hi):
        carry = 0
        for j in range(5):
            if i + j < on:
                t = h * c[j] + o[i + j] + carry
                o[i + j], carry = t & 0xFFFFFFFF, t >> 32
        for k in range(i + 5, on):
            t = o[k] + carry
            o[k], carry = t & 0xFFFFFFFF, t >> 32
    return o


def reduce512_limbs(p):
    p = limbs(p, 16)
    t1 = fold_limbs(p[:8], p[8:], 13)
    t2 = fold_limbs(t1[:8], t1[8:], 9)
    t3 = fold_limbs(t2[:8], t2[8:], 9)
    t4 = fold_limbs(t3[:8], t3[8:], 9)
    v = sum(x << (32 * i) for i, x in enumerate(t4[:8]))
    return v - N if v >= N else v


def test_the_integer_folds_are_the_limb_folds():
    rng = random.Random(1802)
    V = eo.scalar_set()
    pairs = [(rng.choice(V), rng.choice(V)) for _ in range(300)] + [(M - 1, M - 1), (N, N), (N - 1, N - 1), (M - 1, 1)]
    pairs += [(c.r, c.d) for c in by_family('sum')]
    for a, b in pairs:
        assert reduce512(a * b) == reduce512_limbs(a * b) == a * b % N, (hex(a), hex(b))


def mul(a, b, defect=None):
    return reduce512(a * b, defect)


def sqr_n_mul(a, k, b, defect):
    for _ in range(k):
        a = mul(a, a, defect)
    return mul(a, b, defect)


@functools.lru_cache(maxsize=None)
def inv(a, defect=None):
    """``sn::inv``: the addition chain to a^(2^127 - 1), the zero bit, square-and-multiply over the low half."""
    x1 = mul(a, 1, defect)
    x2 = sqr_n_mul(x1, 1, x1, defect)
    x3 = sqr_n_mul(x2, 1, x1, defect)
    x6 = sqr_n_mul(x3, 3, x3, defect)
    x12 = sqr_n_mul(x6, 6, x6, defect)
    x24 = sqr_n_mul(x12, 12, x12, defect)
    x48 = sqr_n_mul(x24, 24, x24, defect)
    x96 = sqr_n_mul(x48, 48, x48, defect)
    t = sqr_n_mul(x96, 24, x24, defect)
    t = sqr_n_mul(t, 6, x6, defect)
    t = sqr_n_mul(t, 1, x1, defect)
    t = mul(t, t, defect)
    low = (N - 2) & (2 ** 128 - 1)
    for i in range(127, -1, -1):
        t = mul(t, t, defect)
        if (low >> i) & 1:
            t = mul(t, x1, defect)
    return t


def add(a, b, defect=None):
    """``sn::add``: the 256-bit sum and its carry, a - n, and the choice between them; 'no_carry' chooses by the
    comparison alone, 'no_sub_below_2_256' by the carry alone."""
    t, carry = (a + b) % M, (a + b) >> 256
    sub = {None: carry or t >= N, 'no_carry': t >= N, 'no_sub_below_2_256': bool(carry)}[defect]
    return (t - N) % M if sub else t


def model_sign(c, red=None, plus=None):
    """``sd_sign_kernel`` from r on: (r, s), or None where it reports no signature."""
    ki = inv(c.k, red)
    em = mul(c.e, 1, red)
    t = add(mul(c.r, c.d, red), em, plus)
    s = mul(ki, t, red)
    return (c.r, s) if s else None


def caught(**how):
    """Per family, the rows on which the model with the defect gives another answer than signing must."""
    count = collections.Counter()
    for c in cases():
        if model_sign(c, **how) != ((c.r, c.s) if c.s else None):
            count[c.family] += 1
    return dict(count)


def test_the_model_of_the_kernel_as_it_is_signs_every_row():
    assert caught() == {}
    c = by_family('k')[3]
    assert inv(c.k) == pow(c.k, -1, N) and inv(N) == 0


def test_each_arithmetic_defect_is_caught_and_by_how_many_rows():
    got = {(kind, d): caught(**{kind: d}) for kind, ds in (('red', REDUCE_DEFECTS), ('plus', ADD_DEFECTS)) for d in ds}
    for key, count in got.items():
        print('%s=%s: caught by %d rows %s' % (key + (sum(count.values()), sorted(count.items()))))
    assert got == ARITHMETIC_CAUGHT


ARITHMETIC_CAUGHT = {
    # the third fold leaves a carry for one product in about 2^123, and no family forces one: not reached
    ('red', 'no_last_fold'): {},
    # the folds leave s + n where s is below 2^256 - n: the short s of 'len', the small values of V as s, and s = 0
    ('red', 'no_cond_sub'): {'len': 490, 's': 99, 'sum': 1},
    # every sum from 2^256 on: half of all seeded rows and the upper 19 of 'sum'
    ('plus', 'no_carry'): {'d': 344, 'k': 357, 'kinv': 373, 'len': 696, 's': 344, 'sum': 19, 't': 326},
    ('plus', 'no_sub_below_2_256'): {},  # not observable: see the module's docstring
}


# ------------------------------------------------------------------ models of the device's DER writer
DER_DEFECTS = ('no_strip', 'pad_on_byte_0', 'strip_one')


def der_int(v, defect=None):
    """``txf::der_int`` over the 32 big-endian bytes of v: the leading zero bytes (31 at the most) are skipped
    and a 0x00 goes in front of a first kept byte with its top bit set."""
    b = b32(v)
    skip = min(len(b) - len(b.lstrip(b'\x00')), 31)
    if defect == 'no_strip':
        skip = 0
    elif defect == 'strip_one':
        skip = min(skip, 1)
    top = b[0 if defect == 'pad_on_byte_0' else skip] & 0x80
    body = (b'\x00' if top else b'') + b[skip:]
    return b'\x02' + bytes([len(body)]) + body


def der(r, s, defect=None):
    body = der_int(r, defect) + der_int(s, defect)
    return b'\x30' + bytes([len(body)]) + body


def test_each_der_defect_is_caught_and_by_how_many_rows():
    rows = [c for c in cases() if c.s]
    assert all(der(c.r, c.s) == eo.der_encode(c.r, c.s) for c in rows)
    got = {}
    for d in DER_DEFECTS:
        count = collections.Counter(c.family for c in rows if der(c.r, c.s, d) != eo.der_encode(c.r, c.s))
        print('der %s: caught by %d rows %s' % (d, sum(count.values()), sorted(count.items())))
        got[d] = dict(count)
    assert got == DER_CAUGHT


DER_CAUGHT = {
    'no_strip': {'d': 2, 'k': 3, 'kinv': 8, 'len': 1032, 's': 239, 'sum': 1, 't': 11},
    'pad_on_byte_0': {'d': 4, 'k': 4, 'kinv': 1, 'len': 473, 's': 85, 't': 6},
    'strip_one': {'k': 2, 'kinv': 4, 'len': 995, 's': 231},
}


# ------------------------------------------------------------------ the strict DER reader, as built for the host
def needless_pad(r, s, which):
    """The DER of (r, s) with one 0x00 more than the sign needs in front of r (which = 0) or s (1)."""
    ints = [v.to_bytes(v.bit_length() // 8 + 1, 'big') for v in (r, s)]  # minimal: the pad where the top bit is set
    ints[which] = b'\x00' + ints[which]
    body = b''.join(b'\x02' + bytes([len(v)]) + v for v in ints)
    return b'\x30' + bytes([len(body)]) + body


def test_the_host_build_of_the_receive_side_parser_reads_every_length(golden):
    """``rxf::der_parse`` as compiled for the host (``receive.walk_msg``'s ``verifiable``) on a fixture msg whose
    signature is replaced by the first pair of the length grid of every DER length 28 .. 72, and by the same
    integers under a needless 0x00.  No msg that verifies can carry the short ones (the digest depends on the
    key in the plaintext, and the key would have to be solved from the digest), so on the device the parser
    sees only the lengths ``tests/test_gpu_sign_constructed.py`` names."""
    from pybitmessage_amd import receive
    m = next(m for m in golden('rx_kats.json')['msgs'] if m['line'] is None)
    obj, plain, ripe = bytes.fromhex(m['obj']), bytes.fromhex(m['plaintext']), bytes.fromhex(m['toRipe'])
    res, verifiable = receive.walk_msg(obj, plain, ripe)
    assert verifiable and int(res.status[0]) == receive.OK
    at, ln = int(res.recs[0]['sig_off']), int(res.recs[0]['sig_len'])
    assert plain[at - 1] == ln and at + ln == len(plain)
    first = {}
    for _, r, s in eo.len_grid():
        first.setdefault(len(eo.der_encode(r, s)), (r, s))
    assert sorted(first) == list(range(28, 73))
    seen = collections.Counter()
    for ln, (r, s) in sorted(first.items()):
        for sig, want in ((eo.der_encode(r, s), True), (needless_pad(r, s, 0), False), (needless_pad(r, s, 1), False)):
            assert (eo.der_decode(sig) == (r, s)) == want and (want or eo.der_decode(sig) is None)
            res, verifiable = receive.walk_msg(obj, plain[:at - 1] + bytes([len(sig)]) + sig, ripe)
            assert int(res.status[0]) == receive.OK and res.signature(0) == sig, ln  # the walk reads no signature
            assert verifiable == want, (ln, sig.hex())
            seen[want] += 1
    assert seen == {True: 45, False: 90}
