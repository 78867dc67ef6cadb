"""The address SEARCH path (``ar_search_kernel<false, W>`` through ``try_quad``: four combs per lane,
X and Y parked in LDS, the four-way inversion, the mode selects, the ``ntries`` tail, the early
exit and ``atomicMin``) against whole windows of tries made by the reference's primitives
(tests/golden/addr_window_kats.json).  The per-try values the other tests compare come from the
resolve instantiation (``try_keys``), one try per launch behind a two-point inversion.

A window is enumerated through the public calls only: search with one null byte from ``cur``,
record the hit, go on at ``k + 1``.  The list must equal the fixture's, so no true hit is skipped
and no false one appears in any slot of any lane, at whatever alignment each restart gives, and
the final ``None`` covers the tail without a hit.

The ``key_hash`` sweep runs the search kernel on one try (``ntries = 1``) and then the resolve
kernel, at every tail offset of ``varint(m) || 0x80`` and every varint size."""
import ctypes
import hashlib

import pytest

from oracle import addrgen_oracle as ao
from pybitmessage_amd import _lib, addressgen

pytestmark = pytest.mark.gpu

_pubs = {}  # private key -> public key by the oracle, shared by every test of the module


@pytest.fixture(scope='module')
def pm():
    try:  # libcrypto's EC_POINT_mul (pinned by test_oracle_openssl_pointmult_matches_restatement)
        mult = ao.OpenSSLPointMult()
    except Exception:  # noqa: BLE001
        mult = ao.point_mult

    def cached(priv):
        if priv not in _pubs:
            _pubs[priv] = mult(priv)
        return _pubs[priv]
    return cached


@pytest.fixture(scope='module')
def windows(golden):
    return {(w['mode'], w['index']): w for w in golden('addr_window_kats.json')['windows']}


@pytest.fixture(autouse=True)
def comb16(gpulib):
    """The 16-bit comb, whatever an earlier test left built; restore automatic choice after."""
    gpulib.bmpow_addr_set_comb(16)
    yield
    gpulib.bmpow_addr_set_comb(0)


@pytest.fixture
def comb24(comb16, shards, gpulib):
    """Force the 24-bit comb (10.7 GB table) for the test; the shard set is renewed after, which
    releases the table."""
    gpulib.bmpow_addr_set_comb(24)
    yield gpulib
    gpulib.bmpow_addr_set_comb(0)


def search_random(priv_s, seed, null_bytes, start, max_tries=None):
    lib = _lib.get()
    out = _lib.BmpowAddress()
    n = addressgen.CALL_TRIES if max_tries is None else max_tries
    rc = _lib.check(lib, lib.bmpow_address_search_random(priv_s, seed, len(seed), start, n, null_bytes, ctypes.byref(out)),
                    'bmpow_address_search_random')
    return addressgen.Found(out) if rc == _lib.FOUND else None


def search(w, start, max_tries, null_bytes=1):
    seed = bytes.fromhex(w['seed'])
    if w['mode'] == 0:
        return addressgen.search_deterministic(seed, null_bytes, start, max_tries)
    return search_random(bytes.fromhex(w['priv_signing']), seed, null_bytes, start, max_tries)


def enumerate_window(w, bounded=True):
    """Every hit the public calls report in the window, in order, and what ended the walk: None
    (bounded: the budget ends with the window) or the first hit past the window's end."""
    end, cur, found = w['start'] + w['count'], w['start'], []
    while True:
        f = search(w, cur, end - cur if bounded else None)
        if f is None or f.k >= end:
            return found, f
        assert f.k >= cur and len(found) < w['count'], (f.k, cur)
        found.append(f)
        cur = f.k + 1


def check_window(w, pm, bounded=True):
    found, last = enumerate_window(w, bounded)
    got = [(f.k - w['start'], f.ripe.hex(), f.priv_signing.hex(), f.priv_encryption.hex()) for f in found]
    want = [(h['k'] - w['start'], h['ripe'], h['priv_signing'], h['priv_encryption']) for h in w['hits']]
    assert [g[0] for g in got] == [x[0] for x in want]  # the offsets first: the readable failure
    assert got == want
    for f in found:
        assert (f.pub_signing, f.pub_encryption) == (pm(f.priv_signing), pm(f.priv_encryption)), f.k
    if bounded:
        assert last is None
    return found


DET = [(0, i) for i in range(8)]
RND = [(1, i) for i in range(5)]


@pytest.mark.parametrize('key', DET + RND, ids=lambda k: 'mode%d-w%d' % k)
def test_gpu_window_enumeration(gpulib, windows, pm, key):
    check_window(windows[key], pm)
    assert gpulib.bmpow_addr_last_comb() == 16


@pytest.mark.parametrize('key', [(0, 7), (1, 2)], ids=lambda k: 'mode%d-w%d' % k)
def test_gpu_window_enumeration_three_shards(gpulib, shards, windows, pm, key):
    """Unbounded steps: all three shards launch their slice, the minimum comes from shard 0."""
    shards([0, 0, 0])
    check_window(windows[key], pm, bounded=False)


@pytest.mark.parametrize('key', [(0, 2), (1, 1)], ids=lambda k: 'mode%d-w%d' % k)
def test_gpu_window_enumeration_large_comb(comb24, windows, pm, key):
    check_window(windows[key], pm)
    assert comb24.bmpow_addr_last_comb() == 24


# ------------------------------------------------------------------ deterministic lane boundaries
def test_gpu_deterministic_first_try_and_lane_boundaries(gpulib, windows):
    """Mode 0 runs two tries per lane, aligned to ``start``: the search must return the FIRST
    k >= start with the prefix whatever the alignment of the start and of the budget's end."""
    cases = 0
    for index in (0, 3, 5):
        w = windows[(0, index)]
        ks = [h['k'] for h in w['hits']]
        end = w['start'] + w['count']
        for h in [k for k in ks if k - w['start'] >= 257][:2]:
            for d in (0, 1, 2, 3, 5, 64, 257):
                start = h - d
                want = next(k for k in ks if k >= start)
                assert search(w, start, end - start).k == want, (index, h, d)
                assert search(w, start, h - start + 1).k == want, (index, h, d)  # the budget ends on the hit
                if want == h:
                    assert search(w, start, h - start) is None, (index, h, d)  # ... or just before it
                cases += 1
    assert cases == 6 * 7


def test_gpu_deterministic_adjacent_hits(gpulib, windows):
    """Hits at offsets 466 and 468: both slots of one lane, or the same slot of neighbouring
    lanes, depending on the start."""
    w = windows[(0, 7)]
    s, end = w['start'], w['start'] + w['count']
    offs = [h['k'] - s for h in w['hits']]
    assert [o for o in offs if 466 <= o <= 606] == [466, 468, 606]
    for o, want in ((466, 466), (467, 468), (468, 468), (469, 606)):
        assert search(w, s + o, end - s - o).k - s == want, o


# ------------------------------------------------------------------ key_hash at every tail offset
SWEEP_LENGTHS = list(range(128)) + [128, 129, 255, 256, 383]
DET_KS = [0, 126, 127, 32767, 32768, 2 ** 31 - 1, 2 ** 31, 2 ** 40 + 3, 2 ** 63 - 1]
RND_KS = [0, 252, 253, 65535, 65536, 2 ** 32 - 1, 2 ** 32, 2 ** 64 - 2]


def sweep_bytes(n):
    """Distinct per position, so a misplaced tail byte changes the hash."""
    return bytes((7 * i + 1) % 251 for i in range(n))


@pytest.mark.parametrize('k', DET_KS)
def test_gpu_key_hash_sweep_deterministic(gpulib, pm, k):
    for i, n in enumerate(SWEEP_LENGTHS):
        pp = sweep_bytes(n)
        f = addressgen.search_deterministic(pp, 0, k, 1)
        ps = hashlib.sha512(pp + ao.encode_varint(2 * k)).digest()[:32]
        pe = hashlib.sha512(pp + ao.encode_varint(2 * k + 1)).digest()[:32]
        assert f.k == k
        assert (f.priv_signing, f.priv_encryption) == (ps, pe), n
        if i % 8 == 0:
            assert (f.pub_signing, f.pub_encryption) == (pm(ps), pm(pe)), n
            assert f.ripe == ao.ripe_of(pm(ps), pm(pe)), n


@pytest.mark.parametrize('k', RND_KS)
def test_gpu_key_hash_sweep_random(gpulib, pm, k):
    priv_s = hashlib.sha256(b'bmpow random-mode signing key').digest()
    for n in range(128):
        seed = sweep_bytes(n)
        f = search_random(priv_s, seed, 0, k, 1)
        pe = hashlib.sha512(seed + ao.encode_varint(k)).digest()[:32]
        assert f.k == k
        assert (f.priv_signing, f.priv_encryption) == (priv_s, pe), n
        if n % 8 == 0:
            assert (f.pub_signing, f.pub_encryption) == (pm(priv_s), pm(pe)), n
            assert f.ripe == ao.ripe_of(pm(priv_s), pm(pe)), n


# ------------------------------------------------------------------ the top of the deterministic range
# k = 2^63 - 1 is the last try (nonces 2^64 - 2 and 2^64 - 1, the last ``encodeVarint`` takes).  A
# lane above it would compute 2k + q wrapped, that is the keys of a small try under a k >= 2^63.
@pytest.mark.parametrize('back, budget', [(98, 98), (98, 100000), (98, None), (1, 2 ** 40)])
def test_gpu_budget_across_the_last_try(gpulib, windows, back, budget):
    """Window 4's last hit is 2^63 - 99: a search of the tries after it finds nothing, whether its
    budget ends on the last try or reaches past it."""
    w = windows[(0, 4)]
    assert w['hits'][-1]['k'] == 2 ** 63 - 99
    f = addressgen.search_deterministic(bytes.fromhex(w['seed']), 1, 2 ** 63 - back, budget)
    assert f is None, 'k = 2^63 + %d' % (f.k - 2 ** 63)


def test_gpu_the_last_try_and_above(gpulib, windows, pm):
    pp = bytes.fromhex(windows[(0, 4)]['seed'])
    f = addressgen.search_deterministic(pp, 0, 2 ** 63 - 1, 5)
    ps = hashlib.sha512(pp + ao.encode_varint(2 ** 64 - 2)).digest()[:32]
    pe = hashlib.sha512(pp + ao.encode_varint(2 ** 64 - 1)).digest()[:32]
    assert f.k == 2 ** 63 - 1 and (f.priv_signing, f.priv_encryption) == (ps, pe)
    assert (f.pub_signing, f.pub_encryption) == (pm(ps), pm(pe)) and f.ripe == ao.ripe_of(pm(ps), pm(pe))
    for start in (2 ** 63, 2 ** 63 + 1, 2 ** 64 - 1):
        with pytest.raises(_lib.BmpowError) as e:
            addressgen.search_deterministic(pp, 1, start, 5)
        assert e.value.code == _lib.E_ARG
