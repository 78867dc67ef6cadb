"""The window fixture of the address search (tests/golden/addr_window_kats.json, made by the
reference's primitives in tests/golden/make_addr_window_golden.py) against the project's oracle:
every listed hit is re-derived, a sample of the tries it does not list has no prefix, and the
coverage the GPU tests (tests/test_gpu_addr_windows.py) rely on is still in the file."""
import hashlib
import random

import pytest

from oracle import addrgen_oracle as ao

# windows that straddle a varint boundary of the nonce: (mode, index) -> first k on its far side
BOUNDARIES = {(0, 0): 127, (0, 1): 32768, (0, 2): 2 ** 31, (1, 1): 65536, (1, 2): 2 ** 32, (1, 4): 253}
SHAPES = {0: [(0, 2048), (32768 - 1024, 2048), (2 ** 31 - 1024, 2048), (2 ** 40 + 3, 2048), (2 ** 63 - 2048, 2048),
              (12345, 2048), (65536 - 1000, 2048), (2 ** 32 - 1, 2048)],
          1: [(0, 4096), (65536 - 2048, 4096), (2 ** 32 - 2048, 4096), (2 ** 40 + 1, 4096), (0, 512)]}
NON_HIT_SAMPLE = 32  # per window; pure-Python point multiplications take ~14 ms each


@pytest.fixture(scope='module')
def windows(golden):
    return golden('addr_window_kats.json')['windows']


@pytest.fixture(scope='module')
def pm():
    try:  # libcrypto's EC_POINT_mul (pinned by test_oracle_openssl_pointmult_matches_restatement)
        return ao.OpenSSLPointMult()
    except Exception:  # noqa: BLE001
        return ao.point_mult


def window_keys(w, k):
    """Private keys of try k of a window, by the oracle."""
    seed = bytes.fromhex(w['seed'])
    if w['mode'] == 0:
        return ao.try_keys(seed, k)
    return bytes.fromhex(w['priv_signing']), hashlib.sha512(seed + ao.encode_varint(k)).digest()[:32]


def test_window_hits_match_oracle(windows, pm):
    for w in windows:
        for h in w['hits']:
            ps, pe = window_keys(w, h['k'])
            assert (ps.hex(), pe.hex()) == (h['priv_signing'], h['priv_encryption']), (w['mode'], w['index'], h['k'])
            assert ao.ripe_of(pm(ps), pm(pe)).hex() == h['ripe'], (w['mode'], w['index'], h['k'])
            assert h['ripe'][:2] == '00'


def test_window_non_hits_have_no_prefix(windows, pm):
    rng = random.Random(20250216)
    for w in windows:
        hits = {h['k'] for h in w['hits']}
        pub_s = pm(bytes.fromhex(w['priv_signing'])) if w['mode'] == 1 else None
        others = [k for k in (w['start'] + o for o in rng.sample(range(w['count']), NON_HIT_SAMPLE + len(hits)))
                  if k not in hits][:NON_HIT_SAMPLE]
        assert len(others) == NON_HIT_SAMPLE
        for k in others:
            ps, pe = window_keys(w, k)
            ripe = ao.ripe_of(pub_s or pm(ps), pm(pe))
            assert ripe[:1] != b'\x00', (w['mode'], w['index'], k)


def test_window_coverage(windows):
    """What the GPU tests need from the file: the windows of the issue, >= 3 hits each, sorted and
    inside the window; hits in every slot of a lane (offset parity in mode 0, offset mod 4 in mode
    1); a hit on each side of every varint boundary a window straddles."""
    for mode in (0, 1):
        ws = [w for w in windows if w['mode'] == mode]
        assert [w['index'] for w in ws] == list(range(len(SHAPES[mode])))
        assert [(w['start'], w['count']) for w in ws] == SHAPES[mode]
        mod = 2 if mode == 0 else 4
        slots = [0] * mod
        for w in ws:
            ks = [h['k'] for h in w['hits']]
            assert len(ks) >= 3 and ks == sorted(set(ks))
            assert w['start'] <= ks[0] and ks[-1] < w['start'] + w['count']
            for k in ks:
                slots[(k - w['start']) % mod] += 1
            b = BOUNDARIES.get((mode, w['index']))
            if b is not None:
                assert w['start'] < b < w['start'] + w['count']
                assert any(k < b for k in ks) and any(k >= b for k in ks), (mode, w['index'])
        assert all(slots), (mode, slots)
    det = {w['index']: w for w in windows if w['mode'] == 0}
    assert det[4]['start'] + det[4]['count'] == 2 ** 63  # 2k + 1 = 2^64 - 1 is the last nonce there is
    assert {466, 468, 606} <= {h['k'] - det[7]['start'] for h in det[7]['hits']}  # the adjacent pair
    assert sum(len(w['hits']) for w in windows if w['mode'] == 0) == 65
    assert sum(len(w['hits']) for w in windows if w['mode'] == 1) == 73
