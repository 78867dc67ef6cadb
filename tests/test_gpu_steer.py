"""The search kernels' own trial function (sha512_dev.h kSearch: the steered 3-input ops and the extra
hoisted schedule terms, whichever of them the build carries) against the C oracle and against the
library's unsteered kernels, on constructed first hits.

The targets are built on the CPU, so where the first hit lies is chosen: every lane position at which
the lo / hi operands, the wave reduction or the early exit could go wrong, in one or two 256-nonce
blocks.  bmpow_min_trial_batch and bmpow_trials keep the plain trial function, so they check the search
independently.  Run on an MI355X: pytest -m gpu."""
import ctypes
import random

import numpy as np
import pytest

from pybitmessage_amd import _lib, proofofwork

pytestmark = pytest.mark.gpu
U64 = (1 << 64) - 1
P64 = ctypes.POINTER(ctypes.c_uint64)
LANES = (0, 63, 64, 255, 256)  # offsets from the window's start: 256 is lane 0 of the second block


def first_hit_at(coracle, rng, start, off, n):
    """n (ih, target, trial) whose first nonce >= start with trial <= target is start + off: random
    initialHashes kept when the minimum over [start, start + off] falls on its last nonce (one in
    off + 1 does), with that minimum as the target."""
    out = []
    nonces = np.uint64(start) + np.arange(off + 1, dtype=np.uint64)
    while len(out) < n:
        ih = rng.randbytes(64)
        tv = coracle.trials(ih, nonces)
        if int(np.argmin(tv)) == off and (off == 0 or int(tv[:off].min()) > int(tv[off])):
            out.append((ih, int(tv[off]), int(tv[off])))
    return out


def search_batch(lib, ihs, targets, starts, budget=1 << 20):
    n = len(ihs)
    nxt = _lib.u64_array(starts)
    nonce, trial = (ctypes.c_uint64 * n)(), (ctypes.c_uint64 * n)()
    done = (ctypes.c_uint8 * n)()
    for _ in range(64):
        left = _lib.check(lib, lib.bmpow_search_batch(n, b''.join(ihs), _lib.u64_array(targets), nxt, budget, nonce,
                                                      trial, done), 'bmpow_search_batch')
        if left == 0:
            break
    assert all(d == _lib.DONE_FOUND for d in done)
    return [(int(t), int(k)) for t, k in zip(trial, nonce)]


def search_one(lib, ih, target, start, max_trials):
    n, t = ctypes.c_uint64(), ctypes.c_uint64()
    rc = _lib.check(lib, lib.bmpow_search(ih, target, start, max_trials, ctypes.byref(n), ctypes.byref(t)),
                    'bmpow_search')
    return (t.value, n.value) if rc == _lib.FOUND else None


def min_trials(lib, ihs, starts, counts):
    n = len(ihs)
    mn, arg = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    st, ct = np.array(starts, dtype=np.uint64), np.array(counts, dtype=np.uint64)
    _lib.check(lib, lib.bmpow_min_trial_batch(n, b''.join(ihs), st.ctypes.data_as(P64), ct.ctypes.data_as(P64),
                                              mn.ctypes.data_as(P64), arg.ctypes.data_as(P64)), 'bmpow_min_trial_batch')
    return [int(x) for x in mn]


def trial_at(lib, ih, nonce):
    a, out = (ctypes.c_uint64 * 1)(nonce), (ctypes.c_uint64 * 1)()
    _lib.check(lib, lib.bmpow_trials(ih, a, 1, out), 'bmpow_trials')
    return int(out[0])


@pytest.mark.parametrize('off', LANES)
def test_first_hit_at_chosen_lane(gpulib, coracle, off):
    """Eight objects whose first hit is lane `off` of the window: through the C ABI from nonce 0 (the
    hit is nonce `off`) and through run_batch / run, which start at nonce 1 (the hit is 1 + off)."""
    rng = random.Random(1000 + off)
    from0 = first_hit_at(coracle, rng, 0, off, 8)
    want0 = [(tv, off) for _, _, tv in from0]
    assert search_batch(gpulib, [o[0] for o in from0], [o[1] for o in from0], [0] * 8) == want0
    assert [search_one(gpulib, ih, t, 0, 512) for ih, t, _ in from0] == want0
    from1 = first_hit_at(coracle, rng, 1, off, 8)
    want1 = [[tv, 1 + off] for _, _, tv in from1]
    assert proofofwork.run_batch([(t, ih) for ih, t, _ in from1]) == want1
    assert [proofofwork.run(t, ih) for ih, t, _ in from1] == want1
    assert want1 == [list(coracle.search(ih, t)) for ih, t, _ in from1]


@pytest.mark.parametrize('hit', [(1 << 32) - 1, 1 << 32, (1 << 32) + 1])
def test_first_hit_across_the_2_32_carry(gpulib, coracle, hit):
    """A window from 2^32 - 300 with its first hit either side of the carry of W0's low half into its
    high half (the add beside the steered ops): both search paths, four objects each."""
    start = (1 << 32) - 300
    objs = first_hit_at(coracle, random.Random(hit), start, hit - start, 4)
    want = [(tv, hit) for _, _, tv in objs]
    assert search_batch(gpulib, [o[0] for o in objs], [o[1] for o in objs], [start] * 4) == want
    assert [search_one(gpulib, ih, t, start, 600) for ih, t, _ in objs] == want
    assert [search_one(gpulib, ih, t - 1, start, hit - start + 1) for ih, t, _ in objs] == [None] * 4


@pytest.fixture(scope='module')
def easy(coracle):
    """64 random objects whose first nonce is expected near 2^12, with the oracle's answers."""
    rng = random.Random(4096)
    objs = [(U64 >> 12, rng.randbytes(64)) for _ in range(64)]
    return objs, [list(r) for r in coracle.search_many(objs)]


def check_against_unsteered(lib, objs, res):
    """res[i] = [trial, nonce]: nothing below the nonce hits (the min-trial probe over [1, nonce)) and
    the trial value is the plain kernel's."""
    ihs = [ih for _, ih in objs]
    below = min_trials(lib, ihs, [1] * len(objs), [n - 1 for _, n in res])
    for (target, ih), (tv, n), m in zip(objs, res, below):
        assert n >= 1 and tv <= target
        assert m > target
        assert trial_at(lib, ih, n) == tv


def test_search_against_unsteered_probe(gpulib, easy):
    objs, want = easy
    res = proofofwork.run_batch(objs)
    check_against_unsteered(gpulib, objs, res)
    assert res == want
    one = [proofofwork.run(t, ih) for t, ih in objs[:16]]
    check_against_unsteered(gpulib, objs[:16], one)
    assert one == want[:16]


def test_split_layout_relay_beside_columns(gpulib, shards, engine_split, easy):
    """Three shards as three device groups: with fewer objects than groups the engine splits every
    window into pieces, so each launch carries the relay workgroup beside its columns (kX).  The 64
    objects two at a time, then all at once; and the single-object kernel's relay with run()'s window
    cut into one piece per shard."""
    objs, want = easy
    shards([0, 0, 0])
    engine_split(True)
    gpulib.bmpow_set_step_trials(1 << 22)
    res = []
    for i in range(0, len(objs), 2):
        res += proofofwork.run_batch(objs[i:i + 2])
    check_against_unsteered(gpulib, objs, res)
    assert res == want
    assert proofofwork.run_batch(objs) == want
    prev = gpulib.bmpow_set_run_split(1)
    try:
        one = [proofofwork.run(t, ih) for t, ih in objs[:8]]
    finally:
        gpulib.bmpow_set_run_split(prev)
    check_against_unsteered(gpulib, objs[:8], one)
    assert one == want[:8]
