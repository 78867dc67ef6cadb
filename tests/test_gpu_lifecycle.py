"""Device-set lifecycle: every subsystem's per-shard state (the engine's launch buffers, the probe's
staging, run()'s rings, the verification pool and staging chunks, the address search's comb table) is
released and rebuilt by each bmpow_set_devices, with right answers in every layout and no device
memory left behind.  Small leaks are the native owner test's job (tests/native/own_sim.cpp); a comb
table (64 MiB) or a verification staging chunk's pool left behind shows here.  Run on an MI355X."""
import ctypes
import hashlib
import random

import pytest

from oracle import oracle
from pybitmessage_amd import addressgen, proofofwork, targets, verify
from tests.test_addressgen import SAMPLE_DET_RIPE, SAMPLE_SEED

pytestmark = pytest.mark.gpu

LAYOUTS = ([0], [0, 0, 0, 0], [0], [0, 0])
MIB = 1 << 20
# Free device memory right after the fourth re-selection may be lower than right after the second by at
# most what the library before the owners (one translation unit, hand-kept free lists) lost over the same
# body -- PARENT_DROP, measured on an MI355X with this test's body: free memory after the four
# re-selections read 294108, 294044, 293992, 293988 MiB, the same with the owners (the HIP runtime's own
# growth with the streams of the wider layouts) -- plus 32 MiB: half a 16-bit comb table, so a leaked
# table or verification pool exceeds it.
PARENT_DROP = 56 * MIB
BOUND = PARENT_DROP + 32 * MIB


def device_free_bytes():
    """hipMemGetInfo of device 0, asked of the HIP runtime the library itself has loaded (a second
    runtime in the process -- the one bundled with PyTorch -- need not see the device at all)."""
    with open('/proc/self/maps') as f:
        path = next(line.split()[-1] for line in f if 'libamdhip64.so' in line)
    hip = ctypes.CDLL(path)
    free, total = ctypes.c_size_t(), ctypes.c_size_t()
    assert hip.hipSetDevice(0) == 0
    assert hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
    return free.value


def test_reselecting_devices_releases_every_subsystem(gpulib, shards, golden, monkeypatch):
    ih = hashlib.sha512(b'hello').digest()
    batch = golden('batch_kats.json')['kats']
    batch_objs = [(k['target'], bytes.fromhex(k['ih'])) for k in batch]
    batch_want = [[k['trial'], k['nonce']] for k in batch]
    trials = [oracle.trial(n, ih) for n in range(1, 4097)]
    probe_want = (min(trials), 1 + trials.index(min(trials)))
    rng = random.Random(20)
    objs = [bytes(8) + rng.randbytes(rng.randrange(8, 301)) for _ in range(4096)]
    pow_want = [targets.pow_value(o) for o in objs]
    free = []
    for layout in LAYOUTS:
        shards(layout)
        free.append(device_free_bytes())
        assert proofofwork.run(2 ** 64 // 1000, ih) == [2417842470843601, 1315]
        assert proofofwork.run(184467440737095, ih) == [141019321561983, 129430]
        assert proofofwork.run_batch(batch_objs) == batch_want
        m, a = ctypes.c_uint64(), ctypes.c_uint64()
        assert gpulib.bmpow_min_trial(ih, 1, 4096, ctypes.byref(m), ctypes.byref(a)) == 0
        assert (m.value, a.value) == probe_want
        monkeypatch.delenv('BMPOW_VBINNED', raising=False)
        assert verify.pow_values(objs) == pow_want
        monkeypatch.setenv('BMPOW_VBINNED', '1')  # read per call
        assert verify.pow_values(objs) == pow_want
        monkeypatch.delenv('BMPOW_VBINNED')
        g = addressgen.deterministic_addresses(SAMPLE_SEED, 1, 1)[0]  # one null byte: the 16-bit comb table
        assert (g['k'], g['ripe'].hex()) == (21, SAMPLE_DET_RIPE)
    drop = free[1] - free[3]
    print('free MiB after each re-selection: %s; drop from the second to the fourth: %.1f MiB (bound %.1f)'
          % ([round(f / MIB, 1) for f in free], drop / MIB, BOUND / MIB))
    assert drop <= BOUND
