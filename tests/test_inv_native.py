"""The inventory sets' slot steps, key load and payload walk as a stand-alone program under AddressSanitizer +
UBSan (tests/native/inv_sim.cpp builds pybitmessage_amd/csrc/bmpow_inv_fmt.h with g++): no device, and no
sanitizer in this process."""
import os
import subprocess

from tests.conftest import ROOT

CSRC = os.path.join(ROOT, 'pybitmessage_amd', 'csrc')


def test_inv_sim_under_sanitizers(tmp_path):
    """A program of its own (its own main, the sanitizer runtimes linked in), never loaded into this process:
    seeded random adds, lookups, removes and rebuilds on tables of 8 to 64 slots through the functions the
    kernels call, against std::unordered_map; the walk over heap blocks of every cut length; the unaligned key
    load for every residue from a block that ends on the item's last byte.  A single-threaded model: it checks
    the slot logic and the memory accesses, and cannot show the kernels' races."""
    exe = tmp_path / 'inv_sim'
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-Werror', '-Wno-unknown-pragmas',
                           '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-static-libasan',
                           '-static-libubsan', '-I', CSRC, os.path.join(ROOT, 'tests', 'native', 'inv_sim.cpp'),
                           '-o', str(exe)])
    env = dict(os.environ)
    env['ASAN_OPTIONS'] = 'halt_on_error=1 detect_leaks=1'
    env['UBSAN_OPTIONS'] = 'halt_on_error=1 print_stacktrace=1'
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    assert 'all inv checks passed' in r.stderr
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr
