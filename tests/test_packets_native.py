"""The packet kernels' byte logic and the frame walk as a stand-alone program under AddressSanitizer + UBSan
(tests/native/packets_sim.cpp builds pybitmessage_amd/csrc/bmpow_packets_fmt.h with g++): no device, and no
sanitizer in this process."""
import os
import subprocess

from tests.conftest import ROOT

CSRC = os.path.join(ROOT, 'pybitmessage_amd', 'csrc')


def test_packets_sim_under_sanitizers(tmp_path):
    """A program of its own (its own main, the sanitizer runtimes linked in), never loaded into this process:
    the pack for every source residue 0 .. 15, every length 0 .. 300 and both kinds, from a heap block of exactly
    the arena's size into one of exactly the pool's, rows that end on the arena's last byte among them, against
    data || 0x80 || zeros || bit length; and the frame walk over heap blocks of every cut length."""
    exe = tmp_path / 'packets_sim'
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-Werror', '-Wno-unknown-pragmas',
                           '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-static-libasan',
                           '-static-libubsan', '-I', CSRC, os.path.join(ROOT, 'tests', 'native', 'packets_sim.cpp'),
                           '-o', str(exe)])
    env = dict(os.environ)
    env['ASAN_OPTIONS'] = 'halt_on_error=1 detect_leaks=1'
    env['UBSAN_OPTIONS'] = 'halt_on_error=1 print_stacktrace=1'
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    assert 'all packets checks passed' in r.stderr
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr
