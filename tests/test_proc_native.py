"""The dispatch's watch probe, byte compare, mix and walks as a stand-alone program under AddressSanitizer + UBSan
(tests/native/proc_sim.cpp builds pybitmessage_amd/csrc/bmpow_proc_fmt.h with g++): no device, and no sanitizer in
this process."""
import os
import subprocess

from tests.conftest import ROOT

CSRC = os.path.join(ROOT, 'pybitmessage_amd', 'csrc')


def test_proc_sim_under_sanitizers(tmp_path):
    """A program of its own (its own main, the sanitizer runtimes linked in), never loaded into this process:
    seeded random watch sets of 0 to 40 keys through the functions the kernels call, against std::unordered_map;
    the key compare and the mix on heap blocks that end on the run's last byte, for every offset residue mod 8 and
    every length from 16 to 48; both walks over every cut length of a valid object, from blocks that hold exactly
    the uploaded bytes.  A single-threaded model: it checks the logic and the memory accesses, and cannot show the
    kernels' meeting at first[]."""
    exe = tmp_path / 'proc_sim'
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-Werror', '-Wno-unknown-pragmas',
                           '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-static-libasan',
                           '-static-libubsan', '-I', CSRC, os.path.join(ROOT, 'tests', 'native', 'proc_sim.cpp'),
                           '-o', str(exe)])
    env = dict(os.environ)
    env['ASAN_OPTIONS'] = 'halt_on_error=1 detect_leaks=1'
    env['UBSAN_OPTIONS'] = 'halt_on_error=1 print_stacktrace=1'
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    assert 'all proc checks passed' in r.stderr
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr
