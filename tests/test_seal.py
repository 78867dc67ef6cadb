"""The device seal without a GPU: the seal kernels' per-row code and the set planner as a stand-alone
program under AddressSanitizer + UBSan (tests/native/seal_sim.cpp, against libcrypto); the planner again
through the library's host-only probe ``bmpow_seal_plan``; the argument checks of the new calls that return
before any device is touched; the mode knob; and the published AES-256 vectors against the library's host
code (libcrypto), which pins the constants tests/test_gpu_seal.py shares."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from pybitmessage_amd import _lib, ecies, sender
from tests.conftest import ROOT

HEADER = os.path.join(ROOT, 'include', 'bmpow_seal.h')
CSRC = os.path.join(ROOT, 'pybitmessage_amd', 'csrc')
PU8, P64, PU32 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32)

SET_ROWS = 1 << 18
SET_BYTES = 256 << 20

# FIPS-197 C.3: one block under the key 00 01 .. 1f (CBC with a zero IV is the bare cipher on the first block)
C3_KEY = bytes(range(32))
C3_PLAIN = bytes.fromhex('00112233445566778899aabbccddeeff')
C3_CIPHER = bytes.fromhex('8ea2b7ca516745bfeafc49904b496089')
# SP 800-38A F.2.5 (CBC-AES256.Encrypt); the fifth block is the PKCS#7 padding block behind the four
F25_KEY = bytes.fromhex('603deb1015ca71be2b73aef0857d77811f352c073b6108d72d9810a30914dff4')
F25_IV = bytes(range(16))
F25_PLAIN = bytes.fromhex('6bc1bee22e409f96e93d7e117393172a' 'ae2d8a571e03ac9c9eb76fac45af8e51'
                          '30c81c46a35ce411e5fbc1191a0a52ef' 'f69f2445df4f9b17ad2b417be66c3710')
F25_CIPHER = bytes.fromhex('f58c4c04d6e5f1ba779eabfb5f7bfbd6' '9cfc4e967edb808d679f777bc6702c7d'
                           '39f23369a9d9bacfa530e26304231461' 'b2eb05e2c39be9fcda6c19078c6a9d1b'
                           '3f461796d6b0d6b2e0c2a72b4d80e644')

FULL_R = bytes([0x11] * 64)  # a point field with no leading zero byte: the head is 86 bytes


def host_cbc_encrypt(key_e, iv, plain):
    """AES-256-CBC by the host's sealer (libcrypto): the ciphertext part of ``sender.seal``'s blob."""
    blob = sender.seal(plain, iv, FULL_R, key_e + bytes(32))
    return blob[86:-32]


def host_cbc_decrypt(key_e, iv, cipher):
    """The same the other way by ``ecies.decrypt`` (libcrypto): a payload around the ciphertext."""
    return ecies.decrypt(iv + b'\x02\xca\x00\x20' + FULL_R[:32] + b'\x00\x20' + FULL_R[32:] + cipher + bytes(32), key_e)


@pytest.fixture(scope='module')
def hostlib():
    return _lib.load()


def test_every_declared_symbol_is_exported_and_bound(hostlib):
    text = open(HEADER).read()
    syms = sorted(set(re.findall(r'BMPOW_API\s+[\w\s\*]+?\b(\w+)\s*\(', text)))
    assert syms == ['bmpow_aes256_cbc', 'bmpow_ecies_seal_batch', 'bmpow_seal_get_stats', 'bmpow_seal_plan',
                    'bmpow_seal_reset_stats', 'bmpow_send_set_seal']
    assert syms == sorted(name for name, _, _ in _lib.SEAL_SIGNATURES)
    raw = ctypes.CDLL(_lib.lib_path())
    for name, res, args in _lib.SEAL_SIGNATURES:
        assert hasattr(raw, name), name
        fn = getattr(hostlib, name)
        assert fn.restype == res and list(fn.argtypes) == args, name
    for header in ('bmpow_send.h', 'bmpow_ecies.h'):  # both carry the new calls along
        assert '#include "bmpow_seal.h"' in open(os.path.join(ROOT, 'include', header)).read()


def test_stats_struct_matches_the_header():
    text = open(HEADER).read()
    body = re.search(r'typedef struct bmpow_seal_stats \{(.*?)\} bmpow_seal_stats;', text, re.S).group(1)
    declared = re.findall(r'^\s*(uint64_t|double)\s+(\w+);', body, re.M)
    ctype = {'uint64_t': ctypes.c_uint64, 'double': ctypes.c_double}
    assert [(n, ctype[t]) for t, n in declared] == list(_lib.BmpowSealStats._fields_)
    assert [n for _, n in declared] == ['calls', 'rows_device', 'rows_host', 'sets', 'launches', 'seal_kernel_ms',
                                        'pack_ms', 'copy_ms', 'scatter_ms']


# ------------------------------------------------------------------ the kernels' row code on the host
def test_row_code_and_planner_under_sanitizers(tmp_path):
    """A program of its own (its own main, the sanitizer runtimes linked in), never loaded into this
    process: every head length 22..86 crossed with plaintext lengths 0..64 and a few long rows, raw CBC
    both ways with libcrypto's padding verdicts, the two published vectors, and the planner's shapes."""
    exe = tmp_path / 'seal_sim'
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-Werror', '-Wno-unknown-pragmas',
                           '-fsanitize=undefined,address', '-fno-sanitize-recover=all', '-static-libasan',
                           '-static-libubsan', '-I', CSRC, os.path.join(ROOT, 'tests', 'native', 'seal_sim.cpp'),
                           os.path.join(CSRC, 'bmpow_seal_plan.cpp'), '-o', str(exe), '-lcrypto'])
    env = dict(os.environ)
    env['ASAN_OPTIONS'] = 'halt_on_error=1 detect_leaks=1'
    env['UBSAN_OPTIONS'] = 'halt_on_error=1 print_stacktrace=1'
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    assert 'all seal checks passed' in r.stderr
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr


# ------------------------------------------------------------------ the planner through the library
def slot_bytes(length):
    """bmseal::seal_slot_bytes restated: the plaintext at 96, the blob, the padded hash blocks."""
    clen = 16 * (length // 16 + 1)
    need = max((clen + 95 + 63) // 64 * 64, clen + 118)
    assert need >= 96 + clen
    return (need + 15) // 16 * 16


def plan(hostlib, lens, max_rows=SET_ROWS, max_bytes=SET_BYTES):
    n = len(lens)
    arr = np.asarray(lens, dtype=np.uint64)
    sets = np.zeros(max(n, 1), dtype=np.uint32)
    offs = np.zeros(max(n, 1), dtype=np.uint64)
    rc = hostlib.bmpow_seal_plan(n, arr.ctypes.data_as(P64), max_rows, max_bytes, sets.ctypes.data_as(PU32),
                                 offs.ctypes.data_as(P64))
    return rc, sets[:n].astype(np.int64), offs[:n].astype(np.int64)


def check_plan(lens, rc, sets, offs, max_rows, max_bytes):
    n = len(lens)
    assert rc == (int(sets[-1]) + 1 if n else 0)
    if n == 0:
        return
    uniq, inv = np.unique(lens, return_inverse=True)
    slots = np.array([slot_bytes(int(u)) for u in uniq], dtype=np.int64)[inv]
    assert sets[0] == 0 and set(np.diff(sets).tolist()) <= {0, 1}
    assert not (offs % 16).any() and not (slots % 16).any()
    first = np.flatnonzero(np.diff(sets, prepend=-1))  # the first row of every set
    assert not offs[first].any()
    same = np.diff(sets) == 0
    assert (offs[1:][same] == (offs + slots)[:-1][same]).all()  # slots follow each other: no gap, no overlap
    counts = np.diff(np.append(first, n))
    assert counts.max() <= max_rows
    ends = (offs + slots)[np.append(first[1:], n) - 1]
    assert ((ends <= max_bytes) | (counts == 1)).all()
    # greedy: a set is closed only when the next row would not fit
    for k in range(1, len(first)):
        i = first[k]
        assert counts[k - 1] == max_rows or ends[k - 1] + slots[i] > max_bytes


@pytest.mark.parametrize('lens,max_rows,max_bytes,want_sets', [
    ([], SET_ROWS, SET_BYTES, 0),
    ([0], SET_ROWS, SET_BYTES, 1),
    ([0, 15, 16], SET_ROWS, SET_BYTES, 1),
    ([16] * SET_ROWS, SET_ROWS, SET_BYTES, 1),
    ([16] * (SET_ROWS + 1), SET_ROWS, SET_BYTES, 2),
    ([200] * 10, SET_ROWS, 10 * 336, 1),       # the byte cap met exactly (a 200-byte row's slot is 336)
    ([200] * 10, SET_ROWS, 10 * 336 - 1, 2),   # crossed by one byte
    ([200] * 11, SET_ROWS, 10 * 336, 2),
    ([300000, 16, 16], SET_ROWS, 1000, 2),     # a row alone above the byte cap
    ([16, 300000, 16], SET_ROWS, 1000, 3),
    ([2 ** 31 - 17, 2 ** 31 - 17, 0], SET_ROWS, SET_BYTES, 3),
    ([5, 4, 3, 2, 1], 2, SET_BYTES, 3),
], ids=['empty', 'one', 'lens_0_15_16', 'full_set', 'full_set_plus_one', 'bytes_exact', 'bytes_plus_one',
        'bytes_one_row_more', 'big_row_first', 'big_row_between', 'longest_rows', 'row_cap_2'])
def test_seal_plan_shapes(hostlib, lens, max_rows, max_bytes, want_sets):
    assert slot_bytes(200) == 336
    rc, sets, offs = plan(hostlib, lens, max_rows, max_bytes)
    assert rc == want_sets
    check_plan(np.asarray(lens, dtype=np.int64), rc, sets, offs, max_rows, max_bytes)


def test_seal_plan_argument_errors(hostlib):
    one = np.array([5], dtype=np.uint64)
    s, o = np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.uint64)
    args = (one.ctypes.data_as(P64), SET_ROWS, SET_BYTES, s.ctypes.data_as(PU32), o.ctypes.data_as(P64))
    assert hostlib.bmpow_seal_plan(1, *args) == 1
    assert hostlib.bmpow_seal_plan(1, None, *args[1:]) == _lib.E_ARG
    assert hostlib.bmpow_seal_plan(1, args[0], SET_ROWS, SET_BYTES, None, args[4]) == _lib.E_ARG
    assert hostlib.bmpow_seal_plan(1, args[0], SET_ROWS, SET_BYTES, args[3], None) == _lib.E_ARG
    assert hostlib.bmpow_seal_plan(1, args[0], 0, SET_BYTES, args[3], args[4]) == _lib.E_ARG
    assert hostlib.bmpow_seal_plan(1, args[0], SET_ROWS, 0, args[3], args[4]) == _lib.E_ARG
    over = np.array([2 ** 31 - 16], dtype=np.uint64)
    assert hostlib.bmpow_seal_plan(1, over.ctypes.data_as(P64), *args[1:]) == _lib.E_ARG
    huge = np.array([2 ** 64 - 1], dtype=np.uint64)
    assert hostlib.bmpow_seal_plan(1, huge.ctypes.data_as(P64), *args[1:]) == _lib.E_ARG
    assert hostlib.bmpow_seal_plan(0, None, SET_ROWS, SET_BYTES, None, None) == 0


# ------------------------------------------------------------------ argument errors before any device
def test_new_calls_refuse_bad_arguments_without_a_device(hostlib):
    plain = b'x' * 20
    pp = (ctypes.c_char_p * 1)(plain)
    lens = np.array([20], dtype=np.uint64)
    cap = sender.blob_cap(20)
    out = np.zeros(cap, dtype=np.uint8)
    outs = np.array([out.ctypes.data], dtype=np.uint64)
    caps = np.array([cap], dtype=np.uint64)
    got = np.zeros(1, dtype=np.uint64)
    vp = ctypes.c_void_p
    good = [ctypes.cast(pp, vp), lens.ctypes.data_as(P64), bytes(16), bytes(64), bytes(64), outs.ctypes.data_as(vp),
            caps.ctypes.data_as(P64), got.ctypes.data_as(P64)]
    assert hostlib.bmpow_ecies_seal_batch(0, *([None] * 8)) == 0
    for hole in range(8):
        args = list(good)
        args[hole] = None
        assert hostlib.bmpow_ecies_seal_batch(1, *args) == _lib.E_ARG, hole
    short = np.array([cap - 1], dtype=np.uint64)
    assert hostlib.bmpow_ecies_seal_batch(1, *good[:6], short.ctypes.data_as(P64), good[7]) == _lib.E_ARG
    assert b'BMPOW_ECIES_BLOB_CAP' in hostlib.bmpow_last_error()
    long = np.array([2 ** 31 - 16], dtype=np.uint64)
    assert hostlib.bmpow_ecies_seal_batch(1, good[0], long.ctypes.data_as(P64), *good[2:]) == _lib.E_ARG
    nullrow = np.zeros(1, dtype=np.uint64)
    assert hostlib.bmpow_ecies_seal_batch(1, *good[:5], nullrow.ctypes.data_as(vp), *good[6:]) == _lib.E_ARG

    got64 = np.zeros(1, dtype=np.int64)
    pi64 = ctypes.POINTER(ctypes.c_int64)
    cgood = [bytes(32), bytes(16), ctypes.cast(pp, vp), lens.ctypes.data_as(P64), outs.ctypes.data_as(vp),
             caps.ctypes.data_as(P64), got64.ctypes.data_as(pi64)]
    for decrypt in (0, 1):
        assert hostlib.bmpow_aes256_cbc(0, decrypt, *([None] * 7)) == 0
        for hole in range(7):
            args = list(cgood)
            args[hole] = None
            assert hostlib.bmpow_aes256_cbc(1, decrypt, *args) == _lib.E_ARG, (decrypt, hole)
    small = np.array([31], dtype=np.uint64)  # 20 bytes pad to 32
    assert hostlib.bmpow_aes256_cbc(1, 0, *cgood[:5], small.ctypes.data_as(P64), cgood[6]) == _lib.E_ARG
    ct = np.array([32], dtype=np.uint64)
    pc = (ctypes.c_char_p * 1)(b'c' * 32)
    assert hostlib.bmpow_aes256_cbc(1, 1, cgood[0], cgood[1], ctypes.cast(pc, vp), ct.ctypes.data_as(P64), cgood[4],
                                    small.ctypes.data_as(P64), cgood[6]) == _lib.E_ARG
    assert hostlib.bmpow_aes256_cbc(1, 0, cgood[0], cgood[1], cgood[2], long.ctypes.data_as(P64), *cgood[4:]) == _lib.E_ARG
    # a ciphertext that is empty or no multiple of 16 is that row's verdict, not an error; nothing is launched
    for bad_len in (0, 17):
        got64[0] = 5
        bl = np.array([bad_len], dtype=np.uint64)
        assert hostlib.bmpow_aes256_cbc(1, 1, cgood[0], cgood[1], ctypes.cast(pc, vp), bl.ctypes.data_as(P64),
                                        *cgood[4:]) == 0
        assert got64[0] == -1
    assert hostlib.bmpow_seal_get_stats(None) == _lib.E_ARG


def test_python_wrappers_check_sizes_first():
    with pytest.raises(ValueError):
        sender.seal_batch([b'p'], [bytes(15)], [bytes(64)], [bytes(64)])
    with pytest.raises(ValueError):
        sender.seal_batch([b'p'], [bytes(16)], [bytes(63)], [bytes(64)])
    with pytest.raises(ValueError):
        sender.seal_batch([b'p'], [bytes(16)], [bytes(64)], [bytes(32)])
    with pytest.raises(ValueError):
        sender.seal_batch([b'p', b'q'], [bytes(16)], [bytes(64)], [bytes(64)])
    with pytest.raises(ValueError):  # two wrong sizes that add up
        sender.seal_batch([b'p', b'q'], [bytes(15), bytes(17)], [bytes(64)] * 2, [bytes(64)] * 2)
    with pytest.raises(ValueError):
        ecies.aes_cbc_batch([bytes(31)], [bytes(16)], [b'data'])
    with pytest.raises(ValueError):
        ecies.aes_cbc_batch([bytes(32)], [bytes(17)], [b'data'])
    with pytest.raises(ValueError):
        ecies.aes_cbc_batch([bytes(32)], [bytes(16)], [b'data', b'more'])
    assert sender.seal_batch([], [], [], []) == [] and ecies.aes_cbc_batch([], [], []) == []


def test_seal_mode_knob_round_trip(hostlib):
    first = hostlib.bmpow_send_set_seal(-1)
    assert first in (0, 1) and sender.set_seal(-1) == first
    try:
        assert sender.set_seal(1) == first
        assert sender.set_seal(-1) == 1 and sender.set_seal(7) == 1 and sender.set_seal(-1) == 1
        assert sender.set_seal(0) == 1
        assert sender.set_seal(-1) == 0
    finally:
        sender.set_seal(first)
    assert sender.set_seal(-1) == first


def test_seal_mode_follows_the_environment():
    code = ('import sys; sys.path.insert(0, %r); from pybitmessage_amd import sender; print(sender.set_seal(-1))' % ROOT)
    for value, want in (('device', '1'), ('host', '0')):
        env = dict(os.environ, BMPOW_SEAL=value)
        assert subprocess.check_output([sys.executable, '-c', code], env=env).decode().strip() == want


def test_seal_stats_start_at_zero_and_reset(hostlib):
    sender.reset_seal_stats()
    st = sender.seal_stats()
    assert set(st) == {f for f, _ in _lib.BmpowSealStats._fields_} and not any(st.values())


# ------------------------------------------------------------------ the vectors, by the host's libcrypto
def test_published_vectors_by_the_host_code():
    assert host_cbc_encrypt(C3_KEY, bytes(16), C3_PLAIN)[:16] == C3_CIPHER
    assert len(F25_PLAIN) == 64 and len(F25_CIPHER) == 80
    assert host_cbc_encrypt(F25_KEY, F25_IV, F25_PLAIN) == F25_CIPHER
    assert host_cbc_decrypt(F25_KEY, F25_IV, F25_CIPHER) == F25_PLAIN
    c3 = host_cbc_encrypt(C3_KEY, bytes(16), C3_PLAIN)
    assert len(c3) == 32 and host_cbc_decrypt(C3_KEY, bytes(16), c3) == C3_PLAIN
    assert host_cbc_decrypt(F25_KEY, F25_IV, F25_CIPHER[:64]) is None  # the fourth block ends in 0x10 0x37 0x10: no padding
