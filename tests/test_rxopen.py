"""The one-call opening of received msgs without a GPU (include/bmpow_rxopen.h): the opening kernel's per-row
code as a stand-alone program under AddressSanitizer + UBSan (tests/native/rxopen_sim.cpp, against libcrypto);
the host's plan of an object (``bmpow_rx_sealed_plan``) against ``ecies.msg_payload`` and ``ecies.parse`` on the
fixture's msgs and on refusals; the declared symbols and the stats struct; and the argument checks that return
before any device is touched."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from pybitmessage_amd import _lib, ecies, receive
from tests.conftest import ROOT, load_golden

HEADER = os.path.join(ROOT, 'include', 'bmpow_rxopen.h')
CSRC = os.path.join(ROOT, 'pybitmessage_amd', 'csrc')


@pytest.fixture(scope='module')
def kats():
    return load_golden('rx_kats.json')


@pytest.fixture(scope='module')
def hostlib():
    return _lib.load()


def test_every_declared_symbol_is_exported_and_bound(hostlib):
    text = open(HEADER).read()
    syms = sorted(set(re.findall(r'BMPOW_API\s+[\w\s\*]+?\b(\w+)\s*\(', text)))
    assert syms == ['bmpow_rx_sealed_get_stats', 'bmpow_rx_sealed_msgs', 'bmpow_rx_sealed_plan',
                    'bmpow_rx_sealed_reset_stats']
    assert syms == sorted(name for name, _, _ in _lib.RXOPEN_SIGNATURES)
    raw = ctypes.CDLL(_lib.lib_path())
    for name, res, args in _lib.RXOPEN_SIGNATURES:
        assert hasattr(raw, name), name
        fn = getattr(hostlib, name)
        assert fn.restype == res and list(fn.argtypes) == args, name
    for other in (_lib.RX_SIGNATURES, _lib.RXOBJ_SIGNATURES, _lib.ECIES_SIGNATURES):
        assert not set(syms) & set(name for name, _, _ in other)
    # bmpow_rx.h does not need the new header; its remark on NOT_MINE names the call that now sets it
    rx = open(os.path.join(ROOT, 'include', 'bmpow_rx.h')).read()
    assert 'bmpow_rxopen.h' not in [line.split('"')[1] for line in rx.splitlines() if line.startswith('#include "')]
    assert 'never set by this library' not in rx.split('BMPOW_RX_NOT_MINE 2')[1].split('\n')[0]


def test_stats_struct_matches_the_header():
    text = open(HEADER).read()
    body = re.search(r'typedef struct bmpow_rx_sealed_stats \{(.*?)\} bmpow_rx_sealed_stats;', text, re.S).group(1)
    declared = re.findall(r'^\s*(uint64_t|double)\s+(\w+);', body, re.M)
    ctype = {'uint64_t': ctypes.c_uint64, 'double': ctypes.c_double}
    assert [(n, ctype[t]) for t, n in declared] == list(_lib.BmpowRxSealedStats._fields_)
    names = [n for _, n in declared]
    for want in ('calls', 'rows', 'matched', 'sets', 'launches', 'match_ms', 'open_ms', 'walk_ms', 'hash_ms', 'scalar_ms',
                 'curve_ms', 'ident_ms', 'finish_ms', 'bytes_up', 'bytes_down', 'host_ms'):
        assert want in names, want


# ------------------------------------------------------------------ the kernel's row code on the host
def test_row_code_under_sanitizers(tmp_path):
    """A program of its own (its own main, the sanitizer runtimes linked in), never loaded into this process:
    every source alignment 0..15 inside a pool row of exactly its size, ciphertexts of 1, 2, 3, 4, 5 and 17
    blocks, every plaintext length mod 16, every head length 22..86, and every shape of bad padding, each against
    libcrypto's verdict and bytes."""
    exe = tmp_path / 'rxopen_sim'
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-Werror', '-Wno-unknown-pragmas',
                           '-fsanitize=undefined,address', '-fno-sanitize-recover=all', '-static-libasan',
                           '-static-libubsan', '-I', CSRC, os.path.join(ROOT, 'tests', 'native', 'rxopen_sim.cpp'),
                           '-o', str(exe), '-lcrypto'])
    env = dict(os.environ)
    env['ASAN_OPTIONS'] = 'halt_on_error=1 detect_leaks=1'
    env['UBSAN_OPTIONS'] = 'halt_on_error=1 print_stacktrace=1'
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    assert 'all rxopen checks passed' in r.stderr
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr


# ------------------------------------------------------------------ the plan of one object
def test_plan_agrees_with_the_python_parsers_on_every_fixture_msg(kats):
    seen = set()
    for m in kats['msgs']:
        obj = bytes.fromhex(m['obj'])
        ok, reason, payload_off, body_off, clen = receive.sealed_plan(obj)
        payload = ecies.msg_payload(obj)
        seen.add(reason)
        if m['line'] == 444:
            assert payload is None and (ok, reason) == (False, receive.PLAN_HEAD), m['name']
            assert (payload_off, body_off, clen) == (0, 0, 0)
            continue
        assert payload is not None and obj[payload_off:] == payload, m['name']
        parsed = ecies.parse(payload)
        assert parsed is not None and (ok, reason) == (True, receive.PLAN_OK), m['name']
        assert body_off == parsed[2] and clen == len(payload) - 32 - body_off and clen % 16 == 0 and clen > 0
        # the ciphertext the plan names is the one that decrypts to the fixture's plaintext
        assert clen == 16 * (len(m['plaintext']) // 2 // 16 + 1) or not m['decrypts'], m['name']
    assert seen == {receive.PLAN_OK, receive.PLAN_HEAD}


def _head(stream=b'\x01', version=b'\x01'):
    return bytes(range(16)) + b'\x00\x00\x00\x02' + version + stream


def _payload(clen, xl=32, yl=32):
    return (bytes(16) + b'\x02\xca' + xl.to_bytes(2, 'big') + b'\x11' * xl + yl.to_bytes(2, 'big') + b'\x22' * yl +
            b'\x33' * clen + b'\x44' * 32)


def test_plan_refusals():
    good = _head() + _payload(48)
    assert receive.sealed_plan(good) == (True, receive.PLAN_OK, 22, 86, 48)
    # odd coordinate lengths, as a sender that strips leading zero bytes writes them
    assert receive.sealed_plan(_head() + _payload(16, 31, 30)) == (True, receive.PLAN_OK, 22, 83, 16)
    assert receive.sealed_plan(_head(b'\xfd\x01\x2c') + _payload(16, 0, 0)) == (True, receive.PLAN_OK, 24, 22, 16)
    # the head: a varint that is not minimal or is cut short, another msg version, nothing behind the header
    for head in (_head(version=b'\xfd\x00\x01'), _head(b'\xfd\x00\x10'), _head(b'\xfe\x00\x00\x01\x00'), _head(version=b'\x02')):
        assert ecies.msg_payload(head + _payload(48)) is None
        assert receive.sealed_plan(head + _payload(48)) == (False, receive.PLAN_HEAD, 0, 0, 0)
    for cut in (bytes(20), bytes(20) + b'\xfd\x00', _head(b'\xfd\x01'), _head(b'\xff' + bytes(5)), b''):
        assert ecies.msg_payload(cut) is None
        assert receive.sealed_plan(cut) == (False, receive.PLAN_HEAD, 0, 0, 0)
    # a payload shorter than its header says, by every count
    whole = _payload(0)
    for keep in list(range(0, 20)) + [21, 52, 53, 54, 85, 86, 117]:
        obj = _head() + whole[:keep]
        assert ecies.parse(obj[22:]) is None
        assert receive.sealed_plan(obj) == (False, receive.PLAN_PAYLOAD, 22, 0, 0), keep
    assert receive.sealed_plan(_head() + b'') == (False, receive.PLAN_PAYLOAD, 22, 0, 0)
    # a ciphertext of 0 and of 8 bytes, and of one byte more than a block: tried, never opened
    for clen in (0, 8, 17):
        obj = _head() + _payload(clen)
        assert ecies.parse(obj[22:])[2] == 86
        assert receive.sealed_plan(obj) == (False, receive.PLAN_CIPHER, 22, 86, clen)
    # a stream varint that ends the object: the payload is empty
    assert receive.sealed_plan(bytes(20) + b'\x01') == (False, receive.PLAN_PAYLOAD, 21, 0, 0)
    assert ecies.msg_payload(bytes(20) + b'\x01') == b''


def test_plan_null_pointers(hostlib):
    z = ctypes.c_size_t(0)
    r = ctypes.c_int(0)
    assert hostlib.bmpow_rx_sealed_plan(b'x', 1, None, ctypes.byref(z), ctypes.byref(z), ctypes.byref(r)) == _lib.E_ARG
    assert hostlib.bmpow_rx_sealed_plan(None, 1, ctypes.byref(z), ctypes.byref(z), ctypes.byref(z), ctypes.byref(r)) == _lib.E_ARG
    assert hostlib.bmpow_rx_sealed_plan(None, 0, ctypes.byref(z), ctypes.byref(z), ctypes.byref(z), ctypes.byref(r)) == 0
    assert r.value == receive.PLAN_HEAD


# ------------------------------------------------------------------ arguments, before any device
def test_argument_errors_before_any_device(hostlib):
    obj = _head() + _payload(48)
    ripe, key = bytes(20), bytes(31) + b'\x01'
    with pytest.raises(ValueError):
        receive.open_sealed_msgs([obj], {ripe: bytes(33)})        # a key longer than 32 bytes
    with pytest.raises(ValueError):
        receive.open_sealed_msgs([obj], {bytes(19): key})          # a ripe is 20 bytes
    with pytest.raises(ValueError):
        receive.open_sealed_msgs([obj], ([ripe, ripe], [key]))     # one ripe per key
    with pytest.raises(ValueError):
        receive.process_sealed_msgs([obj], ([ripe], [key, key]))
    # the library's own checks that come before it looks for a device
    recs = np.zeros(1, dtype=receive.MSG_REC)
    match = np.zeros(1, dtype=np.int32)
    off, ln = np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint64)
    arena = np.zeros(len(obj), dtype=np.uint8)
    ptrs = (ctypes.c_char_p * 1)(obj)
    lens = np.array([len(obj)], dtype=np.uint64)
    p64 = ctypes.POINTER(ctypes.c_uint64)

    def call(n=1, objs=ptrs, keys=key, n_keys=1, cap=len(obj), recs_at=recs.ctypes.data):
        return hostlib.bmpow_rx_sealed_msgs(n, ctypes.cast(objs, ctypes.c_void_p), lens.ctypes.data_as(p64), n_keys, keys,
                                            ripe, recs_at, match.ctypes.data, arena.ctypes.data, cap, off.ctypes.data,
                                            ln.ctypes.data)

    assert call(n=0) == 0
    assert call(recs_at=None) == _lib.E_ARG
    assert call(cap=len(obj) - 1) == _lib.E_ARG                   # the arena, one byte too small
    assert b'arena' in hostlib.bmpow_last_error()
    assert call(keys=bytes(32)) == _lib.E_ARG                      # the key 0
    order = bytes.fromhex('fffffffffffffffffffffffffffffffebaaedce6af48a03bbfd25e8cd0364141')
    assert call(keys=order) == _lib.E_ARG                          # the group order itself
    assert b'private key' in hostlib.bmpow_last_error()
    # heads that refuse and no keys at all never reach a device: the records are the host's
    bad = _head(version=b'\x02') + _payload(48)
    ptrs_bad = (ctypes.c_char_p * 1)(bad)
    assert call(objs=ptrs_bad) == 0
    assert (int(recs['status'][0]), int(match[0]), int(ln[0])) == (receive.MSG_VERSION, -1, 0)
    want, _ = receive.walk_msg(bad, b'', ripe)
    assert recs.tobytes() == want.recs.tobytes()
    assert call(n_keys=0, keys=None) == 0
    assert (int(recs['status'][0]), int(match[0]), int(ln[0])) == (receive.NOT_MINE, -1, 0)
    assert (int(recs['claimed_stream'][0]), int(recs['prefix_len'][0])) == (1, 14)
    only = np.zeros(1, dtype=receive.MSG_REC)
    only['status'], only['claimed_stream'], only['prefix_len'] = receive.NOT_MINE, 1, 14
    assert recs.tobytes() == only.tobytes()
