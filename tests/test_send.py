"""The send side, the parts that need no device: the ABI table of ``include/bmpow_send.h``,
``bmpow_sig_der`` against the oracle's encoder and back through ``bmpow_sig_parse``, ``bmpow_ecies_seal``
against every blob the reference made (``tests/golden/send_kats.json``, tests/golden/make_send_golden.py)
with the key derived by the integer oracle, the fixture's signatures against the oracle,
``worker.msg_plaintext`` against the fixture layout ``signatures.msg_signed_parts`` reads, and the host
units' scalar and byte toolkit as a stand-alone program under the sanitizers
(tests/native/hostscalar_sim.cpp)."""
import ctypes
import hashlib
import itertools
import re
import os
import subprocess

import pytest

from oracle import ecdsa_oracle as eo
from pybitmessage_amd import _lib, sender, signatures, worker
from tests.conftest import ROOT

HEADER = os.path.join(ROOT, 'include', 'bmpow_send.h')
N = eo.N
_PU8 = ctypes.POINTER(ctypes.c_uint8)


@pytest.fixture(scope='module')
def kats(golden):
    return golden('send_kats.json')


@pytest.fixture(scope='module')
def hostlib():
    return _lib.load()


def b32(v):
    return v.to_bytes(32, 'big')


def test_every_declared_symbol_is_exported_and_bound(hostlib):
    text = open(HEADER).read()
    syms = sorted(set(re.findall(r'BMPOW_API\s+[\w\s\*]+?\b(\w+)\s*\(', text)))
    assert syms == ['bmpow_ec_pubkeys', 'bmpow_ecdsa_sign_digest', 'bmpow_ecies_encrypt', 'bmpow_ecies_seal',
                    'bmpow_send_get_stats', 'bmpow_send_reset_stats', 'bmpow_sig_der', 'bmpow_sig_sign']
    assert syms == sorted(name for name, _, _ in _lib.SEND_SIGNATURES)
    raw = ctypes.CDLL(_lib.lib_path())
    for name, res, args in _lib.SEND_SIGNATURES:
        assert hasattr(raw, name), name
        fn = getattr(hostlib, name)
        assert fn.restype == res and list(fn.argtypes) == args, name


def test_stats_struct_matches_the_header():
    text = open(HEADER).read()
    body = re.search(r'typedef struct bmpow_send_stats \{(.*?)\} bmpow_send_stats;', text, re.S).group(1)
    declared = re.findall(r'^\s*(uint64_t|double)\s+(\w+);', body, re.M)
    ctype = {'uint64_t': ctypes.c_uint64, 'double': ctypes.c_double}
    assert [(name, ctype[t]) for t, name in declared] == list(_lib.BmpowSendStats._fields_)
    assert ctypes.sizeof(_lib.BmpowSendStats) == 8 * len(declared)


def test_blob_cap_macro_and_python_agree():
    text = open(HEADER).read()
    assert '#define BMPOW_ECIES_BLOB_CAP(len) (118 + 16 * ((size_t)(len) / 16 + 1))' in text
    for n in (0, 1, 15, 16, 17, 1000):
        assert sender.blob_cap(n) == 16 + 2 + 2 * (2 + 32) + 16 * (n // 16 + 1) + 32


DER_VALUES = (1, 0x7f, 0x80, 2 ** 248 - 1, 2 ** 255, N - 1)


@pytest.mark.parametrize('r,s', list(itertools.product(DER_VALUES, DER_VALUES)))
def test_sig_der_is_the_oracles_encoding_and_parses_back(hostlib, r, s):
    got = sender.der(b32(r) + b32(s))
    assert got == eo.der_encode(r, s)
    assert signatures.parse(got) == (b32(r), b32(s))


def test_sig_der_refuses_zero(hostlib):
    out = ctypes.create_string_buffer(72)
    ln = ctypes.c_size_t(0)
    for rs in (b32(0) + b32(5), b32(5) + b32(0)):
        assert hostlib.bmpow_sig_der(rs, ctypes.cast(out, _PU8), ctypes.byref(ln)) == _lib.E_ARG


def kat_key(kats, k):
    """key_e || key_m of a blob: SHA512(x(ephemeral * recipient point)), by the integer oracle."""
    Q = eo.key_xy(bytes.fromhex(kats['recipient_pubs'][k['recipient']]))
    shared = eo.mult(int(k['ephemeral'], 16), Q)
    return hashlib.sha512(b32(shared[0])).digest()


def test_seal_reproduces_every_reference_blob(hostlib, kats):
    short = 0
    for k in kats['encrypt_kats']:
        R = eo.xy_key(eo.mult_g(int(k['ephemeral'], 16)))
        blob = sender.seal(bytes.fromhex(k['plaintext']), bytes.fromhex(k['iv']), R, kat_key(kats, k))
        assert blob == bytes.fromhex(k['blob']), k['coord_lens']
        short += k['coord_lens'] != [32, 32]
    assert short >= 2  # the 31-byte coordinates are in
    assert {len(k['plaintext']) // 2 for k in kats['encrypt_kats']} >= {0, 1, 15, 16, 17, 100, 1000}


def test_seal_refuses_a_cap_one_byte_too_small(hostlib, kats):
    for k in (kats['encrypt_kats'][0], kats['encrypt_kats'][-1]):  # full-width and short coordinates
        R = eo.xy_key(eo.mult_g(int(k['ephemeral'], 16)))
        want = bytes.fromhex(k['blob'])
        pt, iv, key = bytes.fromhex(k['plaintext']), bytes.fromhex(k['iv']), kat_key(kats, k)
        out = ctypes.create_string_buffer(len(want))
        assert hostlib.bmpow_ecies_seal(pt, len(pt), iv, R, key, ctypes.cast(out, _PU8), len(want) - 1) == _lib.E_ARG
        assert b'smaller than the blob' in hostlib.bmpow_last_error()
        assert hostlib.bmpow_ecies_seal(pt, len(pt), iv, R, key, ctypes.cast(out, _PU8), len(want)) == len(want)
        assert out.raw == want


def test_fixture_signatures_are_the_oracles(kats):
    kinds = set()
    for k in kats['sign_kats']:
        d, nonce, msg = int(k['priv'], 16), int(k['nonce'], 16), bytes.fromhex(k['msg'])
        e = int.from_bytes(hashlib.new(k['digest'], msg).digest(), 'big')
        r, s = eo.sign(d, nonce, e)
        assert eo.der_encode(r, s) == bytes.fromhex(k['sig']), k['name']
        assert k['verdict'] is True
        assert eo.verify(msg, bytes.fromhex(k['sig']), bytes.fromhex(k['pub'])) == (1 if k['digest'] == 'sha1' else 2)
        kinds |= {'short_r'} if r < 2 ** 248 else set()
        kinds.add('s_high' if s >= 2 ** 255 else 's_low')
    assert kinds == {'short_r', 's_high', 's_low'}


def test_pointmult_fixture_is_the_oracles(kats):
    for k in kats['pointmult_kats']:
        assert bytes.fromhex(k['pub']) == b'\x04' + eo.xy_key(eo.mult_g(int(k['priv'], 16)))


@pytest.mark.parametrize('version', [2, 3, 4])
def test_msg_plaintext_is_what_the_receive_side_reads(version):
    pub_s, pub_e, ripe, ack = bytes(range(64)), bytes(range(64, 128)), b'\x07' * 20, b'A' * 70
    text = b'Subject:s\nBody:' + b'b' * 300
    plain = worker.msg_plaintext(version, 1, worker.get_bitfield(), b'\x04' + pub_s, pub_e, ripe, 2, text, ack, 2000, 3000)
    want = worker._varint(version) + worker._varint(1) + b'\x00\x00\x00\x01' + pub_s + pub_e
    if version >= 3:
        want += worker._varint(2000) + worker._varint(3000)
    want += ripe + worker._varint(2) + worker._varint(len(text)) + text + worker._varint(len(ack)) + ack
    assert plain == want
    # the receive side's walk over it ends exactly where the signature begins
    head = bytes(8) + (1760000000).to_bytes(8, 'big') + b'\x00\x00\x00\x02' + b'\x01\x01'
    sig = b'\x30' + b'S' * 70
    signed, got_sig, key = signatures.msg_signed_parts(head, plain + worker._varint(len(sig)) + sig)
    assert signed == head[8:] + plain and got_sig == sig and key == pub_s


def test_host_scalar_toolkit_under_sanitizers(tmp_path):
    """pybitmessage_amd/csrc/bmpow_host_scalar.h built alone with g++ under AddressSanitizer + UBSan
    (tests/native/hostscalar_sim.cpp), a stand-alone program that loads neither HIP nor the library: the
    range checks at 0, 1, n - 1, n, n + 1, 2^256 - 1 and around p limb by limb, the byte conversions both
    ways, the SHA padding into heap blocks of exactly msg_blocks(len) * 64 bytes, the DER encoder against
    libcrypto's i2d_ECDSA_SIG and the strict parser, the parser on the encoder's outputs bent four ways, and
    64 drawn scalars in range and distinct."""
    csrc = os.path.join(ROOT, 'pybitmessage_amd', 'csrc')
    exe = tmp_path / 'hostscalar_sim'
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-Werror', '-Wno-unknown-pragmas',
                           '-fsanitize=undefined,address', '-fno-sanitize-recover=all', '-static-libasan',
                           '-static-libubsan', '-I', csrc, os.path.join(ROOT, 'tests', 'native', 'hostscalar_sim.cpp'),
                           '-o', str(exe), '-lcrypto'])
    env = dict(os.environ)
    env['ASAN_OPTIONS'] = 'halt_on_error=1 detect_leaks=1'
    env['UBSAN_OPTIONS'] = 'halt_on_error=1 print_stacktrace=1'
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    assert 'all host scalar checks passed' in r.stderr
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr
