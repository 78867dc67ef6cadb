"""Signature verification, the parts that need no device: the ABI table of ``include/bmpow_sig.h``, the
stats struct's layout, ``bmpow_sig_parse`` (host only; the library loads without a GPU) against every
signature of the reference-made fixture ``tests/golden/sig_kats.json``
(tests/golden/make_sig_golden.py), ``scalar_dev.h`` compiled for the host as a stand-alone program
against Python integers, and the two extractors against the fixture's objects."""
import ctypes
import os
import random
import re
import subprocess

import pytest

from oracle.ecdsa_oracle import der_decode, scalar_set, sign_cases
from pybitmessage_amd import _lib, signatures
from tests.conftest import ROOT

HEADER = os.path.join(ROOT, 'include', 'bmpow_sig.h')
CSRC = os.path.join(ROOT, 'pybitmessage_amd', 'csrc')
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141


@pytest.fixture(scope='module')
def kats(golden):
    return golden('sig_kats.json')


@pytest.fixture(scope='module')
def hostlib():
    return _lib.load()


def declared_symbols():
    text = open(HEADER).read()
    return sorted(set(re.findall(r'BMPOW_API\s+[\w\s\*]+?\b(\w+)\s*\(', text)))


def test_every_declared_symbol_is_exported_and_bound(hostlib):
    syms = declared_symbols()
    assert syms == ['bmpow_ecdsa_verify_digest', 'bmpow_sig_get_stats', 'bmpow_sig_parse', 'bmpow_sig_reset_stats',
                    'bmpow_sig_verify']
    assert syms == sorted(name for name, _, _ in _lib.SIG_SIGNATURES)
    raw = ctypes.CDLL(_lib.lib_path())
    for name, res, args in _lib.SIG_SIGNATURES:
        assert hasattr(raw, name), name
        fn = getattr(hostlib, name)
        assert fn.restype == res and list(fn.argtypes) == args, name
    # the other headers' tables keep their own sets
    for other in (_lib.SIGNATURES, _lib.ECIES_SIGNATURES, _lib.INTAKE_SIGNATURES):
        assert not set(syms) & set(name for name, _, _ in other)


def test_stats_struct_matches_the_header(tmp_path):
    fields = [f for f, _ in _lib.BmpowSigStats._fields_]
    assert fields == ['calls', 'submitted', 'uploaded', 'ladders', 'launches', 'hash_ms', 'scalar_ms', 'curve_ms',
                      'host_ms']
    src = tmp_path / 'sz.c'
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "bmpow_sig.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(bmpow_sig_stats));\n' +
                   ''.join('  printf(" %%zu", offsetof(bmpow_sig_stats, %s));\n' % f for f in fields) +
                   '  return 0;\n}\n')
    exe = tmp_path / 'sz'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got[0] == ctypes.sizeof(_lib.BmpowSigStats)
    assert got[1:] == [getattr(_lib.BmpowSigStats, f).offset for f in fields]


def test_verdict_codes_match_the_header():
    text = open(HEADER).read()
    for name, code in (('INVALID', signatures.INVALID), ('SHA1', signatures.SHA1), ('SHA256', signatures.SHA256)):
        assert re.search(r'#define BMPOW_SIG_%s %d\b' % (name, code), text), name


# ------------------------------------------------------------------ DER
py_der = der_decode  # Python's own strict decode: (r, s) of a canonical DER SEQUENCE { INTEGER, INTEGER }, else None


def test_parse_against_every_fixture_signature(kats):
    seen = {True: 0, False: 0}
    sigs = [(k['name'], bytes.fromhex(k['sig']), k['der_ok']) for k in kats['cases']]
    sigs += [(o['name'], bytes.fromhex(o['parts']['sig']), None)
             for o in kats['pubkey_objects'] + kats['msg_objects'] if o['parts']]
    for name, sig, der_ok in sigs:
        got = signatures.parse(sig)
        dec = py_der(sig)
        want = dec is not None and 1 <= dec[0] < N and 1 <= dec[1] < N
        if der_ok is not None:
            assert want == der_ok, name  # the fixture's own flag and the decode here agree
        assert (got is not None) == want, name
        if want:
            assert got == (dec[0].to_bytes(32, 'big'), dec[1].to_bytes(32, 'big')), name
        seen[want] += 1
    assert seen[True] > 40 and seen[False] >= 16
    # whatever the reference accepts parses: a refusal here must be a refusal there
    for k in kats['cases']:
        assert k['der_ok'] or not k['verdict'], k['name']
    names = {k['name'] for k in kats['cases'] if not k['der_ok']}
    assert {'der_trailing_byte', 'der_zero_padded_r', 'der_long_form_length', 'der_negative_r', 'der_r_zero', 'der_s_zero',
            'der_r_plus_n', 'der_s_plus_n', 'der_s_is_n', 'der_empty', 'der_truncated'} <= names
    assert next(k for k in kats['cases'] if k['name'] == 'der_high_s')['verdict'] is True


def test_parse_leaves_the_output_alone_on_refusal(hostlib):
    rs = (ctypes.c_uint8 * 64)(*([0x5a] * 64))
    assert hostlib.bmpow_sig_parse(b'\x30\x00', 2, rs) == 0
    assert bytes(rs) == b'\x5a' * 64
    assert hostlib.bmpow_sig_parse(None, 0, rs) == 0
    one = bytes.fromhex('3006020101020101')
    assert hostlib.bmpow_sig_parse(one, len(one), rs) == 1
    assert bytes(rs) == (b'\x00' * 31 + b'\x01') * 2
    for cut in range(len(one)):
        assert hostlib.bmpow_sig_parse(one[:cut], cut, rs) == 0, cut


# ------------------------------------------------------------------ scalar_dev.h on the host
@pytest.fixture(scope='module')
def scalar_sim(tmp_path_factory):
    """tests/native/scalar_sim.cpp built with the sanitizers on: a program of its own, never loaded
    into this process."""
    d = tmp_path_factory.mktemp('scalar')
    exe = d / 'scalar_sim'
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-Werror', '-Wno-unknown-pragmas',
                           '-fsanitize=undefined,address', '-fno-sanitize-recover=all',
                           '-static-libasan', '-static-libubsan',  # the runtimes inside the program: nothing to load first
                           '-I', CSRC,
                           os.path.join(ROOT, 'tests', 'native', 'scalar_sim.cpp'), '-o', str(exe)])

    def run(ops):
        path = d / 'ops.txt'
        path.write_text(''.join(' '.join([op] + ['%064x' % v for v in vals]) + '\n' for op, *vals in ops))
        out = subprocess.check_output([str(exe), str(path)]).decode().splitlines()
        assert len(out) == len(ops)
        return out
    return run


def scalar_values():
    rng = random.Random(29)
    edge = [1, 2, N - 1, N - 2, (N + 1) // 2, (N - 1) // 2]
    edge += [2 ** k for k in range(1, 256)] + [N - 2 ** k for k in range(1, 256)]
    rand = [rng.randrange(1, N) for _ in range(1500)]
    for _ in range(300):  # sparse and dense limb patterns (the folds' carry chains)
        x = 0
        for i in range(8):
            x |= rng.choice([0, 0xFFFFFFFF, rng.getrandbits(32)]) << (32 * i)
        if 0 < x < N:
            rand.append(x)
    return edge, rand, rng


def test_scalar_products_and_inverses(scalar_sim):
    edge, rand, rng = scalar_values()
    unreduced = [2 ** 256 - 1, N, N + 1, 2 ** 256 - 2 ** 32, 2 ** 255]  # a digest is used as it comes
    ops = [('mul', a, b) for a in edge[:6] + unreduced for b in edge[:6] + unreduced]
    ops += [('mul', a, rng.choice(edge + rand + unreduced)) for a in edge + rand + unreduced]
    ops += [('inv', a) for a in edge + rand[:600]]
    ops += [('inv', a) for a in unreduced if a % N]
    # sn::add (the signing kernel's e + r d): V x V, and the operand pairs of the oracle's 'sum' family, whose
    # integer sums lie at n, at 2^256 and at 2 n - 2
    V = scalar_set()
    sums = [(c.r * c.d % N, c.e % N) for c in sign_cases() if c.family == 'sum']
    assert len(V) == 735 and len(sums) == 39
    assert {N - 1, N, N + 1, 2 ** 256 - 1, 2 ** 256, 2 ** 256 + 1, 2 * N - 2} <= {a + b for a, b in sums}
    ops += [('add', a, b) for a in V for b in V]
    ops += [('add', a, b) for a, b in sums] + [('add', b, a) for a, b in sums]
    out = scalar_sim(ops)
    bad = []
    for (op, *v), line in zip(ops, out):
        want = v[0] * v[1] % N if op == 'mul' else (v[0] + v[1]) % N if op == 'add' else pow(v[0], -1, N)
        if int(line, 16) != want:
            bad.append((op, [hex(x) for x in v], line))
    assert not bad, bad[:3]


def test_scalar_recoding(scalar_sim):
    edge, rand, _ = scalar_values()
    vals = edge + rand
    out = scalar_sim([('rec', u) for u in vals])
    for u, line in zip(vals, out):
        flip, *dig = [int(t) for t in line.split()]
        assert len(dig) == 64 and all(d % 2 and abs(d) <= 15 for d in dig), hex(u)
        assert flip == (u % 2 == 0), hex(u)
        assert sum(d * 16 ** i for i, d in enumerate(dig)) == (N - u if flip else u), hex(u)


# ------------------------------------------------------------------ the extractors
def parts_of(entry):
    p = entry['parts']
    return None if p is None else (bytes.fromhex(p['signed']), bytes.fromhex(p['sig']), bytes.fromhex(p['key']))


def test_pubkey_extractor_reproduces_the_fixture(kats):
    objs = kats['pubkey_objects']
    assert sum(o['verdict'] is True for o in objs) >= 2 and any(o['parts'] is None for o in objs)
    for o in objs:
        assert signatures.pubkey_v3_signed_parts(bytes.fromhex(o['obj'])) == parts_of(o), o['name']
    whole = bytes.fromhex(objs[0]['obj'])
    assert signatures.pubkey_v3_signed_parts(whole[:20] + b'\x04' + whole[21:]) is None  # a v4 pubkey: out of scope
    assert signatures.pubkey_v3_signed_parts(whole[:20] + b'\xfd\x00\x03' + whole[21:]) is None  # non-minimal varint
    for cut in range(0, len(whole), 7):  # never an exception, and None below the sanity length
        got = signatures.pubkey_v3_signed_parts(whole[:cut])
        assert cut >= 170 or got is None


def test_msg_extractor_reproduces_the_fixture(kats):
    objs = kats['msg_objects']
    assert sum(o['verdict'] is True for o in objs) >= 2
    assert {'msg_below_170', 'msg_sender_version_0', 'msg_sender_version_5', 'msg_sender_stream_0'} <= \
        {o['name'] for o in objs if o['parts'] is None}
    for o in objs:
        got = signatures.msg_signed_parts(bytes.fromhex(o['obj']), bytes.fromhex(o['plaintext']))
        assert got == parts_of(o), o['name']
    obj, plain = bytes.fromhex(objs[0]['obj']), bytes.fromhex(objs[0]['plaintext'])
    assert signatures.msg_signed_parts(obj[:20] + b'\x02' + obj[21:], plain) is None  # msg version 2
    for cut in range(0, len(plain), 11):
        got = signatures.msg_signed_parts(obj, plain[:cut])
        assert cut >= 170 or got is None


def test_key_forms():
    raw = bytes(range(64))
    for form in (raw, b'\x04' + raw, raw.hex(), (b'\x04' + raw).hex(), (b'\x04' + raw).hex().encode(), bytearray(raw)):
        assert signatures._key64(form) == raw
    for form in (b'', raw[:63], raw + b'xx', 'zz' * 65):
        assert signatures._key64(form) is None
