"""ECIES trial decryption, the parts that need no device: the ABI table of ``include/bmpow_ecies.h``,
``bmpow_ecies_parse`` and ``bmpow_ecies_decrypt`` (host-only entry points; the library loads without a
GPU) against the reference-made fixture ``tests/golden/ecies_kats.json``
(tests/golden/make_ecies_golden.py), and the header walk ``ecies.msg_payload``."""
import ctypes
import hashlib
import os
import re
import struct

import pytest

from pybitmessage_amd import _lib, ecies
from tests.conftest import ROOT

HEADER = os.path.join(ROOT, 'include', 'bmpow_ecies.h')
P = 2 ** 256 - 2 ** 32 - 977


@pytest.fixture(scope='module')
def kats(golden):
    return golden('ecies_kats.json')


@pytest.fixture(scope='module')
def hostlib():
    return _lib.load()


def declared_symbols():
    text = open(HEADER).read()
    return sorted(set(re.findall(r'BMPOW_API\s+[\w\s\*]+?\b(\w+)\s*\(', text)))


def test_every_declared_symbol_is_exported_and_bound(hostlib):
    syms = declared_symbols()
    assert 'bmpow_ecies_match' in syms and 'bmpow_ecdh' in syms and len(syms) == 6
    assert syms == sorted(name for name, _, _ in _lib.ECIES_SIGNATURES)
    raw = ctypes.CDLL(_lib.lib_path())
    for name, res, args in _lib.ECIES_SIGNATURES:
        assert hasattr(raw, name), name
        fn = getattr(hostlib, name)
        assert fn.restype == res and list(fn.argtypes) == args, name
    # the first header and table keep their own set
    assert not set(syms) & set(name for name, _, _ in _lib.SIGNATURES)


def test_stats_struct_matches_the_header(tmp_path):
    import subprocess
    fields = [f for f, _ in _lib.BmpowEciesStats._fields_]
    src = tmp_path / 'sz.c'
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "bmpow_ecies.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(bmpow_ecies_stats));\n' +
                   ''.join('  printf(" %%zu", offsetof(bmpow_ecies_stats, %s));\n' % f for f in fields) +
                   '  return 0;\n}\n')
    exe = tmp_path / 'sz'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got[0] == ctypes.sizeof(_lib.BmpowEciesStats)
    assert got[1:] == [getattr(_lib.BmpowEciesStats, f).offset for f in fields]


def py_parse(blob):
    """The structural rule, restated: the key header lies inside data[:-32]."""
    if len(blob) < 20:
        return None
    xl = struct.unpack('!H', blob[18:20])[0]
    if len(blob) < 22 + xl:
        return None
    yl = struct.unpack('!H', blob[20 + xl:22 + xl])[0]
    off = 22 + xl + yl
    if off + 32 > len(blob):
        return None
    x = int.from_bytes(blob[20:20 + xl], 'big') % P
    y = int.from_bytes(blob[22 + xl:off], 'big') % P
    return x.to_bytes(32, 'big'), y.to_bytes(32, 'big'), off


def test_parse_agrees_with_the_fixture_verdicts(kats):
    for v in kats['verdict_kats']:
        blob = bytes.fromhex(v['blob'])
        got = ecies.parse(blob)
        assert (got is not None) == v['wellformed'], v['name']
        assert got == py_parse(blob), v['name']
        if not v['wellformed']:
            assert v['outcome'] != 'decrypted' and not v['match'], v['name']
    for m in kats['msg_kats']:
        blob = bytes.fromhex(m['blob'])
        assert ecies.parse(blob) == py_parse(blob) != None  # noqa: E711
    by_name = {v['name']: v for v in kats['verdict_kats']}
    pt = kats['verdict_point']
    # lenient encodings of one point all parse to it; the reference decrypts each of them
    for name in ('plain', 'curve_zero', 'curve_other', 'x_33_leading_zero', 'y_34_leading_zeros', 'x_plus_p',
                 'y_plus_p'):
        assert by_name[name]['outcome'] == 'decrypted', name
        x, y, _ = ecies.parse(bytes.fromhex(by_name[name]['blob']))
        assert (x.hex(), y.hex()) == (pt['x'], pt['y']), name
    x, y, _ = ecies.parse(bytes.fromhex(by_name['neg_y']['blob']))
    assert x.hex() == pt['x'] and int.from_bytes(y, 'big') == P - int(pt['y'], 16)


def test_parse_reduces_long_coordinates():
    """Coordinates are integers of any length (BN_bin2bn): hundreds of bytes reduce mod p."""
    for xv, yv in [(P - 1, P + 5), (2 ** 2000 + 12345, 3 ** 700), (0, 2 ** 256 - 1), (2 ** 256, 2 ** 512 - 1)]:
        xb = xv.to_bytes((xv.bit_length() + 7) // 8 + 3, 'big')
        yb = yv.to_bytes((yv.bit_length() + 7) // 8, 'big')
        blob = (b'\x00' * 16 + struct.pack('!HH', 714, len(xb)) + xb + struct.pack('!H', len(yb)) + yb + b'c' * 16 +
                b'm' * 32)
        x, y, off = ecies.parse(blob)
        assert int.from_bytes(x, 'big') == xv % P and int.from_bytes(y, 'big') == yv % P
        assert off == len(blob) - 48


def key_e_for(shared_x_hex):
    return hashlib.sha512(bytes.fromhex(shared_x_hex)).digest()[:32]


def test_decrypt_reproduces_the_fixture_plaintexts(kats):
    key_e = key_e_for(kats['verdict_shared_x'])
    seen_ok = seen_bad = 0
    for v in kats['verdict_kats']:
        blob = bytes.fromhex(v['blob'])
        if not v['match']:
            continue
        got = ecies.decrypt(blob, key_e)
        if v['outcome'] == 'decrypted':
            assert got == bytes.fromhex(v['plaintext']), v['name']
            seen_ok += 1
        else:  # a valid MAC, and the reference raised in the cipher
            assert got is None, v['name']
            seen_bad += 1
    assert seen_ok >= 8 and seen_bad >= 4
    # a wrong key: the padding check refuses nearly every such plaintext, and never returns the original
    plain = next(v for v in kats['verdict_kats'] if v['name'] == 'plain')
    assert ecies.decrypt(bytes.fromhex(plain['blob']), b'\x01' * 32) != bytes.fromhex(plain['plaintext'])
    # a malformed payload and a short output buffer are argument errors
    lib = _lib.host()
    out = ctypes.create_string_buffer(64)
    u8 = ctypes.POINTER(ctypes.c_uint8)
    assert lib.bmpow_ecies_decrypt(b'short', 5, key_e, ctypes.cast(out, u8), 64) == _lib.E_ARG
    blob = bytes.fromhex(plain['blob'])
    assert lib.bmpow_ecies_decrypt(blob, len(blob), key_e, ctypes.cast(out, u8), 16) == _lib.E_ARG


def test_decrypt_msg_kats_from_the_ecdh_restatement(kats):
    """msg_kats through the pure-Python ECDH below: key_e = SHA512(x(k R))[:32] decrypts every blob."""
    for m in kats['msg_kats']:
        blob = bytes.fromhex(m['blob'])
        x, y, _ = ecies.parse(blob)
        k = int(kats['recipient_keys'][m['recipient']], 16)
        sx = ec_mul(k, (int.from_bytes(x, 'big'), int.from_bytes(y, 'big')))[0]
        assert ecies.decrypt(blob, hashlib.sha512(sx.to_bytes(32, 'big')).digest()[:32]) == bytes.fromhex(m['plaintext'])


def ec_add(a, b):
    if a is None:
        return b
    if b is None:
        return a
    if a[0] == b[0]:
        if (a[1] + b[1]) % P == 0:
            return None
        lam = 3 * a[0] * a[0] * pow(2 * a[1], -1, P) % P
    else:
        lam = (b[1] - a[1]) * pow(b[0] - a[0], -1, P) % P
    x = (lam * lam - a[0] - b[0]) % P
    return x, (lam * (a[0] - x) - a[1]) % P


def ec_mul(k, pt):
    acc = None
    while k:
        if k & 1:
            acc = ec_add(acc, pt)
        pt = ec_add(pt, pt)
        k >>= 1
    return acc


def test_ecdh_kats_agree_with_the_restatement(kats):
    """The fixture's shared x values are x(k R) (pins the restatement the GPU tests build payloads with)."""
    e = kats['ecdh_kats']
    assert len(e['points']) == 3 and len(e['points'][2]['x']) == 62
    for p, row in zip(e['points'], e['shared_x']):
        pt = (int(p['x'], 16), int(p['y'], 16))
        for k, sx in list(zip(e['keys'], row))[::7]:
            assert ec_mul(int(k, 16), pt)[0] == int(sx, 16)


def obj_with(version, stream, payload):
    return b'\x00' * 8 + b'\x11' * 8 + b'\x00\x00\x00\x02' + version + stream + payload


def test_msg_payload_header_walk():
    pay = b'encrypted part'
    assert ecies.msg_payload(obj_with(b'\x01', b'\x01', pay)) == pay
    assert ecies.msg_payload(obj_with(b'\x01', b'\xfd\x01\x00', pay)) == pay                     # 3-byte stream
    assert ecies.msg_payload(obj_with(b'\x01', b'\xff' + (2 ** 32).to_bytes(8, 'big'), pay)) == pay  # 9-byte stream
    assert ecies.msg_payload(obj_with(b'\x01', b'\xfe\x00\x01\x00\x00', pay)) == pay             # 5-byte stream
    assert ecies.msg_payload(obj_with(b'\x02', b'\x01', pay)) is None                            # version 2
    assert ecies.msg_payload(obj_with(b'\xfd\x01\x00', b'\x01', pay)) is None                    # version 256
    assert ecies.msg_payload(obj_with(b'\xfd\x00\x01', b'\x01', pay)) is None                    # 1, not minimal
    assert ecies.msg_payload(b'\x00' * 20) is None                                               # nothing after the header
    assert ecies.msg_payload(obj_with(b'\x01', b'', b'')) == b''                                 # empty stream varint: (0, 0)
    assert ecies.msg_payload(obj_with(b'\x01', b'\xfd\x01', b'')) is None                        # truncated varint
