"""Object intake, the parts that need no device: the ABI table of ``include/bmpow_intake.h``, the struct
layouts, ``bmpow_intake_header`` / ``bmpow_intake_status`` (host-only entry points; the library loads
without a GPU) against the reference-made fixture ``tests/golden/intake_kats.json``
(tests/golden/make_intake_golden.py) and a Python restatement, and the rule by which the kernel reads the
full object's padded message out of the payload pool."""
import ctypes
import hashlib
import os
import random
import re
import struct
import subprocess

import pytest

from pybitmessage_amd import _lib, intake
from tests.conftest import ROOT
from tests.golden.make_intake_golden import regen, varint

HEADER = os.path.join(ROOT, 'include', 'bmpow_intake.h')
MAX_TTL = 28 * 24 * 60 * 60 + 10800


@pytest.fixture(scope='module')
def kats(golden):
    return golden('intake_kats.json')


@pytest.fixture(scope='module')
def hostlib():
    return _lib.load()


def declared_symbols():
    text = open(HEADER).read()
    return sorted(set(re.findall(r'BMPOW_API\s+[\w\s\*]+?\b(\w+)\s*\(', text)))


def test_every_declared_symbol_is_exported_and_bound(hostlib):
    syms = declared_symbols()
    assert 'bmpow_intake_batch' in syms and 'bmpow_inventory_hashes' in syms and len(syms) == 6
    assert syms == sorted(name for name, _, _ in _lib.INTAKE_SIGNATURES)
    raw = ctypes.CDLL(_lib.lib_path())
    for name, res, args in _lib.INTAKE_SIGNATURES:
        assert hasattr(raw, name), name
        fn = getattr(hostlib, name)
        assert fn.restype == res and list(fn.argtypes) == args, name
    # the other headers' tables keep their own sets
    assert not set(syms) & set(name for name, _, _ in _lib.SIGNATURES)
    assert not set(syms) & set(name for name, _, _ in _lib.ECIES_SIGNATURES)


@pytest.mark.parametrize('ctype,cls', [('bmpow_intake_stats', _lib.BmpowIntakeStats),
                                       ('bmpow_intake_rec', _lib.BmpowIntakeRec),
                                       ('bmpow_intake_params', _lib.BmpowIntakeParams)])
def test_structs_match_the_header(tmp_path, ctype, cls):
    fields = [f for f, _ in cls._fields_]
    src = tmp_path / 'sz.c'
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "bmpow_intake.h"\nint main(void) {\n'
                   '  printf("%%zu", sizeof(%s));\n' % ctype +
                   ''.join('  printf(" %%zu", offsetof(%s, %s));\n' % (ctype, f) for f in fields) +
                   '  return 0;\n}\n')
    exe = tmp_path / 'sz'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got[0] == ctypes.sizeof(cls)
    assert got[1:] == [getattr(cls, f).offset for f in fields]
    if cls is _lib.BmpowIntakeRec:  # the numpy view check_objects returns
        assert intake.REC_DTYPE.itemsize == got[0]
        assert [intake.REC_DTYPE.fields[f][1] for f in fields] == got[1:]


def test_status_constants_match_the_header_and_the_fixture(kats):
    text = open(HEADER).read()
    for code, name in intake.STATUS_NAMES.items():
        assert re.search(r'#define BMPOW_INTAKE_%s %d\b' % (name, code), text), name
        assert getattr(intake, name) == code and kats['status_names'][code] == name
    assert '#define BMPOW_INTAKE_MAX_TTL %d ' % MAX_TTL in text


def rec_fields(rec):
    return {'nonce': rec.nonce, 'expires': rec.expires, 'type': rec.object_type, 'version': rec.version,
            'stream': rec.stream, 'payloadOffset': rec.payload_offset}


def test_header_and_status_reproduce_the_fixture(kats):
    seen = set()
    for k in kats['kats']:
        obj = regen(k)
        rec = intake.header(obj)
        if k['fields'] is None:
            assert rec is None, k['name']
            assert all(c['status'] == intake.MALFORMED for c in k['checks']), k['name']
            seen.add(intake.MALFORMED)
            continue
        assert rec is not None, k['name']
        want = {f: v for f, v in k['fields'].items() if f not in ('inv', 'tag')}
        assert rec_fields(rec) == want, k['name']
        assert bytes(rec.inv) == bytes(32) and rec.pow == 0 and rec.status == 0
        assert obj[rec.payload_offset:rec.payload_offset + 32].hex() == k['fields']['tag'], k['name']
        assert hashlib.sha512(hashlib.sha512(obj).digest()).digest()[:32].hex() == k['fields']['inv']
        for c in k['checks']:
            got = intake.status_of(rec, len(obj), c['pow_ok'], c['now'], c['streams'])
            assert got == c['status'], (k['name'], c)
            seen.add(got)
    assert seen == set(range(9))  # every status has a case
    # a record the header walk did not fill
    assert intake.status_of(_lib.BmpowIntakeRec(), 100, True, kats['now']) == intake.MALFORMED


def py_varint(data):
    """addresses.decodeVarint restated: (value, size) or None where it raises."""
    if not data:
        return 0, 0
    f = data[0]
    if f < 253:
        return f, 1
    size, least = {253: (3, 253), 254: (5, 65536), 255: (9, 4294967296)}[f]
    if len(data) < size:
        return None
    v = int.from_bytes(data[1:size], 'big')
    return None if v < least else (v, size)


def py_header(obj):
    if len(obj) < 20:
        return None
    nonce, expires, otype = struct.unpack('>QQI', obj[:20])
    a = py_varint(obj[20:])
    if a is None:
        return None
    b = py_varint(obj[20 + a[1]:])
    if b is None:
        return None
    return {'nonce': nonce, 'expires': expires, 'type': otype, 'version': a[0], 'stream': b[0],
            'payloadOffset': 20 + a[1] + b[1]}


def py_status(h, length, pow_ok, now, streams):
    if length - h['payloadOffset'] > 2 ** 18:
        return intake.TOO_LARGE
    if not pow_ok:
        return intake.INSUFFICIENT_POW
    if h['expires'] - now > MAX_TTL:
        return intake.EXPIRED_FUTURE
    if h['expires'] - now < -3600:
        return intake.EXPIRED_PAST
    if h['stream'] < 1 or h['stream'] > 2 ** 63 - 1:
        return intake.INVALID_STREAM
    if h['stream'] not in streams:
        return intake.UNWANTED_STREAM
    t = h['type']
    if (t == 0 and length < 42) or (t == 1 and (length < 146 or length > 440)) or \
            (t == 3 and (length < 180 or h['version'] < 2)):
        return intake.INVALID_FOR_TYPE
    return intake.OK


def test_random_headers_agree_with_the_restatement():
    rng = random.Random(20250302)
    now = 1700000000
    edge_values = [0, 1, 2, 252, 253, 254, 255, 65535, 65536, 2 ** 32 - 1, 2 ** 32, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1]
    statuses = set()
    decoded = 0
    for _ in range(4000):
        def some_varint():
            r = rng.random()
            if r < 0.6:
                return varint(rng.choice(edge_values) if rng.random() < 0.5 else rng.randrange(0, 300))
            if r < 0.8:  # any prefix byte over any value: often not minimal
                return bytes([rng.choice([253, 254, 255])]) + rng.randbytes(8)
            return rng.randbytes(rng.randrange(0, 4))
        expires = now + rng.choice([0, 300, MAX_TTL, MAX_TTL + 1, -3600, -3601, rng.randrange(-10 ** 7, 10 ** 7),
                                    2 ** 63, -now])
        obj = (rng.randbytes(8) + struct.pack('>QI', expires, rng.choice([0, 1, 2, 3, 4, 0x746f72, 2 ** 32 - 1])) +
               some_varint() + some_varint() + rng.randbytes(rng.choice([0, 1, 20, 130, 420])))
        obj = obj[:rng.choice([len(obj), len(obj), len(obj), rng.randrange(0, len(obj) + 1)])]
        want = py_header(obj)
        rec = intake.header(obj)
        if want is None:
            assert rec is None, obj.hex()
            continue
        decoded += 1
        assert rec is not None and rec_fields(rec) == want, obj.hex()
        streams = rng.choice([(1,), (), (1, 2), (want['stream'],), (2 ** 63 - 1, 5)])
        length = rng.choice([len(obj), len(obj), 41, 42, 145, 146, 440, 441, 179, 180, want['payloadOffset'] + 2 ** 18,
                             want['payloadOffset'] + 2 ** 18 + 1])
        pow_ok = rng.random() < 0.85
        got = intake.status_of(rec, length, pow_ok, now, streams)
        assert got == py_status(want, length, pow_ok, now, streams), (obj.hex(), length, streams)
        statuses.add(got)
    assert decoded > 1500 and statuses == set(range(9)) - {intake.MALFORMED}


def pad(msg):
    bits = struct.pack('>QQ', len(msg) >> 61, (len(msg) << 3) & (2 ** 64 - 1))
    return msg + b'\x80' + bytes(-(len(msg) + 17) % 128) + bits


def test_the_pool_word_rule_gives_the_padded_object_for_every_length():
    """bmpow_intake.hip reads the full object's SHA-512 message out of the pool of padded object[8:]:
    word k is the nonce (k = 0), 8 L (k = 16 nblk2 - 1), 0 (k >= 16 nblk), else pool word k - 1.  Direct
    padding of the object gives the same words, for every L across both block edges of either count; and
    so does the kernel's form of the rule, block by block with the previous block's last word carried."""
    rng = random.Random(7)
    for L in list(range(8, 442)) + [1000, 1015, 1016, 1017, 262152]:
        obj = rng.randbytes(L)
        pool = pad(obj[8:])
        nblk = len(pool) // 128
        nblk2 = (L + 17 + 127) // 128
        assert nblk2 in (nblk, nblk + 1)
        P = struct.unpack('>%dQ' % (16 * nblk), pool)
        nonce = struct.unpack('>Q', obj[:8])[0]

        def word(k):
            if k == 0:
                return nonce
            if k == 16 * nblk2 - 1:
                return 8 * L
            if k >= 16 * nblk:
                return 0
            return P[k - 1]
        direct = pad(obj)
        assert len(direct) == 128 * nblk2
        want = struct.unpack('>%dQ' % (16 * nblk2), direct)
        assert tuple(word(k) for k in range(16 * nblk2)) == want, L
        got, carry = [], 0
        for c in range(nblk2):
            lb = c if c < nblk else nblk - 1
            w = list(P[16 * lb:16 * lb + 16])
            w15 = w[15]
            w = [nonce if c == 0 else carry] + w[:15]
            carry = w15
            if c >= nblk:
                w = [0] * 16
            if c == nblk2 - 1:
                w[15] = 8 * L
            got += w
        assert tuple(got) == want, L


def test_the_c_list_walk_hands_over_the_objects_where_they_lie():
    """_bmpow_fast.intake_list: pointers into the bytes objects themselves, their lengths, and the caller's
    params / records addresses, passed to the entry point whose address it is given."""
    from pybitmessage_amd import verify
    fast = verify._fast()
    assert fast is not None and hasattr(fast, 'intake_list')
    seen = {}
    proto = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p),
                             ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p, ctypes.c_void_p)

    def entry(n, ptrs, lens, prm, out):
        seen.update(n=n, ptrs=[ptrs[i] for i in range(n)], data=[ctypes.string_at(ptrs[i], lens[i]) for i in range(n)],
                    prm=prm, out=out)
        return -3
    cb = proto(entry)
    objs = [b'', b'abc', bytes(range(200)), b'x' * 5000]
    assert fast.intake_list(ctypes.cast(cb, ctypes.c_void_p).value, objs, 1234, 5678) == -3
    assert seen['n'] == 4 and seen['data'] == objs and (seen['prm'], seen['out']) == (1234, 5678)
    assert seen['ptrs'] == verify._pointers(objs).tolist()
    with pytest.raises(TypeError):
        fast.intake_list(ctypes.cast(cb, ctypes.c_void_p).value, [b'ok', bytearray(3)], 0, 0)
    assert fast.intake_list(ctypes.cast(cb, ctypes.c_void_p).value, [], 0, 0) == -3 and seen['n'] == 0
