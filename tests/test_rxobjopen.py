"""The one-call opening of received broadcasts and pubkeys without a GPU (include/bmpow_rxobjopen.h): the host-only
table and row code as a stand-alone program under AddressSanitizer + UBSan (tests/native/rxobjopen_sim.cpp); the
host's plan of an object (``bmpow_rx_sealed_object_plan``) against ``signatures.broadcast_header``,
``signatures.pubkey_v4_header`` and ``ecies.parse`` on the fixture's objects and on refusals; the declared symbols
and the stats struct; and the argument checks that return before any device is touched."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from pybitmessage_amd import _lib, ecies, receive, signatures
from tests.conftest import ROOT, load_golden

HEADER = os.path.join(ROOT, 'include', 'bmpow_rxobjopen.h')
CSRC = os.path.join(ROOT, 'pybitmessage_amd', 'csrc')
BROADCAST, PUBKEY_V4, PUBKEY = receive.KIND_BROADCAST, receive.KIND_PUBKEY_V4, receive.KIND_PUBKEY
ORDER = bytes.fromhex('fffffffffffffffffffffffffffffffebaaedce6af48a03bbfd25e8cd0364141')


@pytest.fixture(scope='module')
def kats():
    return load_golden('rxobj_kats.json')


@pytest.fixture(scope='module')
def hostlib():
    return _lib.load()


def test_every_declared_symbol_is_exported_and_bound(hostlib):
    text = open(HEADER).read()
    syms = sorted(set(re.findall(r'BMPOW_API\s+[\w\s\*]+?\b(\w+)\s*\(', text)))
    assert syms == ['bmpow_rx_sealed_obj_get_stats', 'bmpow_rx_sealed_obj_reset_stats', 'bmpow_rx_sealed_object_plan',
                    'bmpow_rx_sealed_objects']
    assert syms == sorted(name for name, _, _ in _lib.RXOBJOPEN_SIGNATURES)
    raw = ctypes.CDLL(_lib.lib_path())
    for name, res, args in _lib.RXOBJOPEN_SIGNATURES:
        assert hasattr(raw, name), name
        fn = getattr(hostlib, name)
        assert fn.restype == res and list(fn.argtypes) == args, name
    for other in (_lib.RX_SIGNATURES, _lib.RXOBJ_SIGNATURES, _lib.ECIES_SIGNATURES, _lib.RXOPEN_SIGNATURES):
        assert not set(syms) & set(name for name, _, _ in other)
    # the header says what becomes of a tag that is there twice
    assert 'FIRST entry wins' in text
    for fn in ('open_sealed_objects', 'open_sealed_broadcasts', 'open_sealed_pubkeys', 'sealed_object_plan', 'sealed_obj_stats',
               'sealed_obj_reset_stats'):
        assert callable(getattr(receive, fn)), fn


def test_structs_match_the_header():
    text = open(HEADER).read()
    body = re.search(r'typedef struct bmpow_rx_sealed_obj_stats \{(.*?)\} bmpow_rx_sealed_obj_stats;', text, re.S).group(1)
    declared = re.findall(r'^\s*(uint64_t|double)\s+(\w+);', body, re.M)
    ctype = {'uint64_t': ctypes.c_uint64, 'double': ctypes.c_double}
    assert [(n, ctype[t]) for t, n in declared] == list(_lib.BmpowRxSealedObjStats._fields_)
    names = [n for _, n in declared]
    for want in ('calls', 'rows', 'matched', 'sets', 'launches', 'rx_launches', 'tagged_tries', 'trial_tries', 'match_ms',
                 'open_ms', 'walk_ms', 'hash_ms', 'scalar_ms', 'curve_ms', 'ident_ms', 'finish_ms', 'bytes_up', 'bytes_down',
                 'host_ms'):
        assert want in names, want
    body = re.search(r'typedef struct bmpow_rx_obj_tables \{(.*?)\} bmpow_rx_obj_tables;', text, re.S).group(1)
    declared = re.findall(r'^\s*(size_t|const uint8_t \*|const uint64_t \*)\s*(\w+);', body, re.M)
    assert [n for _, n in declared] == [n for n, _ in _lib.BmpowRxObjTables._fields_]
    for (t, n), (_, c) in zip(declared, _lib.BmpowRxObjTables._fields_):
        assert (c is ctypes.c_size_t) == (t == 'size_t'), n


# ------------------------------------------------------------------ the table and row code on the host
def test_table_and_row_code_under_sanitizers(tmp_path):
    """A program of its own (its own main, the sanitizer runtimes linked in), never loaded into this process: the
    tag table with 0, 1, repeated and colliding entries; the routing of heads of every kind around every floor; the
    opening row code over a pool of object slots at every ciphertext alignment, against libcrypto."""
    exe = tmp_path / 'rxobjopen_sim'
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-Werror', '-Wno-unknown-pragmas',
                           '-fsanitize=undefined,address', '-fno-sanitize-recover=all', '-static-libasan',
                           '-static-libubsan', '-I', CSRC, os.path.join(ROOT, 'tests', 'native', 'rxobjopen_sim.cpp'),
                           '-o', str(exe), '-lcrypto'])
    env = dict(os.environ)
    env['ASAN_OPTIONS'] = 'halt_on_error=1 detect_leaks=1'
    env['UBSAN_OPTIONS'] = 'halt_on_error=1 print_stacktrace=1'
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    assert 'all rxobjopen checks passed' in r.stderr
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr


# ------------------------------------------------------------------ the plan of one object
def test_plan_agrees_with_the_python_parsers_on_every_fixture_object(kats):
    seen = set()
    for e in kats['broadcasts']:
        obj = bytes.fromhex(e['obj'])
        ok, reason, routed, payload_off, tag_off, body_off, clen = receive.sealed_object_plan(BROADCAST, obj)
        head = signatures.broadcast_header(obj)  # (version, stream, tag, payloadOffset)
        seen.add((BROADCAST, reason))
        assert routed == BROADCAST
        if head is None:
            assert (ok, reason, payload_off, tag_off, body_off, clen) == (False, receive.PLAN_HEAD, 0, 0, 0, 0), e['name']
            assert e['line'] in (760, 'varint')
            continue
        assert payload_off == head[3] and obj[tag_off:payload_off] == (head[2] or b''), e['name']
        parsed = ecies.parse(obj[payload_off:])
        assert parsed is not None and (ok, reason) == (True, receive.PLAN_OK), e['name']
        assert body_off == parsed[2] and clen == len(obj) - payload_off - 32 - body_off and clen % 16 == 0 and clen > 0
        if e['plaintext'] is not None:
            assert clen == 16 * (len(e['plaintext']) // 2 // 16 + 1), e['name']
    for section in ('pubkeys_v4', 'pubkeys'):
        for e in kats[section]:
            obj = bytes.fromhex(e['obj'])
            ok, reason, routed, payload_off, tag_off, body_off, clen = receive.sealed_object_plan(PUBKEY, obj)
            walked, _ = receive.walk_object(PUBKEY, obj)
            seen.add((routed, reason))
            if int(walked.status[0]) != receive.OBJ_NEEDS_DECRYPTION:
                assert routed == PUBKEY and not ok and (body_off, clen) == (0, 0), e['name']
                assert reason == (receive.PLAN_HEAD if walked.recs[0]['payload_off'] == 0 else receive.PLAN_CLEAR), e['name']
                assert payload_off == tag_off == int(walked.recs[0]['payload_off'])
                continue
            head = signatures.pubkey_v4_header(obj)  # (addressVersion, stream, tag, payloadOffset)
            assert routed == PUBKEY_V4 and head is not None and payload_off == head[3] and obj[tag_off:payload_off] == head[2], e['name']
            if len(obj) < 350:
                assert (ok, reason, body_off, clen) == (False, receive.PLAN_V4_SHORT, 0, 0), e['name']
                continue
            parsed = ecies.parse(obj[payload_off:])
            assert parsed is not None and body_off == parsed[2] and clen == len(obj) - payload_off - 32 - body_off, e['name']
            assert (ok, reason) == ((True, receive.PLAN_OK) if clen and clen % 16 == 0 else (False, receive.PLAN_CIPHER)), e['name']
    assert seen == {(BROADCAST, receive.PLAN_OK), (BROADCAST, receive.PLAN_HEAD), (PUBKEY, receive.PLAN_HEAD),
                    (PUBKEY, receive.PLAN_CLEAR), (PUBKEY_V4, receive.PLAN_OK), (PUBKEY_V4, receive.PLAN_V4_SHORT),
                    (PUBKEY_V4, receive.PLAN_CIPHER)}


def _head(kind, version, stream=b'\x01', tag=True):
    out = bytes(range(16)) + (b'\x00\x00\x00\x03' if kind == BROADCAST else b'\x00\x00\x00\x01') + version + stream
    return out + (b'\x77' * 32 if tag else b'')


def _msg_head():
    return bytes(range(16)) + b'\x00\x00\x00\x02\x01\x01'


def _payload(clen, xl=32, yl=32):
    return (bytes(16) + b'\x02\xca' + xl.to_bytes(2, 'big') + b'\x11' * xl + yl.to_bytes(2, 'big') + b'\x22' * yl +
            b'\x33' * clen + b'\x44' * 32)


def test_plan_refusals_agree_with_the_msg_plan():
    """The same payloads behind a msg's head and behind a v4 / v5 broadcast's and a v4 pubkey's: the reasons are
    those of ``sealed_plan``, the offsets moved by the head's length."""
    heads = ((BROADCAST, _head(BROADCAST, b'\x04', tag=False), BROADCAST), (BROADCAST, _head(BROADCAST, b'\x05'), BROADCAST),
             (PUBKEY, _head(PUBKEY, b'\x04'), PUBKEY_V4))
    whole = _payload(0)
    payloads = [_payload(48), _payload(16, 31, 30), _payload(16, 0, 0)]
    payloads += [whole[:keep] for keep in list(range(0, 20)) + [21, 52, 53, 54, 85, 86, 117]]  # cut inside the header, the point
    payloads += [_payload(clen) for clen in (0, 15, 17, 8)]
    for payload in payloads:
        want = receive.sealed_plan(_msg_head() + payload)
        for kind, head, routed in heads:
            obj = head + payload
            if routed == PUBKEY_V4:
                obj += bytes(max(0, 350 - len(obj)))  # :411's floor; the payload grows, so only whole ones compare
                if len(obj) != len(head) + len(payload):
                    continue
            got = receive.sealed_object_plan(kind, obj)
            assert got[:3] == (want[0], want[1], routed), (kind, len(payload))
            assert got[3] == len(head) and got[4] == len(head) - (32 if len(head) > 30 else 0)
            assert got[5:] == want[3:], (kind, len(payload))
    reasons = {receive.sealed_plan(_msg_head() + p)[1] for p in payloads}
    assert reasons == {receive.PLAN_OK, receive.PLAN_PAYLOAD, receive.PLAN_CIPHER}
    # a v4 pubkey of 350 bytes with each kind of ciphertext length
    for clen, reason in ((350 - 54 - 86 - 32, receive.PLAN_CIPHER), (192, receive.PLAN_OK), (0, receive.PLAN_V4_SHORT)):
        obj = _head(PUBKEY, b'\x04') + _payload(clen)
        assert receive.sealed_object_plan(PUBKEY, obj)[:3] == (reason == receive.PLAN_OK, reason, PUBKEY_V4), clen
    # heads that refuse: a varint that does not decode, broadcast versions 3 and 6, nothing at all
    for version in (b'\xfd\x00\x04', b'\x03', b'\x06', b'\xfe\x00\x00\x00\x05'):
        assert receive.sealed_object_plan(BROADCAST, _head(BROADCAST, version) + _payload(48)) == \
            (False, receive.PLAN_HEAD, BROADCAST, 0, 0, 0, 0)
    for stream in (b'\xfd\x00\x10', b'\xfd\x01', b'\xff' + bytes(5)):
        assert receive.sealed_object_plan(BROADCAST, _head(BROADCAST, b'\x05', stream, tag=False)) == \
            (False, receive.PLAN_HEAD, BROADCAST, 0, 0, 0, 0)
        assert receive.sealed_object_plan(PUBKEY, _head(PUBKEY, b'\x04', stream, tag=False))[:4] == (False, receive.PLAN_HEAD, PUBKEY, 0)
    assert receive.sealed_object_plan(PUBKEY, _head(PUBKEY, b'\xfd\x00\x04') + _payload(48))[:4] == (False, receive.PLAN_HEAD, PUBKEY, 0)
    assert receive.sealed_object_plan(BROADCAST, b'')[:2] == (False, receive.PLAN_HEAD)
    # a v5 broadcast whose tag the object's end cuts: nobody's, no payload
    cut = _head(BROADCAST, b'\x05')[:40]
    assert receive.sealed_object_plan(BROADCAST, cut) == (False, receive.PLAN_PAYLOAD, BROADCAST, 40, 22, 0, 0)
    # clear pubkeys: no key is involved
    for version in (b'\x00', b'\x02', b'\x03', b'\x05'):
        assert receive.sealed_object_plan(PUBKEY, _head(PUBKEY, version, tag=False) + bytes(200))[:4] == \
            (False, receive.PLAN_CLEAR, PUBKEY, 22)


def test_plan_argument_errors(hostlib):
    z = ctypes.c_size_t(0)
    r = ctypes.c_int(0)
    args = [ctypes.byref(r), ctypes.byref(z), ctypes.byref(z), ctypes.byref(z), ctypes.byref(z), ctypes.byref(r)]
    assert hostlib.bmpow_rx_sealed_object_plan(0, b'x', 1, *args) == 0
    for k in range(6):
        assert hostlib.bmpow_rx_sealed_object_plan(0, b'x', 1, *(args[:k] + [None] + args[k + 1:])) == _lib.E_ARG
    assert hostlib.bmpow_rx_sealed_object_plan(0, None, 1, *args) == _lib.E_ARG
    assert hostlib.bmpow_rx_sealed_object_plan(PUBKEY_V4, b'x', 1, *args) == _lib.E_ARG  # the call routes; it is not given
    assert hostlib.bmpow_rx_sealed_object_plan(7, b'x', 1, *args) == _lib.E_ARG
    assert b'kind' in hostlib.bmpow_last_error()


# ------------------------------------------------------------------ arguments, before any device
def test_argument_errors_before_any_device(hostlib, kats):
    v5 = _head(BROADCAST, b'\x05') + _payload(48)
    refused = _head(BROADCAST, b'\x03') + _payload(48)
    key, tag, ripe = bytes(31) + b'\x01', b'\x77' * 32, bytes(20)
    with pytest.raises(ValueError):
        receive.SealedTables(tags=([tag], [bytes(33)]))                 # a key longer than 32 bytes
    with pytest.raises(ValueError):
        receive.SealedTables(tags=([tag[:31]], [key]))                  # a tag is 32 bytes
    with pytest.raises(ValueError):
        receive.SealedTables(trial=([bytes(19)], [key]))                # a ripe is 20 bytes
    with pytest.raises(ValueError):
        receive.SealedTables(trial=([ripe, ripe], [key]))               # one ripe per key
    with pytest.raises(ValueError):
        receive.open_sealed_tables([BROADCAST], [v5, v5], receive.SealedTables())

    p64 = ctypes.POINTER(ctypes.c_uint64)

    def call(objs, kinds=None, tables=None, n=None, cap=None, recs_at='own', with_tables=True):
        n = len(objs) if n is None else n
        kinds = bytes([BROADCAST] * len(objs)) if kinds is None else kinds
        recs = np.zeros(max(len(objs), 1), dtype=receive.OBJ_REC)
        match = np.zeros(max(len(objs), 1), dtype=np.int32)
        off, ln = np.zeros(max(len(objs), 1), dtype=np.uint64), np.zeros(max(len(objs), 1), dtype=np.uint64)
        lens = np.array([len(o) for o in objs] or [0], dtype=np.uint64)
        arena = np.zeros(max(int(lens.sum()), 1), dtype=np.uint8)
        ptrs = (ctypes.c_char_p * max(len(objs), 1))(*objs)
        t, keep = (tables or receive.SealedTables()).struct()
        rc = hostlib.bmpow_rx_sealed_objects(n, kinds, ctypes.cast(ptrs, ctypes.c_void_p), lens.ctypes.data_as(p64),
                                             ctypes.byref(t) if with_tables else None,
                                             recs.ctypes.data if recs_at == 'own' else recs_at, match.ctypes.data,
                                             arena.ctypes.data, int(lens.sum()) if cap is None else cap, off.ctypes.data,
                                             ln.ctypes.data)
        del keep
        return rc, recs, match, ln

    assert call([v5], n=0)[0] == 0
    assert call([v5], recs_at=None)[0] == _lib.E_ARG
    assert call([v5], with_tables=False)[0] == _lib.E_ARG
    assert call([v5], cap=len(v5) - 1)[0] == _lib.E_ARG                   # the arena, one byte too small
    assert b'arena' in hostlib.bmpow_last_error()
    assert call([v5], kinds=bytes([PUBKEY_V4]))[0] == _lib.E_ARG          # the call routes; the kind is not given
    assert call([v5], kinds=bytes([3]))[0] == _lib.E_ARG
    assert b'kind' in hostlib.bmpow_last_error()
    for bad in (bytes(32), ORDER, b'\xff' * 32):                           # the key 0, the group order, above it
        assert call([v5], tables=receive.SealedTables(tags=([tag], [bad])))[0] == _lib.E_ARG
        assert b'private key' in hostlib.bmpow_last_error()
        assert call([v5], tables=receive.SealedTables(trial=([ripe], [bad])))[0] == _lib.E_ARG
        both = receive.NEEDED_DECODED | receive.NEEDED_OWN_TAG
        assert call([v5], tables=receive.SealedTables(needed=([tag], [bad], [ripe], [4], [1], [both])))[0] == _lib.E_ARG
    # ... but the key of an entry that is never tried is not looked at
    rc, recs, match, ln = call([refused], tables=receive.SealedTables(needed=([tag], [bytes(32)], [ripe], [0], [0], [0])))
    assert rc == 0
    # heads that refuse, unknown tags and empty tables never reach a device: the records are the host's
    want, _ = receive.walk_object(BROADCAST, refused)
    assert recs.tobytes() == want.recs.tobytes() and int(recs['status'][0]) == receive.OBJ_BC_VERSION
    assert (int(match[0]), int(ln[0])) == (-1, 0)
    for tables in (None, receive.SealedTables(tags=([b'\x78' * 32], [key])), receive.SealedTables(trial=([ripe], [key]))):
        rc, recs, match, ln = call([v5], tables=tables)
        want, _ = receive.walk_object(BROADCAST, v5)
        want.recs['status'] = receive.OBJ_NOT_SUBSCRIBED
        assert rc == 0 and recs.tobytes() == want.recs.tobytes() and (int(match[0]), int(ln[0])) == (-1, 0)
    # a tag twice in a table is no error: the first entry wins (the device half: tests/test_gpu_rxobjopen.py)
    short = bytes.fromhex(next(e for e in kats['pubkeys_v4'] if e['name'] == 'length_349')['obj'])
    twice = receive.SealedTables(tags=([tag, tag], [key, key]), needed=([tag, tag], [key, key], [ripe, ripe], [4, 4], [1, 1], [3, 3]))
    rc, recs, match, ln = call([refused, short], kinds=bytes([BROADCAST, PUBKEY]), tables=twice)
    assert rc == 0 and recs['status'].tolist() == [receive.OBJ_BC_VERSION, receive.OBJ_V4_TOO_SHORT]
    assert recs['kind'].tolist() == [BROADCAST, PUBKEY_V4]
    # the needed table's order of checks, without a key tried: protocol.py:417, :423, :428, :442
    v4 = _head(PUBKEY, b'\x04') + _payload(192)
    assert len(v4) >= 350
    for tables, status in ((receive.SealedTables(), receive.OBJ_NOT_NEEDED),
                           (receive.SealedTables(needed=([tag], [key], [ripe], [4], [1], [0])), receive.OBJ_ADDRESS_MISMATCH),
                           (receive.SealedTables(needed=([tag], [key], [ripe], [3], [1], [1])), receive.OBJ_ADDRESS_MISMATCH),
                           (receive.SealedTables(needed=([tag], [key], [ripe], [4], [2], [1])), receive.OBJ_ADDRESS_MISMATCH),
                           (receive.SealedTables(needed=([tag], [key], [ripe], [4], [1], [1])), receive.OBJ_NOT_NEEDED)):
        rc, recs, match, ln = call([v4], kinds=bytes([PUBKEY]), tables=tables)
        want, _ = receive.walk_object(PUBKEY_V4, v4)
        want.recs['status'] = status
        assert rc == 0 and recs.tobytes() == want.recs.tobytes() and int(match[0]) == -1, status
