"""The host-only half of the one-call assembly of outgoing objects (``include/bmpow_tx.h``,
``pybitmessage_amd.outgoing``): the byte-oriented device code as a stand-alone program under the sanitizers,
the bound and the slot layout, the record's layout, the field builders against the reference-made fixture
``tests/golden/tx_kats.json`` (tests/golden/make_tx_golden.py), and the argument errors.  No GPU."""
import ctypes
import hashlib
import os
import subprocess

import numpy as np
import pytest

from pybitmessage_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'pybitmessage_amd', 'csrc')


@pytest.fixture(scope='module')
def kats(golden):
    return golden('tx_kats.json')['objects']


def test_tx_sim_under_sanitizers(tmp_path):
    """A program of its own (its own main, the sanitizer runtimes linked in), never loaded into this process:
    DER against libcrypto's i2d_ECDSA_SIG, the packed signed data for every head length and every residue of
    the signed length mod 64, the tail for every body length 0 .. 80 and signature length 8 .. 72 in a heap
    block of exactly the slot's size, and the words the payload's SHA-512 reads."""
    exe = tmp_path / 'tx_sim'
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-Werror', '-Wno-unknown-pragmas',
                           '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-static-libasan',
                           '-static-libubsan', '-I', CSRC, os.path.join(ROOT, 'tests', 'native', 'tx_sim.cpp'),
                           '-o', str(exe), '-lcrypto'])
    env = dict(os.environ)
    env['ASAN_OPTIONS'] = 'halt_on_error=1 detect_leaks=1'
    env['UBSAN_OPTIONS'] = 'halt_on_error=1 print_stacktrace=1'
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    assert 'all tx checks passed' in r.stderr
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr


def test_record_layouts():
    from pybitmessage_amd import outgoing
    assert ctypes.sizeof(_lib.BmpowTxRec) == outgoing.REC.itemsize == 152
    for name, _ in _lib.BmpowTxRec._fields_:
        assert getattr(_lib.BmpowTxRec, name).offset == outgoing.REC.fields[name][1], name
    assert ctypes.sizeof(_lib.BmpowTxLayout) == 32
    assert ctypes.sizeof(_lib.BmpowTxStats) == 4 * 8 + 7 * 8
    lib = _lib.load()  # binds every symbol of include/bmpow_tx.h; no device
    assert lib.bmpow_tx_objects and lib.bmpow_tx_layout_row and lib.bmpow_tx_get_stats and lib.bmpow_tx_reset_stats
    assert (outgoing.SEALED, outgoing.CLEAR) == (0, 1)
    assert (outgoing.OK, outgoing.BAD_RECIPIENT, outgoing.NO_SIGNATURE, outgoing.TOO_LARGE) == (0, 1, 2, 3)


def test_obj_cap_bounds_actual_lengths(kats):
    from pybitmessage_amd import outgoing, sender
    for k in kats:
        head, body, payload = (bytes.fromhex(k[f]) for f in ('head', 'body', 'payload'))
        assert len(payload) <= outgoing.obj_cap(len(head), len(body)), k['name']
    for head_len in (12, 14, 46, 62):
        for body_len in list(range(0, 70)) + [199, 200, 2000, 2 ** 18]:
            cap = outgoing.obj_cap(head_len, body_len)
            assert cap == head_len + 118 + 16 * ((body_len + 73) // 16 + 1)
            for sig_len in (8, 70, 71, 72):  # a sealed payload with whole coordinates, and a clear one
                plain = body_len + 1 + sig_len
                assert head_len + 22 + 64 + 16 * (plain // 16 + 1) + 32 <= cap
                assert head_len + plain <= cap
            assert head_len + sender.blob_cap(body_len + 73) == cap  # reached: a 72-byte signature, 32-byte coordinates


def _seal_slot_bytes(length):
    clen = 16 * (length // 16 + 1)
    return (max((clen + 95 + 63) // 64 * 64, clen + 118) + 15) // 16 * 16


def test_layout_row_is_the_seal_slot():
    from pybitmessage_amd import outgoing
    lib = _lib.load()
    for head_len in (12, 13, 38, 62):
        for body_len in list(range(0, 130)) + [200, 2000, 4095, 4096, 2 ** 18 - 1, 2 ** 18]:
            lay = outgoing.layout_row(head_len, body_len)
            assert lay['slot_bytes'] == _seal_slot_bytes(body_len + 73) and lay['slot_bytes'] % 16 == 0
            # the library's own planner: the second row of a set starts where the first one's slot ends
            lens = (ctypes.c_uint64 * 2)(body_len + 73, 0)
            sets, offs = (ctypes.c_uint32 * 2)(), (ctypes.c_uint64 * 2)()
            assert lib.bmpow_seal_plan(2, lens, 1 << 18, 1 << 40, sets, offs) == 1
            assert offs[1] == lay['slot_bytes']
            assert lay['body_at'] == 96 and lay['tail_at'] == 96 + body_len
            assert lay['plain_cap'] == body_len + 73 and lay['tail_at'] + 73 <= lay['slot_bytes']
            assert lay['signed_len'] == head_len + body_len
            assert lay['hash_blocks'] == (head_len + body_len + 9 + 63) // 64
            # the padded signed data never outgrows the slot: one cut of the sets bounds both pools
            assert 64 * lay['hash_blocks'] <= lay['slot_bytes']
    lay = _lib.BmpowTxLayout()
    for head_len, body_len in ((11, 0), (63, 0), (0, 0), (12, 2 ** 18 + 1)):
        assert lib.bmpow_tx_layout_row(head_len, body_len, ctypes.byref(lay)) == _lib.E_ARG
    assert lib.bmpow_tx_layout_row(12, 0, None) == _lib.E_ARG


def _tag(f):
    from pybitmessage_amd.worker import _varint
    data = _varint(f['version']) + _varint(f['stream']) + bytes.fromhex(f['ripe'])
    return hashlib.sha512(hashlib.sha512(data).digest()).digest()[32:]


def test_builders_give_the_fixtures_head_and_body(kats):
    from pybitmessage_amd import outgoing, worker
    seen = set()
    for k in kats:
        f = k['fields']
        h = {name: bytes.fromhex(f[name]) for name in ('bitfield', 'pubSigningKey', 'pubEncryptionKey')}
        if f['type'] == 'msg':
            head = outgoing.msg_head(f['embeddedTime'], f['toStream'])
            body = worker.msg_plaintext(f['version'], f['stream'], h['bitfield'], h['pubSigningKey'], h['pubEncryptionKey'],
                                        bytes.fromhex(f['toRipe']), f['encoding'], bytes.fromhex(f['message']),
                                        bytes.fromhex(f['fullAckPayload']), f['ntpb'], f['extra'])
        elif f['type'] == 'broadcast':
            head = outgoing.broadcast_head(f['embeddedTime'], f['version'], f['stream'], _tag(f))
            body = worker.broadcast_plaintext(f['version'], f['stream'], h['bitfield'], h['pubSigningKey'],
                                              h['pubEncryptionKey'], f['encoding'], bytes.fromhex(f['message']), f['ntpb'],
                                              f['extra'])
        else:
            head = outgoing.pubkey_head(f['embeddedTime'], f['version'], f['stream'], _tag(f))
            body = worker.pubkey_plaintext(h['bitfield'], h['pubSigningKey'], h['pubEncryptionKey'], f['ntpb'], f['extra'])
        assert head.hex() == k['head'], k['name']
        assert body.hex() == k['body'], k['name']
        assert 12 <= len(head) <= 62
        assert hashlib.sha512(bytes.fromhex(k['payload'])).hexdigest() == k['initial_hash']
        seen.add((f['type'], f['version'], k['kind'], k['digest']))
    # the cases the fixture must hold: msgs from v2, v3, v4; broadcasts v4 and v5; pubkeys v3 (clear) and v4; both digests
    for want in (('msg', 2, 'sealed', 'sha256'), ('msg', 3, 'sealed', 'sha256'), ('msg', 4, 'sealed', 'sha256'),
                 ('msg', 3, 'sealed', 'sha1'), ('broadcast', 2, 'sealed', 'sha256'), ('broadcast', 3, 'sealed', 'sha256'),
                 ('broadcast', 4, 'sealed', 'sha256'), ('broadcast', 4, 'sealed', 'sha1'), ('pubkey', 3, 'clear', 'sha256'),
                 ('pubkey', 3, 'clear', 'sha1'), ('pubkey', 4, 'sealed', 'sha256'), ('pubkey', 4, 'sealed', 'sha1')):
        assert want in seen, want
    assert {len(bytes.fromhex(k['head'])) for k in kats} >= {14, 16, 18, 22, 46, 48, 50}
    assert any(k['fields'].get('message') == '' for k in kats)
    assert any(k['fields'].get('fullAckPayload') for k in kats) and any(k['fields'].get('fullAckPayload') == '' for k in kats)


def test_built_pow_object_carries_the_given_hash():
    from pybitmessage_amd import worker
    payload = bytes(8) + b'\x00\x00\x00\x02\x01\x01' + b'x' * 100
    o = worker.BuiltPowObject(payload, bytes(range(64)), 3600, 10, 10, tag=7)
    assert o.initial_hash == bytes(range(64)) and o.payload == payload and o.tag == 7
    assert o.target == worker.PowObject(payload, 3600, 10, 10).target
    with pytest.raises(ValueError):
        worker.BuiltPowObject(payload, bytes(63), 3600)


def test_argument_errors_before_any_device():
    from pybitmessage_amd import outgoing
    head, key = bytes(14), b'\x01' * 32
    with pytest.raises(ValueError):
        outgoing.build_objects([0], [head], [b''], [key], [None], 'md5')
    with pytest.raises(ValueError):
        outgoing.build_objects([0, 0], [head], [b''], [key], [None])
    with pytest.raises(ValueError):
        outgoing.build_objects([2], [head], [b''], [key], [None])
    with pytest.raises(ValueError):
        outgoing.build_objects([1], [bytes(11)], [b''], [key], [None])
    with pytest.raises(ValueError):
        outgoing.build_objects([1], [bytes(63)], [b''], [key], [None])
    with pytest.raises(ValueError):
        outgoing.build_objects([1], [head], [b''], [bytes(33)], [None])
    with pytest.raises(ValueError):
        outgoing.build_objects([1], [head], [b''], [key], [None], nonces=[key, key])
    with pytest.raises(ValueError):
        outgoing.build_objects([0], [head], [b''], [key], [bytes(64)], ivs=[bytes(15)])
    with pytest.raises(ValueError):
        outgoing.build_pubkeys([outgoing.PubkeyFields(0, 2, 1, bytes(20), bytes(4), bytes(64), bytes(64), None, None, key)])
    assert len(outgoing.build_objects([], [], [], [], [])) == 0  # nothing to launch: no device needed
    assert outgoing.build_objects([], [], [], [], []).accepted() == []


def test_c_abi_refuses_bad_arguments_before_any_device():
    lib = _lib.load()
    rec = (_lib.BmpowTxRec * 1)()
    out = ctypes.create_string_buffer(1024)
    outs = (ctypes.c_void_p * 1)(ctypes.addressof(out))
    N = bytes.fromhex('FFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141')
    one = bytes(31) + b'\x01'

    def call(kind=1, head_len=14, body=b'body', priv=one, pub=None, digest=2, nonce=one, eph=None, cap=1024, n=1):
        heads = (ctypes.c_char_p * 1)(bytes(64))
        bodies = (ctypes.c_char_p * 1)(body)
        lens = (ctypes.c_uint64 * 1)(len(body))
        caps = (ctypes.c_uint64 * 1)(cap)
        return lib.bmpow_tx_objects(n, bytes([kind]), ctypes.cast(heads, ctypes.c_void_p), bytes([head_len]),
                                    ctypes.cast(bodies, ctypes.c_void_p), lens, priv, pub, digest, nonce, eph, None,
                                    ctypes.cast(outs, ctypes.c_void_p), caps, ctypes.cast(rec, ctypes.c_void_p))

    assert call(n=0) == 0  # nothing launched
    for bad in (dict(kind=2), dict(head_len=11), dict(head_len=63), dict(priv=bytes(32)), dict(priv=N), dict(digest=3),
                dict(nonce=bytes(32)), dict(nonce=N), dict(kind=0), dict(kind=0, pub=bytes(64), eph=bytes(32)),
                dict(kind=0, pub=bytes(64), eph=N), dict(cap=14 + 118 + 16 * ((4 + 73) // 16 + 1) - 1)):
        assert call(**bad) == _lib.E_ARG, bad
        assert lib.bmpow_last_error()
    st = _lib.BmpowTxStats()
    assert lib.bmpow_tx_get_stats(None) == _lib.E_ARG and lib.bmpow_tx_get_stats(ctypes.byref(st)) == 0
    assert st.launches == 0 and st.sets == 0
