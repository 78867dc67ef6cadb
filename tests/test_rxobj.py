"""Broadcast and pubkey processing without a GPU: the walks the kernels are built from
(pybitmessage_amd/csrc/bmpow_rx_fmt.h) through their host-only entry point ``bmpow_rx_walk_object`` against
tests/golden/rxobj_kats.json (made by running the reference's primitives, tests/golden/make_rxobj_golden.py), against
the ``broadcasts`` and ``pubkeys_v4`` of ident_kats.json and, with one plaintext of each kind cut at every length,
against the extractors of ``signatures`` as an independent restatement; the same header as a stand-alone program
under AddressSanitizer + UBSan (tests/native/rxobj_sim.cpp); and the Python-level checks that need no device."""
import hashlib
import os
import subprocess

import pytest

from tests.conftest import ROOT, load_golden

CSRC = os.path.join(ROOT, 'pybitmessage_amd', 'csrc')
BROADCAST, PUBKEY_V4, PUBKEY = 0, 1, 2
# the reference's returning line -> BMPOW_RXO_* (include/bmpow_rx.h), per kind
LINE_STATUS = {
    BROADCAST: {None: 0, 'varint': 1, 760: 2, 830: 3, 838: 3, 848: 4, 882: 5, 893: 6, 901: 7, 916: 8, 801: 14, 810: 14, 820: 15},
    PUBKEY_V4: {None: 0, 'varint': 1, 484: 8, 497: 5, 457: 15, 417: 16, 442: 16, 423: 17, 428: 17, 411: 18},
    PUBKEY: {None: 0, 'varint': 1, 283: 9, 287: 10, 410: 11, 293: 12, 346: 12, 304: 13, 374: 8},
}
BEFORE_THE_DEVICE = (14, 15, 16, 17, 18)  # the wrappers' statuses: no plaintext exists
SECTIONS = (('broadcasts', BROADCAST), ('pubkeys_v4', PUBKEY_V4), ('pubkeys', PUBKEY))


@pytest.fixture(scope='module')
def kats():
    return load_golden('rxobj_kats.json')


@pytest.fixture(scope='module')
def ident_kats():
    return load_golden('ident_kats.json')


def fixture_rows(kats):
    """(kind, entry, obj, plaintext or None, expect) of every row of rxobj_kats.json."""
    out = []
    for section, kind in SECTIONS:
        for e in kats[section]:
            plain = bytes.fromhex(e['plaintext']) if e.get('plaintext') is not None else None
            out.append((kind, e, bytes.fromhex(e['obj']), plain, bytes.fromhex(e.get('expect') or '')))
    return out


def device_rows(kats):
    """The rows for the device call: those with a plaintext, every clear pubkey, and -- with an empty plaintext,
    which they never read -- those whose header the walk itself refuses."""
    out = []
    for kind, e, obj, plain, expect in fixture_rows(kats):
        if plain is None and kind != PUBKEY and e['line'] in (760, 'varint'):
            plain = b''
        if kind == PUBKEY or plain is not None:
            out.append((kind, e, obj, plain, expect))
    return out


def walked_fields(res, i=0):
    """The record's walked fields under the fixture's names."""
    r = res.recs[i]
    out = {'objectVersion': int(r['object_version']), 'objectStream': int(r['object_stream']), 'tagOff': int(r['tag_off']),
           'payloadOff': int(r['payload_off']), 'senderVersion': int(r['sender_version']),
           'senderStream': int(r['sender_stream']), 'behaviour': r['behaviour'].tobytes().hex(),
           'nonceTrialsPerByte': int(r['ntpb']), 'extraBytes': int(r['extra']), 'encoding': int(r['encoding']),
           'message': res.message(i).hex(), 'signature': res.signature(i).hex()}
    if r['kind'] == BROADCAST:
        out['pubkeyData'] = res.pubkeyData(i).hex()
    else:
        out['storedData'] = res.storedData(i).hex()
    return out


def check_row_against_fixture(kind, e, res, i, final):
    """final: the record went through the device (the comparisons and the verdict count); else the walk alone,
    which leaves the status that follows the ripe / tag comparison beside ``keys_hashed`` and stops at verify."""
    want, rec = LINE_STATUS[kind][e['line']], res.recs[i]
    status = int(rec['status'])
    assert int(rec['kind']) == kind
    if final or want not in (5, 6, 8):
        assert status == want, e['name']
    elif want in (5, 6):
        assert rec['keys_hashed'] == 1 and status != want, e['name']  # whole keys: the device compares
    else:
        assert status == 0 and rec['keys_hashed'] == 1, e['name']
    if final and want in (5, 6) and kind == BROADCAST:  # the reference returns before it reads on
        assert (int(rec['encoding']), int(rec['msg_len']), int(rec['sig_len']), int(rec['bottom'])) == (0, 0, 0, 0)
    got = walked_fields(res, i)
    for k, v in (e['record'] or {}).items():
        assert got[k] == v, (e['name'], k)
    if e['signed'] is not None:
        signed = res.signedData(i)
        assert (len(signed), hashlib.sha256(signed).hexdigest()) == (e['signed']['len'], e['signed']['sha256']), e['name']
        assert int(rec['prefix_len']) == (0 if kind == PUBKEY else int(rec['payload_off']) - 8)


def test_fixture_covers_every_status_of_every_kind(kats):
    from pybitmessage_amd import receive
    for section, kind in SECTIONS:
        lines = {e['line'] for e in kats[section]}
        assert {LINE_STATUS[kind][ln] for ln in lines} == set(receive.OBJ_STATUS_LINES[kind]), section
        # ... and every line the status table names, but :442, which needs two entries of neededPubkeys to collide
        named = {ln for st in receive.OBJ_STATUS_LINES[kind].values() for ln in st}
        assert named - lines <= {442}, section
    by_name = {section: {e['name']: e for e in kats[section]} for section, _ in SECTIONS}
    b, v4, pk = by_name['broadcasts'], by_name['pubkeys_v4'], by_name['pubkeys']
    assert b['v4_wrong_ripe_and_encoding_0']['line'] == 882 and b['v5_wrong_tag_and_mlen_not_minimal']['line'] == 893
    assert b['v5_right_tag_siglen_not_minimal']['line'] == 'varint'
    assert b['v4_signing_key_off_the_curve_right_ripe']['line'] == 916 and b['v4_signing_key_x_is_p_right_ripe']['line'] == 916
    assert v4['wrong_ripe_and_signature_bit_flipped']['line'] == 484 and v4['keys_of_another_address']['line'] == 497
    assert (len(v4['length_349']['obj']), len(v4['length_350_does_not_decrypt']['obj'])) == (698, 700)
    assert (v4['length_349']['line'], v4['length_350_does_not_decrypt']['line'], v4['tag_not_needed']['line']) == (411, 457, 417)
    assert len(pk['v2_length_146_encryption_key_short']['obj']) == 292 and len(pk['v2_length_145']['obj']) == 290
    assert (len(pk['v3_length_169']['obj']), len(pk['v3_length_170_signature_cut_short']['obj'])) == (338, 340)
    assert {e['digest'] for e in kats['pubkeys'] if e['line'] is None} == {0, 1, 2}
    for section in ('broadcasts', 'pubkeys_v4'):
        ok = [e for e in kats[section] if e['line'] is None]
        assert {e['digest'] for e in ok} == {1, 2}
        want = {46, 48, 50, 54} if section == 'pubkeys_v4' else {14, 16, 18, 22, 46, 48, 50, 54}
        assert {e['record']['payloadOff'] - 8 for e in ok} == want
    assert {e['record']['objectStream'] for e in kats['pubkeys'] if e['line'] is None} == {1, 300, 70000, 2 ** 32}
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'rxobj_kats.json')) < 200 * 1024


def test_walk_reproduces_every_fixture_record(kats):
    from pybitmessage_amd import receive
    seen = {BROADCAST: set(), PUBKEY_V4: set(), PUBKEY: set()}
    for kind, e, obj, plain, _expect in fixture_rows(kats):
        want = LINE_STATUS[kind][e['line']]
        res, verifiable = receive.walk_object(kind, obj, plain)
        if want in BEFORE_THE_DEVICE:
            # the wrapper decides these; the header walk it uses gets through
            assert plain is None and int(res.status[0]) == 0, e['name']
            for k, v in (e['record'] or {}).items():
                assert walked_fields(res)[k] == v, (e['name'], k)
            continue
        check_row_against_fixture(kind, e, res, 0, final=False)
        seen[kind].add(int(res.status[0]))
        if e['line'] is None and (kind != PUBKEY or e['record']['objectVersion'] == 3):
            assert verifiable, e['name']
        if 'x_is_p' in e['name'] or 'cut_short' in e['name'] or e['line'] == 'varint':
            assert not verifiable, e['name']
        if 'off_the_curve' in e['name']:
            assert verifiable == (e['line'] == 916 or e['line'] == 374), e['name']  # the curve kernels decide
    assert seen == {BROADCAST: {0, 1, 2, 3, 4, 7}, PUBKEY_V4: {0, 1}, PUBKEY: {0, 1, 9, 10, 11, 12, 13}}


def test_walk_reproduces_the_identification_fixture(ident_kats):
    """The 50 broadcasts and the encrypted pubkeys of ident_kats.json carry ``line`` and ``plaintext``; its cut
    plaintexts are the keys cut short that the walk itself turns into :882 / :893 and :484."""
    from pybitmessage_amd import receive
    lines = {760: 2, 801: 0, 810: 0, 820: 0, 'varint': 1, 830: 3, 838: 3, 848: 4, 901: 7}
    for b in ident_kats['broadcasts']:
        obj = bytes.fromhex(b['obj'])
        plain = bytes.fromhex(b['plaintext']) if b['plaintext'] is not None else None
        res, _ = receive.walk_object(BROADCAST, obj, plain)
        status, hashed = int(res.status[0]), int(res.recs[0]['keys_hashed'])
        if b['line'] in (882, 893):
            assert hashed or status == (5 if b['line'] == 882 else 6), b['name']
            assert hashed == (len(plain) >= int(res.recs[0]['end_of_pubkey']) >= 128), b['name']
        elif b['line'] in (None, 916):
            assert (status, hashed) == (0, 1), b['name']
        else:
            assert status == lines[b['line']], b['name']
        if b['parts'] is not None and status == 0:
            p = b['parts']
            assert res.signedData(0).hex() == p['signedData'] and res.signature(0).hex() == p['signature'], b['name']
            assert (res.message(0).hex(), res.pubkeyData(0).hex()) == (p['message'], p['pubkeyData']), b['name']
            assert (int(res.senderVersion[0]), int(res.senderStream[0]), int(res.encoding[0])) == \
                (p['senderVersion'], p['senderStream'], p['encoding']), b['name']
    for k in ident_kats['pubkeys_v4']:
        obj, plain = bytes.fromhex(k['obj']), bytes.fromhex(k['plaintext'])
        res, verifiable = receive.walk_object(PUBKEY_V4, obj, plain)
        status = int(res.status[0])
        if k['line'] == 'varint':
            assert status == 1, k['name']
        elif len(plain) < 132:
            assert k['line'] == 484 and status == 8 and not verifiable, k['name']
        else:
            assert status == 0 and res.recs[0]['keys_hashed'] == 1, k['name']
        if k['parts'] is not None:
            p = k['parts']
            assert (res.signedData(0).hex(), res.signature(0).hex(), res.storedData(0).hex()) == \
                (p['signedData'], p['signature'], p['storedData']), k['name']
            assert (int(res.objectVersion[0]), int(res.objectStream[0])) == (p['addressVersion'], p['stream'])
            assert obj[int(res.recs[0]['tag_off']):int(res.recs[0]['payload_off'])].hex() == p['tag']


def test_every_truncation_agrees_with_the_python_extractors(kats):
    from pybitmessage_amd import receive, signatures
    by_name = {section: {e['name']: e for e in kats[section]} for section, _ in SECTIONS}
    counts = {}
    # a broadcast: broadcast_signed_parts refuses what the plaintext alone decides; keys cut short are the
    # walk's :882 / :893, which the extractor leaves to its caller
    for name in ('v4_ok_stream_300', 'v5_ok_stream_70000'):
        e = by_name['broadcasts'][name]
        obj, plain = bytes.fromhex(e['obj']), bytes.fromhex(e['plaintext'])
        for cut in range(len(plain) + 1):
            res, verifiable = receive.walk_object(BROADCAST, obj, plain[:cut])
            parts = signatures.broadcast_signed_parts(obj, plain[:cut])
            status = int(res.status[0])
            counts[name, status] = counts.get((name, status), 0) + 1
            if status in (5, 6):
                assert res.recs[0]['keys_hashed'] == 0 and (parts is None or len(parts.pubEncryptionKey64) < 64), cut
                continue
            assert (status == 0) == (parts is not None), (name, cut, status)
            if parts is None:
                assert status in (1, 3, 4, 7), (name, cut, status)
                continue
            assert (res.signedData(0), res.signature(0), res.message(0), res.pubkeyData(0)) == \
                (parts.signedData, parts.signature, parts.message, parts.pubkeyData), (name, cut)
            assert (int(res.senderVersion[0]), int(res.senderStream[0]), int(res.encoding[0])) == \
                (parts.senderVersion, parts.senderStream, parts.encoding)
            assert verifiable == (cut == len(plain)), (name, cut)
    e = by_name['pubkeys_v4']['ok_stream_300']
    obj, plain = bytes.fromhex(e['obj']), bytes.fromhex(e['plaintext'])
    for cut in range(len(plain) + 1):
        res, verifiable = receive.walk_object(PUBKEY_V4, obj, plain[:cut])
        parts = signatures.pubkey_v4_signed_parts(obj, plain[:cut])
        status = int(res.status[0])
        counts['v4', status] = counts.get(('v4', status), 0) + 1
        assert (status == 1) == (parts is None), cut
        if parts is None:
            continue
        assert status == (8 if cut < 132 else 0) and res.recs[0]['keys_hashed'] == (cut >= 132), cut
        assert (res.signedData(0), res.signature(0), res.storedData(0)) == (parts.signedData, parts.signature, parts.storedData), cut
        assert verifiable == (cut == len(plain)), cut
    e = by_name['pubkeys']['v3_ok_stream_300']
    obj = bytes.fromhex(e['obj'])
    for cut in range(len(obj) + 1):
        res, verifiable = receive.walk_object(PUBKEY, obj[:cut])
        parts = signatures.pubkey_v3_signed_parts(obj[:cut])
        status = int(res.status[0])
        counts['v3', status] = counts.get(('v3', status), 0) + 1
        assert (status == 0) == (parts is not None), (cut, status)
        if parts is None:
            continue
        key_off = int(res.recs[0]['payload_off']) + 4
        assert (res.signedData(0), res.signature(0), obj[key_off:key_off + 64]) == parts, cut
        assert verifiable == (cut == len(obj)), cut
    # cuts 0 .. 20 read as version 0; 22 and 23 end inside the stream's three bytes; 21 (the stream reads as 0)
    # and 24 .. 169 are below the floor of :346, which comes before the plaintext's varints are read
    assert counts['v3', 9] == 21 and counts['v3', 1] == 2 and counts['v3', 12] == 1 + 170 - 24 and counts['v3', 0] > 60
    assert counts['v4', 8] == 132 and counts['v4', 1] == 4 and counts['v4', 0] > 70
    for name in ('v4_ok_stream_300', 'v5_ok_stream_70000'):
        assert counts[name, 3] == 1 and counts[name, 4] >= 1 and counts[name, 7] >= 1 and counts[name, 0] > 60
    assert counts['v4_ok_stream_300', 5] > 100 and counts['v5_ok_stream_70000', 6] > 100


def test_status_constants_and_record_layout():
    import ctypes

    from pybitmessage_amd import _lib, receive
    assert ctypes.sizeof(_lib.BmpowRxObjRec) == 216 == receive.OBJ_REC.itemsize
    for name, _ in _lib.BmpowRxObjRec._fields_:
        assert getattr(_lib.BmpowRxObjRec, name).offset == receive.OBJ_REC.fields[name][1], name
    names = ['OK', 'VARINT', 'BC_VERSION', 'SENDER_VERSION', 'STREAM_MISMATCH', 'WRONG_RIPE', 'WRONG_TAG', 'ENCODING_0',
             'BAD_SIGNATURE', 'ADDRESS_VERSION_0', 'ADDRESS_VERSION', 'NEEDS_DECRYPTION', 'TOO_SHORT', 'KEY_SHORT',
             'NOT_SUBSCRIBED', 'NOT_DECRYPTED', 'NOT_NEEDED', 'ADDRESS_MISMATCH', 'V4_TOO_SHORT']
    assert [getattr(receive, 'OBJ_' + n) for n in names] == list(range(19))
    assert (receive.KIND_BROADCAST, receive.KIND_PUBKEY_V4, receive.KIND_PUBKEY) == (BROADCAST, PUBKEY_V4, PUBKEY)
    # the header's numbers are these
    with open(os.path.join(ROOT, 'include', 'bmpow_rx.h')) as f:
        text = f.read()
    for value, n in enumerate(names):
        assert '#define BMPOW_RXO_%s %d ' % (n, value) in text or '#define BMPOW_RXO_%s %d\n' % (n, value) in text, n
    for kind in (BROADCAST, PUBKEY_V4, PUBKEY):
        for status, lines in receive.OBJ_STATUS_LINES[kind].items():
            assert all(LINE_STATUS[kind][ln] == status for ln in lines), (kind, status)
    lib = _lib.load()  # binds every symbol of include/bmpow_rx.h; no device
    assert lib.bmpow_rx_objects and lib.bmpow_rx_walk_object and lib.bmpow_rx_obj_get_stats and lib.bmpow_rx_obj_reset_stats


def test_argument_errors_before_any_device():
    import ctypes

    import numpy as np

    from pybitmessage_amd import _lib, receive
    with pytest.raises(ValueError):
        receive.open_objects([0], [b'o'], [b'p', b'q'], [None])
    with pytest.raises(ValueError):
        receive.open_objects([0, 1], [b'o'], [b'p'], [None])
    with pytest.raises(ValueError):
        receive.open_objects([3], [b'o'], [b'p'], [None])
    with pytest.raises(ValueError):
        receive.open_objects([0], [b'o'], [b'p'], [bytes(33)])
    with pytest.raises(ValueError):
        receive.walk_object(5, b'o', b'p')
    assert len(receive.open_objects([], [], [], [])) == 0  # nothing to launch: no device needed
    for empty in (receive.open_broadcasts([], []), receive.open_pubkeys([], {})):
        assert len(empty) == 0 and empty.accepted() == []
    lib = _lib.load()
    rec = _lib.BmpowRxObjRec()
    assert lib.bmpow_rx_walk_object(3, b'o', 1, b'p', 1, None, ctypes.byref(rec)) == _lib.E_ARG
    assert lib.bmpow_rx_walk_object(0, b'o', 1, None, 1, None, ctypes.byref(rec)) == _lib.E_ARG
    assert lib.bmpow_rx_walk_object(0, b'o', 1, b'p', (1 << 31) + 1, None, ctypes.byref(rec)) == _lib.E_ARG
    assert lib.bmpow_rx_walk_object(2, b'o', (1 << 31) + 1, None, 0, None, ctypes.byref(rec)) == _lib.E_ARG
    # the batch call checks its rows before it selects a device
    out = np.zeros(1, dtype=receive.OBJ_REC)
    one = (ctypes.c_char_p * 1)(b'o')
    lens = (ctypes.c_uint64 * 1)(1)
    big = (ctypes.c_uint64 * 1)((1 << 31) + 1)
    ptr = ctypes.cast(one, ctypes.c_void_p)
    assert lib.bmpow_rx_objects(0, None, None, None, None, None, None, out.ctypes.data) == 0
    assert lib.bmpow_rx_objects(1, bytes([3]), ptr, lens, ptr, lens, bytes(32), out.ctypes.data) == _lib.E_ARG
    assert b'kind' in lib.bmpow_last_error()
    assert lib.bmpow_rx_objects(1, bytes([0]), ptr, lens, ptr, big, bytes(32), out.ctypes.data) == _lib.E_ARG
    assert lib.bmpow_rx_objects(1, bytes([2]), ptr, big, ptr, lens, bytes(32), out.ctypes.data) == _lib.E_ARG
    assert lib.bmpow_rx_objects(1, bytes([0]), ptr, lens, ptr, lens, None, out.ctypes.data) == _lib.E_ARG


def test_rxobj_sim_under_sanitizers(tmp_path, kats, ident_kats):
    """A program of its own (its own main, the sanitizer runtimes linked in), never loaded into this process:
    the rows of both fixtures through the header the kernels are built from, one source of each kind cut at
    every length, and the pack routine against prefix || data || 0x80 || zeros || bit length for every signed
    length 130 .. 400 under every prefix length 0, 14 .. 22, 46 .. 62 with the source read from byte 0 and 8."""
    from pybitmessage_amd import receive
    rows = []
    for kind, e, obj, plain, _expect in fixture_rows(kats):
        if kind != PUBKEY and plain is None:
            continue
        res, _ = receive.walk_object(kind, obj, plain)  # pinned to the fixture by the tests above
        rows.append('%d %d %d %s %s' % (kind, int(res.status[0]), int(res.recs[0]['keys_hashed']), obj.hex() or '-',
                                       (plain or b'').hex() or '-'))
    for section, kind in (('broadcasts', BROADCAST), ('pubkeys_v4', PUBKEY_V4)):
        for e in ident_kats[section]:
            if e['plaintext'] is None:
                continue
            res, _ = receive.walk_object(kind, bytes.fromhex(e['obj']), bytes.fromhex(e['plaintext']))
            rows.append('%d %d %d %s %s' % (kind, int(res.status[0]), int(res.recs[0]['keys_hashed']), e['obj'], e['plaintext'] or '-'))
    (tmp_path / 'rows.txt').write_text('\n'.join(rows) + '\n')
    exe = tmp_path / 'rxobj_sim'
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-Werror', '-Wno-unknown-pragmas',
                           '-fsanitize=undefined,address', '-fno-sanitize-recover=all', '-static-libasan',
                           '-static-libubsan', '-I', CSRC, os.path.join(ROOT, 'tests', 'native', 'rxobj_sim.cpp'),
                           '-o', str(exe)])
    env = dict(os.environ)
    env['ASAN_OPTIONS'] = 'halt_on_error=1 detect_leaks=1'
    env['UBSAN_OPTIONS'] = 'halt_on_error=1 print_stacktrace=1'
    r = subprocess.run([str(exe), str(tmp_path / 'rows.txt')], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    assert 'all rxobj checks passed (%d rows)' % len(rows) in r.stderr
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr
