"""Msg processing without a GPU: the walk the kernel is built from (pybitmessage_amd/csrc/bmpow_rx_fmt.h) through
its host-only entry point ``bmpow_rx_walk_msg`` against tests/golden/rx_kats.json (made by running the
reference's primitives, tests/golden/make_rx_golden.py) and, on seeded mutations, against
``signatures.msg_signed_parts`` as an independent restatement; the same header as a stand-alone program under
AddressSanitizer + UBSan (tests/native/rx_sim.cpp); and the Python-level checks that need no device."""
import hashlib
import os
import random
import subprocess

import pytest

from tests.conftest import ROOT, load_golden

CSRC = os.path.join(ROOT, 'pybitmessage_amd', 'csrc')
LINE_STATUS = {None: 0, 444: 1, 478: 2, 492: 3, 496: 4, 500: 5, 506: 6, 531: 7, 'varint': 8, 566: 9}


@pytest.fixture(scope='module')
def kats():
    return load_golden('rx_kats.json')


def walked_fields(res, i=0):
    """The record's walked fields under the fixture's names."""
    r = res.recs[i]
    return {'senderVersion': int(r['sender_version']), 'senderStream': int(r['sender_stream']),
            'behaviour': r['behaviour'].tobytes().hex(), 'nonceTrialsPerByte': int(r['ntpb']), 'extraBytes': int(r['extra']),
            'endOfThePublicKeyPosition': int(r['end_of_pubkey']), 'encoding': int(r['encoding']),
            'message': res.message(i).hex(), 'ackData': res.ackData(i).hex(), 'signature': res.signature(i).hex()}


def signed_data(res, obj, i=0):
    """``signedData`` (``:562-564``) put together again from the record."""
    from pybitmessage_amd.addressgen import encodeVarint
    r = res.recs[i]
    prefix = obj[8:20] + encodeVarint(1) + encodeVarint(int(r['claimed_stream']))
    assert len(prefix) == int(r['prefix_len'])
    return prefix + res.plaintexts[i][:int(r['bottom'])]


def check_row_against_fixture(m, res, i, final):
    """final: the record went through the device (the verdict counts); else the walk alone, which stops at :566"""
    want = LINE_STATUS[m['line']]
    if not final and m['line'] == 566:
        want = 0
    assert int(res.status[i]) == want, m['name']
    got = walked_fields(res, i)
    for k, v in m['record'].items():
        assert got[k] == v, (m['name'], k)
    if m['signed'] is not None:
        signed = signed_data(res, bytes.fromhex(m['obj']), i)
        assert (len(signed), hashlib.sha256(signed).hexdigest()) == (m['signed']['len'], m['signed']['sha256']), m['name']


def test_fixture_covers_what_it_claims(kats):
    msgs = {m['name']: m for m in kats['msgs']}
    assert {None, 444, 478, 492, 496, 500, 506, 531, 566, 'varint'} == {m['line'] for m in msgs.values()}
    for field in ('version', 'stream', 'ntpb', 'extra', 'encoding', 'mlen', 'alen', 'slen', 'head_msgver', 'head_stream'):
        assert msgs[field + '_not_minimal']['line'] in ('varint', 444)
    for field in ('version', 'encoding', 'mlen', 'alen', 'slen', 'head_msgver', 'head_stream'):
        assert msgs[field + '_truncated']['line'] in ('varint', 444)
    ok = [m for m in msgs.values() if m['line'] is None]
    assert {m['record']['senderVersion'] for m in ok} == {1, 2, 3, 4}
    assert {_prefix(m) for m in ok} == {14, 16, 18, 22}
    assert {m['digest'] for m in ok} == {1, 2}
    assert len(msgs['plaintext_169']['plaintext']) == 2 * 169 and msgs['plaintext_169']['line'] == 500
    assert len(msgs['plaintext_170']['plaintext']) == 2 * 170 and msgs['plaintext_170']['line'] == 566
    for name in ('mlen_past_the_end', 'mlen_2_32', 'mlen_2_64_minus_1', 'alen_past_the_end', 'signature_cut_short',
                 'key_x_is_p', 'key_off_the_curve', 'der_r_padded', 'der_r_is_n'):
        assert msgs[name]['line'] == 566, name
    assert msgs['ok_trailing_bytes_behind_signature']['line'] is None
    assert msgs['to_ripe_wrong_then_bad_varint']['line'] == 531
    assert {a['line'] for a in kats['acks']} == {None, 1022, 1030, 1034, 1040, 1048, 1052}
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'rx_kats.json')) <= \
        os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'ident_kats.json'))


def _prefix(m):
    from pybitmessage_amd.ecies import _varint
    obj = bytes.fromhex(m['obj'])
    return 13 + _varint(obj[21:30])[1]


def test_walk_reproduces_every_fixture_record(kats):
    from pybitmessage_amd import receive
    seen = set()
    for m in kats['msgs']:
        obj, plain = bytes.fromhex(m['obj']), bytes.fromhex(m['plaintext'])
        res, verifiable = receive.walk_msg(obj, plain, bytes.fromhex(m['toRipe']))
        if m['line'] == 478:
            continue  # no key decrypts it: the walk never sees this plaintext
        check_row_against_fixture(m, res, 0, final=False)
        if m['line'] is None:
            assert verifiable, m['name']
        if m['name'] in ('key_x_is_p', 'der_r_padded', 'der_r_is_n', 'der_s_is_0', 'signature_cut_short', 'mlen_2_32'):
            assert not verifiable, m['name']
        if m['name'] == 'key_off_the_curve':
            assert verifiable  # the curve kernels decide this one
        seen.add(int(res.status[0]))
    assert seen == {0, 1, 3, 4, 5, 6, 7, 8}


def _mutations(kats, rng):
    """(obj, plaintext) pairs: the fixture's plaintexts with byte flips in the varint region, one plaintext cut
    at every length, and every length varint replaced by the 253 / 254 / 255 forms at their floors, one below
    them (not minimal) and 2^64 - 1."""
    from pybitmessage_amd.ecies import _varint
    rows = [(bytes.fromhex(m['obj']), bytes.fromhex(m['plaintext'])) for m in kats['msgs'] if m['line'] != 478]
    base = next((o, p) for o, p in rows if len(p) > 250)
    out = [(base[0], base[1][:k]) for k in range(len(base[1]) + 1)]
    forms = [b'\xfd\x00\xfd', b'\xfd\x00\xfc', b'\xfe\x00\x01\x00\x00', b'\xfe\x00\x00\xff\xff', b'\xff' + bytes(3) + b'\x01' + bytes(4),
             b'\xff' + bytes(4) + b'\xff' * 4, b'\xff' * 9, b'\xfd', b'\xfe\x01', b'\xff\x01\x02\x03']
    for obj, p in rows:
        if len(p) < 170:
            continue
        # where the varints of a well-formed plaintext lie
        spots, pos = [], 0
        for skip in (0, 4 + 128, 0, 20, 0):
            v = _varint(p[pos:pos + 10])
            if v is None:
                break
            spots.append((pos, v[1]))
            pos += v[1] + skip
        for pos, n in spots + [(150 + k, 1) for k in range(0, 40, 3)]:
            for f in forms:
                out.append((obj, p[:pos] + f + p[pos + n:]))
    while len(out) < 20000:
        obj, p = rows[rng.randrange(len(rows))]
        p = bytearray(p)
        for _ in range(rng.randrange(1, 4)):
            if p:
                region = rng.choice(((0, 12), (130, 190), (0, len(p))))
                i = rng.randrange(region[0], max(region[0] + 1, min(region[1], len(p))))
                if i < len(p):
                    p[i] = rng.choice((0, 1, 252, 253, 254, 255, p[i] ^ (1 << rng.randrange(8))))
        if rng.random() < 0.2:
            del p[rng.randrange(len(p) + 1):]
        if rng.random() < 0.1:
            obj = obj[:20] + bytes(rng.choice((1, 1, 1, 2, 253, 0)) for _ in range(1)) + obj[21:]
        out.append((obj, bytes(p)))
    return out


def test_walk_agrees_with_the_python_extractor_on_mutations(kats):
    """``msg_signed_parts`` knows no toRipe; the row's own bytes at that place are given as the ripe, so the
    walk goes on where the extractor does."""
    from pybitmessage_amd import receive, signatures
    from pybitmessage_amd.ecies import _varint
    rng = random.Random(20251022)
    rows = _mutations(kats, rng)
    assert len(rows) >= 20000
    accepted = refused = 0
    for obj, plain in rows:
        parts = signatures.msg_signed_parts(obj, plain)
        probe, _ = receive.walk_msg(obj, plain, bytes(20))
        end = int(probe.recs[0]['end_of_pubkey'])
        ripe = plain[end:end + 20].ljust(20, b'\x00')
        res, verifiable = receive.walk_msg(obj, plain, ripe)
        status = int(res.status[0])
        if len(plain[end:end + 20]) < 20 and status == receive.WRONG_TO_RIPE:
            # a toRipe slice cut short equals no 20-byte ripe: the reference returns at :531, the extractor goes on
            assert parts is None or len(plain) < end + 20
            refused += 1
            continue
        assert (status == receive.OK) == (parts is not None), (obj.hex(), plain.hex(), status)
        if parts is None:
            refused += 1
            continue
        accepted += 1
        assert signed_data(res, obj) == parts[0]
        assert res.signature(0) == parts[1]
        ver = _varint(plain[:10])
        key_off = ver[1] + _varint(plain[ver[1]:ver[1] + 10])[1] + 4
        assert plain[key_off:key_off + 64] == parts[2]
        assert verifiable == (signatures.parse(parts[1]) is not None and _below_p(parts[2]))
    assert accepted >= 2000 and refused >= 2000, (accepted, refused)


def _below_p(key64):
    p = 2 ** 256 - 2 ** 32 - 977
    return int.from_bytes(key64[:32], 'big') < p and int.from_bytes(key64[32:], 'big') < p


def test_status_constants_and_record_layout():
    import ctypes

    from pybitmessage_amd import _lib, receive
    assert ctypes.sizeof(_lib.BmpowRxMsgRec) == 208 == receive.MSG_REC.itemsize
    for name, _ in _lib.BmpowRxMsgRec._fields_:
        assert getattr(_lib.BmpowRxMsgRec, name).offset == receive.MSG_REC.fields[name][1], name
    assert [receive.OK, receive.MSG_VERSION, receive.NOT_MINE, receive.SENDER_VERSION_0, receive.SENDER_VERSION_HIGH,
            receive.TOO_SHORT, receive.SENDER_STREAM_0, receive.WRONG_TO_RIPE, receive.VARINT,
            receive.BAD_SIGNATURE] == list(range(10))
    assert {receive.STATUS_LINES[s] for s in range(10)} == set(LINE_STATUS)
    lib = _lib.load()  # binds every symbol of include/bmpow_rx.h; no device
    assert lib.bmpow_rx_msgs and lib.bmpow_rx_walk_msg and lib.bmpow_rx_get_stats


def test_argument_errors_before_any_device():
    from pybitmessage_amd import receive
    with pytest.raises(ValueError):
        receive.open_msgs([b'o'], [b'p', b'q'], [bytes(20)])
    with pytest.raises(ValueError):
        receive.open_msgs([b'o'], [b'p'], [bytes(20), bytes(20)])
    with pytest.raises(ValueError):
        receive.open_msgs([b'o'], [b'p'], [bytes(19)])
    with pytest.raises(ValueError):
        receive.walk_msg(b'o', b'p', bytes(21))
    assert len(receive.open_msgs([], [], [])) == 0  # nothing to launch: no device needed


def test_ack_has_valid_header_matches_the_fixture(kats):
    from pybitmessage_amd import receive
    for a in kats['acks']:
        ack = bytes.fromhex(a['ack']) + bytes(a['zeros'])
        assert receive.ack_has_valid_header(ack) == (a['line'] is None), a['name']
    assert receive.ack_has_valid_header(bytearray(bytes.fromhex(kats['acks'][0]['ack'])))


def test_rx_sim_under_sanitizers(tmp_path, kats):
    """A program of its own (its own main, the sanitizer runtimes linked in), never loaded into this process:
    the fixture's rows through the header the kernels are built from, the truncation sweep of one plaintext at
    every length, and the pack routine against data || 0x80 || zeros || bit length for every signed length in
    170 .. 400 under the four prefix widths."""
    rows = []
    for m in kats['msgs']:
        if m['line'] == 478:
            continue
        want = LINE_STATUS[m['line']] if m['line'] != 566 else 0
        rows.append('M %d %s %s %s' % (want, m['obj'][:76] or '-', m['plaintext'] or '-', m['toRipe']))
    (tmp_path / 'rows.txt').write_text('\n'.join(rows) + '\n')
    exe = tmp_path / 'rx_sim'
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-Werror', '-Wno-unknown-pragmas',
                           '-fsanitize=undefined,address', '-fno-sanitize-recover=all', '-static-libasan',
                           '-static-libubsan', '-I', CSRC, os.path.join(ROOT, 'tests', 'native', 'rx_sim.cpp'),
                           '-o', str(exe)])
    env = dict(os.environ)
    env['ASAN_OPTIONS'] = 'halt_on_error=1 detect_leaks=1'
    env['UBSAN_OPTIONS'] = 'halt_on_error=1 print_stacktrace=1'
    r = subprocess.run([str(exe), str(tmp_path / 'rows.txt')], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    assert 'all rx checks passed (%d rows)' % len(rows) in r.stderr
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr
