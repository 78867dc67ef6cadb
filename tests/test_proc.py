"""The object processor's dispatch, the parts that need no device: the ABI table of ``include/bmpow_proc.h``, the
struct layouts, ``bmpow_proc_walk`` against every getpubkey and onionpeer row of the reference-made fixture
``tests/golden/proc_kats.json`` (tests/golden/make_proc_golden.py), and the watch set's host calls on a host-only
dispatcher."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from pybitmessage_amd import _lib, processor
from tests.conftest import ROOT
from tests.proc_expect import address_table, check_verdict, expected_acks, expected_status

HEADER = os.path.join(ROOT, 'include', 'bmpow_proc.h')


@pytest.fixture(scope='module')
def kats(golden):
    return golden('proc_kats.json')


@pytest.fixture(scope='module')
def hostlib():
    return _lib.load()


def test_every_declared_symbol_is_exported_and_bound(hostlib):
    text = open(HEADER).read()
    syms = sorted(set(re.findall(r'BMPOW_API\s+[\w\s\*]+?\b(\w+)\s*\(', text)))
    assert 'bmpow_proc_batch' in syms and 'bmpow_proc_walk' in syms and len(syms) == 13
    assert syms == sorted(name for name, _, _ in _lib.PROC_SIGNATURES)
    raw = ctypes.CDLL(_lib.lib_path())
    for name, res, args in _lib.PROC_SIGNATURES:
        assert hasattr(raw, name), name
        fn = getattr(hostlib, name)
        assert fn.restype == res and list(fn.argtypes) == args, name


@pytest.mark.parametrize('ctype,cls,dtype', [('bmpow_proc_rec', _lib.BmpowProcRec, processor.REC_DTYPE),
                                             ('bmpow_proc_address', _lib.BmpowProcAddress, processor.ADDRESS_DTYPE),
                                             ('bmpow_proc_params', _lib.BmpowProcParams, None),
                                             ('bmpow_proc_stats', _lib.BmpowProcStats, None)])
def test_structs_match_the_header(tmp_path, ctype, cls, dtype):
    fields = [f for f, _ in cls._fields_]
    src = tmp_path / 'sz.c'
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "bmpow_proc.h"\nint main(void) {\n'
                   '  printf("%%zu", sizeof(%s));\n' % ctype +
                   ''.join('  printf(" %%zu", offsetof(%s, %s));\n' % (ctype, f) for f in fields) +
                   '  return 0;\n}\n')
    exe = tmp_path / 'sz'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got[0] == ctypes.sizeof(cls)
    assert got[1:] == [getattr(cls, f).offset for f in fields]
    if dtype is not None:  # the numpy views the Python layer hands out
        assert dtype.itemsize == got[0] and [dtype.fields[f][1] for f in fields] == got[1:]


def test_header_values_match_the_module():
    text = open(HEADER).read()
    values = {name: int(v.rstrip('u'), 0) for name, v in re.findall(r'#define BMPOW_PROC_(\w+) (\w+)', text)}
    for name in ('TOO_LONG', 'MALFORMED', 'VERSION_ZERO', 'VERSION_ONE', 'VERSION_TOO_HIGH', 'SHORT_HASH', 'SHORT_TAG',
                 'NOT_MINE', 'VERSION_MISMATCH', 'STREAM_MISMATCH', 'CHAN', 'SENT_RECENTLY', 'SEND_V2', 'SEND_V3', 'SEND_V4',
                 'NO_HOST', 'RAISES', 'PEER', 'NONE', 'NO_ROW'):
        assert values[name] == getattr(processor, name), name
    for name in ('GETPUBKEY', 'PUBKEY', 'MSG', 'BROADCAST', 'ONIONPEER', 'UNKNOWN_TYPE'):
        assert values['ROUTE_' + name] == getattr(processor, name), name
    for name in ('NOT_CHECKED', 'NOT_WATCHED', 'FOUND', 'FOUND_EARLIER'):
        assert values['ACK_' + name] == getattr(processor, name), name
    for name in ('V4', 'ONION', 'V6'):
        assert values['HOST_' + name] == getattr(processor, name), name


def test_walk_against_every_golden_row(kats):
    table = address_table(kats)
    assert [processor.tag_of(a['version'], a['stream'], bytes.fromhex(a['ripe'])).hex() for a in kats['addresses']] == \
        [a['tag'] for a in kats['addresses']]
    seen = set()
    for row in kats['rows']:
        data = bytes.fromhex(row['data'])
        rec = processor.walk(row['type'], data, table, now=kats['now'])
        check_verdict(kats, row, rec, data, table)
        assert rec['ack'] == processor.NOT_CHECKED and rec['ack_first'] == processor.NO_ROW
        seen.add(int(rec['status']))
    assert seen == set(range(19)), sorted(set(range(19)) - seen)  # every status of the header at least once


def test_the_fixture_holds_the_cases_that_matter(kats):
    rows = {r['name']: r for r in kats['rows']}
    assert len(rows) == len(kats['rows']) > 64
    assert len(bytes.fromhex(rows['gp_len_200']['data'])) == 200 and expected_status(rows['gp_len_200']) == processor.SEND_V3
    assert len(bytes.fromhex(rows['gp_len_201']['data'])) == 201 and expected_status(rows['gp_len_201']) == processor.TOO_LONG
    assert expected_status(rows['gp_len_201_bad_varint']) == processor.TOO_LONG  # judged before any varint
    assert expected_status(rows['gp_20_bytes']) == processor.VERSION_ZERO        # decodeVarint(b'') is (0, 0)
    assert expected_status(rows['gp_v4_last_on_the_edge']) == processor.SEND_V4
    assert expected_status(rows['gp_v3_last_one_above']) == processor.SENT_RECENTLY
    assert expected_status(rows['on_mapped_3_tail_bytes']) == expected_status(rows['on_mapped_5_tail_bytes']) == processor.RAISES
    assert expected_status(rows['on_ends_behind_stream']) == processor.NO_HOST
    for name in ('on_onion_6', 'on_onion_16', 'on_onion_40'):
        assert expected_status(rows[name]) == processor.PEER
    acks = dict(zip(rows, expected_acks(kats)))
    first = list(rows).index('ack_triple_first')
    assert acks['ack_triple_first'][0] == processor.FOUND
    assert acks['ack_triple_second'] == acks['ack_triple_third'] == (processor.FOUND_EARLIER, acks['ack_triple_first'][1], first)
    assert acks['ack_31_byte_object'][0] == processor.NOT_CHECKED and acks['ack_16_byte_tail'][0] == processor.FOUND
    assert acks['ack_on_getpubkey'][0] == processor.FOUND and expected_status(rows['ack_on_getpubkey']) == processor.NOT_MINE
    assert acks['ack_last_byte_c'][0] == processor.NOT_WATCHED


def test_walk_without_addresses_and_with_the_clock():
    data = bytes(20) + b'\x03\x01' + bytes(range(20))
    assert processor.walk(0, data)['status'] == processor.NOT_MINE
    table = processor.address_rows([(3, 1, bytes(range(20)), False, 0)])
    assert processor.walk(0, data, table)['status'] == processor.SEND_V3  # now = 0: the clock, decades past 0
    assert processor.walk(0, data, table, now=2419199)['status'] == processor.SENT_RECENTLY
    assert processor.walk(0, data, table, now=2419200)['status'] == processor.SEND_V3
    assert processor.walk(2, data, table)['route'] == processor.MSG
    assert processor.walk(0x493250, data)['route'] == processor.UNKNOWN_TYPE


def test_walk_refuses_bad_arguments(hostlib):
    out = _lib.BmpowProcRec()
    assert hostlib.bmpow_proc_walk(0, None, 5, 0, None, 0, ctypes.byref(out)) == _lib.E_ARG
    assert hostlib.bmpow_proc_walk(0, b'', 0, 0, None, 0, None) == _lib.E_ARG
    assert hostlib.bmpow_proc_walk(0, b'', 0, 1, None, 0, ctypes.byref(out)) == _lib.E_ARG
    twice = processor.address_rows([(3, 1, bytes(20), False, 0), (4, 1, bytes(20), False, 0)])  # one ripe
    with pytest.raises(_lib.BmpowError) as e:
        processor.walk(0, bytes(42), twice)
    assert e.value.code == _lib.E_ARG


def test_watch_set_host_calls():
    with processor.Dispatcher(seed=5, host_only=True) as d:
        assert len(d) == 0 and not d.watching(b'') and d.stats()['watch_slots'] == 8
        keys = [b'', b'a', b'a' * 16, b'a' * 17, b'a' * 38, b'a' * 37 + b'b', bytes(300)]
        assert d.watch(keys, aux=range(10, 17)).all()
        assert len(d) == 7 and d.stats()['watch_lengths'] == 6 and d.stats()['watch_slots'] == 16
        for i, k in enumerate(keys):
            assert d.watching(k, aux=True) == (True, 10 + i)
        assert not d.watching(b'a' * 15) and not d.watching(b'a' * 37 + b'c') and b'a' * 38 in d
        assert d.watch([b'a', b'new'], aux=[99, 7]).tolist() == [False, True]  # the dict's assignment: the new aux
        assert d.watching(b'a', aux=True) == (True, 99) and len(d) == 8
        assert d.unwatch([b'a' * 38, b'absent', b'a' * 38]).tolist() == [True, False, False]
        assert d.stats()['watch_lengths'] == 7 and d.unwatch([b'a' * 37 + b'b']).all() and d.stats()['watch_lengths'] == 6
        assert len(d) == 6
        d.clear()
        assert len(d) == 0 and d.stats()['watch_lengths'] == 0 and not d.watching(b'')
        # no device behind it: the batch is refused
        with pytest.raises(_lib.BmpowError) as e:
            d.dispatch([bytes(40)], 2)
        assert e.value.code == _lib.E_STATE
    with pytest.raises(ValueError):
        d.watching(b'')


def test_set_addresses_refuses_equal_rows_and_keeps_the_table():
    with processor.Dispatcher(host_only=True) as d:
        good = processor.address_rows([(3, 1, bytes([1]) * 20, False, 0), (4, 1, bytes([2]) * 20, True, 5)])
        d.set_addresses(good)
        assert d.stats()['addresses'] == 2
        for bad in (processor.address_rows([(3, 1, bytes(20), False, 0), (4, 1, bytes(20), False, 0)]),  # one ripe
                    np.concatenate([good, good[:1]])):
            with pytest.raises(_lib.BmpowError) as e:
                d.set_addresses(bad)
            assert e.value.code == _lib.E_ARG
        same_tag = good.copy()
        same_tag['tag'][1] = same_tag['tag'][0]
        with pytest.raises(_lib.BmpowError):
            d.set_addresses(same_tag)
        assert d.stats()['addresses'] == 2 and len(d.address_table) == 2
        d.set_addresses(good[:0])
        assert d.stats()['addresses'] == 0


def test_watch_slot_depends_on_seed_length_and_the_first_16_bytes_only():
    key = bytes(range(40))
    for log2 in (3, 10, 31):
        s = processor.watch_slot(9, log2, key)
        assert 0 <= s < (1 << log2) and s == processor.watch_slot(9, log2, key)
    base = processor.watch_slot(9, 31, key)
    for at in range(16):
        other = bytearray(key)
        other[at] ^= 1
        assert processor.watch_slot(9, 31, bytes(other)) != base, at
    for at in range(16, 40):
        other = bytearray(key)
        other[at] ^= 1
        assert processor.watch_slot(9, 31, bytes(other)) == base, at
    assert processor.watch_slot(9, 31, key[:39]) != base and processor.watch_slot(10, 31, key) != base
    assert processor.watch_slot(9, 31, b'ab') != processor.watch_slot(9, 31, b'ab\x00')  # the length is mixed in
    assert processor.watch_slot(9, 2, key) == 0 and processor.watch_slot(9, 32, key) == 0  # out of range


def test_the_c_list_walk_hands_over_the_objects_where_they_lie():
    """_bmpow_fast.proc_list: pointers into the bytes objects themselves, their lengths, and the caller's
    dispatcher / types / params / records addresses, passed to the entry point whose address it is given."""
    from pybitmessage_amd import verify
    fast = verify._fast()
    assert fast is not None and hasattr(fast, 'proc_list')
    seen = {}
    proto = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p),
                             ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p)

    def entry(d, n, ptrs, lens, types, prm, out):
        seen.update(d=d, n=n, ptrs=[ptrs[i] for i in range(n)], data=[ctypes.string_at(ptrs[i], lens[i]) for i in range(n)],
                    types=types, prm=prm, out=out)
        return -3
    cb = proto(entry)
    addr = ctypes.cast(cb, ctypes.c_void_p).value
    objs = [b'', b'abc', bytes(range(200)), b'x' * 5000]
    assert fast.proc_list(addr, 99, objs, 1234, 5678, 9012) == -3
    assert seen['n'] == 4 and seen['data'] == objs
    assert (seen['d'], seen['types'], seen['prm'], seen['out']) == (99, 1234, 5678, 9012)
    assert seen['ptrs'] == verify._pointers(objs).tolist()
    with pytest.raises(TypeError):
        fast.proc_list(addr, 99, [b'ok', bytearray(3)], 0, 0, 0)
    assert fast.proc_list(addr, 99, [], 0, 0, 0) == -3 and seen['n'] == 0
