"""The inventory sets, the parts that need no device: the ABI table of ``include/bmpow_inv.h``, the struct
layouts, ``bmpow_inv_walk`` against the reference-made fixture ``tests/golden/inv_kats.json``
(tests/golden/make_inv_golden.py), ``bmpow_invset_slot``, and the store mask of ``inventory.admit``."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from pybitmessage_amd import _lib, intake, inventory
from tests.conftest import ROOT
from tests.golden.make_inv_golden import item, regen_payload

HEADER = os.path.join(ROOT, 'include', 'bmpow_inv.h')
KIND = {'inv': inventory.INV, 'dinv': inventory.DINV, 'getdata': inventory.GETDATA}


@pytest.fixture(scope='module')
def kats(golden):
    return golden('inv_kats.json')


@pytest.fixture(scope='module')
def hostlib():
    return _lib.load()


def declared_symbols():
    text = open(HEADER).read()
    return sorted(set(re.findall(r'BMPOW_API\s+[\w\s\*]+?\b(\w+)\s*\(', text)))


def test_every_declared_symbol_is_exported_and_bound(hostlib):
    syms = declared_symbols()
    assert 'bmpow_inv_batch' in syms and 'bmpow_invset_add' in syms and len(syms) == 14
    assert syms == sorted(name for name, _, _ in _lib.INV_SIGNATURES)
    raw = ctypes.CDLL(_lib.lib_path())
    for name, res, args in _lib.INV_SIGNATURES:
        assert hasattr(raw, name), name
        fn = getattr(hostlib, name)
        assert fn.restype == res and list(fn.argtypes) == args, name
    # the other headers' tables keep their own sets
    assert not set(syms) & set(name for name, _, _ in _lib.SIGNATURES + _lib.INTAKE_SIGNATURES + _lib.PACKETS_SIGNATURES)


@pytest.mark.parametrize('ctype,cls', [('bmpow_inv_value', _lib.BmpowInvValue), ('bmpow_inv_pkt', _lib.BmpowInvPkt),
                                       ('bmpow_inv_stats', _lib.BmpowInvStats)])
def test_structs_match_the_header(tmp_path, ctype, cls):
    fields = [f for f, _ in cls._fields_]
    src = tmp_path / 'sz.c'
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "bmpow_inv.h"\nint main(void) {\n'
                   '  printf("%%zu", sizeof(%s));\n' % ctype +
                   ''.join('  printf(" %%zu", offsetof(%s, %s));\n' % (ctype, f) for f in fields) +
                   '  return 0;\n}\n')
    exe = tmp_path / 'sz'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got[0] == ctypes.sizeof(cls)
    assert got[1:] == [getattr(cls, f).offset for f in fields]
    for dtype, owner in ((inventory.VALUE_DTYPE, _lib.BmpowInvValue), (inventory.PKT_DTYPE, _lib.BmpowInvPkt)):
        if cls is owner:  # the numpy views the Python layer hands out
            assert dtype.itemsize == got[0] and [dtype.fields[f][1] for f in fields] == got[1:]


def expected_status(case, pkt):
    """The walk's status from what the reference did: the exception it raised; a dinv it returned from without
    touching missingObjects while dandelion was off."""
    if pkt['exception'] == 'varintDecodeError':
        return inventory.MALFORMED
    if pkt['exception'] == 'BMProtoExcessiveDataError':
        return inventory.TOO_MANY
    assert pkt['exception'] is None
    if pkt['kind'] == 'dinv' and not case['dandelion']:
        return inventory.IGNORED
    return inventory.OK


def test_walk_against_every_golden_case(kats):
    assert kats['max_object_count'] == inventory.MAX_OBJECT_COUNT
    seen = set()
    for case in kats['cases']:
        for pkt in case['packets']:
            payload = regen_payload(pkt)
            assert len(payload) == pkt['len'], case['name']
            got = inventory.walk(payload, KIND[pkt['kind']], case['dandelion'])
            want = expected_status(case, pkt)
            seen.add(want)
            assert got.status == want, (case['name'], got.status)
            if pkt['item_lengths'] is None:
                assert got.count == 0 and got.n_items == 0
                continue
            lengths = [n for n, c in pkt['item_lengths'] for _ in range(c)]
            assert got.count == len(lengths), case['name']
            if want != inventory.OK:
                assert got.n_items == 0
                continue
            cut = [max(0, min(32, len(payload) - got.item_offset - 32 * k)) for k in range(got.n_items)]
            assert cut == lengths[:got.n_items], case['name']
            # what the walk leaves out: empty items behind the payload's end, all but the first
            assert not any(lengths[got.n_items:]) and (got.n_items == len(lengths) or lengths[got.n_items - 1] == 0)
    assert seen == {inventory.OK, inventory.MALFORMED, inventory.TOO_MANY, inventory.IGNORED}


def test_dinv_with_dandelion_off_leaves_missing_alone(kats):
    """What ``IGNORED`` stands for, from the fixture itself."""
    case = next(c for c in kats['cases'] if c['name'] == 'dinv_dandelion_off')
    assert case['missing_final_runs'] == [] and case['missing_final_other'] == []
    case = next(c for c in kats['cases'] if c['name'] == 'dinv_dandelion_on')
    assert case['missing_final_runs'] == [[1, 1], [3, 3]]


def test_walk_refuses_bad_arguments(hostlib):
    out = _lib.BmpowInvPkt()
    assert hostlib.bmpow_inv_walk(None, 0, 3, 0, ctypes.byref(out)) == _lib.E_ARG
    assert hostlib.bmpow_inv_walk(None, 5, 0, 0, ctypes.byref(out)) == _lib.E_ARG
    assert hostlib.bmpow_inv_walk(None, 0, 0, 0, None) == _lib.E_ARG
    assert hostlib.bmpow_inv_walk(None, 0, 0, 0, ctypes.byref(out)) == 0 and (out.count, out.n_items) == (1, 1)


def test_slot_is_stable_under_a_seed_and_differs_across_seeds():
    keys = [item(k) for k in range(64)]
    for log2 in (1, 6, 16, 30):
        a = [inventory.slot_of(1234, log2, k) for k in keys]
        assert a == [inventory.slot_of(1234, log2, k) for k in keys]
        assert all(0 <= s < (1 << log2) for s in a)
    a = [inventory.slot_of(1234, 16, k) for k in keys]
    b = [inventory.slot_of(1235, 16, k) for k in keys]
    assert sum(x == y for x, y in zip(a, b)) <= 2  # 64 draws from 2^16 slots
    assert len(set(a)) >= 60
    # every byte of the key reaches the slot
    base = bytearray(keys[0])
    for at in range(32):
        other = bytearray(base)
        other[at] ^= 1
        assert inventory.slot_of(7, 30, bytes(other)) != inventory.slot_of(7, 30, bytes(base)), at
    assert inventory.slot_of(7, 0, keys[0]) == 0 and inventory.slot_of(7, 31, keys[0]) == 0  # out of range


#: bm_command_object behind checkAlreadyHave (src/network/bmproto.py:401-435), status by status: is
#: ``Inventory()[hash] = ...`` (:431) reached?  (without acceptmismatch, with it)
STORE_TABLE = {
    intake.OK: (True, True),                  # :414-417 no exception
    intake.MALFORMED: (False, False),         # :380-381 decode_payload_content raises
    intake.TOO_LARGE: (False, False),         # :387-391 raise
    intake.INSUFFICIENT_POW: (False, False),  # :393-400 raise
    intake.EXPIRED_FUTURE: (False, False),    # :393-400 raise
    intake.EXPIRED_PAST: (False, False),      # :393-400 raise
    intake.INVALID_STREAM: (False, False),    # :410-412 BMObjectInvalidError: raise
    intake.UNWANTED_STREAM: (False, True),    # :403-409 raise unless acceptmismatch
    intake.INVALID_FOR_TYPE: (True, True),    # :418-419 caught, goes on to :431
}


def test_store_mask_restates_the_reference():
    assert sorted(STORE_TABLE) == sorted(intake.STATUS_NAMES)
    status = np.array(sorted(STORE_TABLE), dtype=np.int32)
    assert list(inventory.store_mask(status)) == [STORE_TABLE[s][0] for s in status]
    assert list(inventory.store_mask(status, acceptmismatch=True)) == [STORE_TABLE[s][1] for s in status]
