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


# ---- items at every byte residue of the upload (the device half is in tests/test_gpu_inv.py) ----

#: the count in front of the probe's two items, and the kind the probe is judged as: (name, count bytes, kind)
RESIDUE_FORMS = (
    ('two', b'\x02', inventory.INV),
    ('announces_256', b'\xfd\x01\x00', inventory.INV),                      # two full items, then the first empty one
    ('announces_65536_inv', b'\xfe\x00\x01\x00\x00', inventory.INV),        # TOO_MANY: none of its items is processed
    ('announces_65536_getdata', b'\xfe\x00\x01\x00\x00', inventory.GETDATA),
    ('announces_2_32_getdata', b'\xff\x00\x00\x00\x01\x00\x00\x00\x00', inventory.GETDATA),  # no bound on a getdata
)
RESIDUE_ITEM_OFFSETS = {1, 3, 5, 9}


def residue_case(r, form, a, b):
    """``(payloads, kinds)`` of one ``check_invs`` call that puts 32-byte items at chosen residues of the upload
    (the payloads go up back to back).  The filler, an ``inv`` of one item ``T == b`` and a pad behind it that is
    not looked at, ends where the probe's first item ``a`` starts at an offset congruent to ``r`` mod 8; the probe,
    ``count + a + b``, is the last payload, so ``b``'s last byte is the upload's last byte and the upload's length
    is congruent to ``r`` too: its last word is partial for r in 1..7.  ``b`` is carried twice, at residue 1 in the
    filler and at residue ``r`` in the probe."""
    _name, count, kind = form
    pad = bytes(0xa0 + i for i in range((r - len(count) - 33) % 8))
    return [b'\x01' + b + pad, count + a + b], [inventory.INV, kind]


def residue_layout(payloads, kinds):
    """``(upload offset of the probe's first item % 8, upload length % 8)``, from the walk and the lengths."""
    filler, probe = payloads
    at = len(filler) + inventory.walk(probe, kinds[1]).item_offset
    return at % 8, (len(filler) + len(probe)) % 8


def residue_expected(form, preloaded):
    """Per packet ``(status, n_items)`` and the item states of a residue case with ``a`` in ``have`` and ``b`` in
    neither set, or (``preloaded``) in ``missing``: the filler's T, then A, B and the first empty item."""
    _name, count, kind = form
    first = inventory.KNOWN if preloaded else inventory.NEW
    if kind == inventory.GETDATA:
        states = [first, inventory.HAVE, inventory.NOT_HAVE, inventory.SHORT]
    elif count == b'\xfe\x00\x01\x00\x00':
        return [(inventory.OK, 1), (inventory.TOO_MANY, 0)], [first]
    else:
        states = [first, inventory.HAVE, inventory.KNOWN if preloaded else inventory.NEW_AGAIN]
        states += [inventory.SHORT] if count != b'\x02' else []
    return [(inventory.OK, 1), (inventory.OK, len(states) - 1)], states


def test_residue_cases_cover_every_residue_and_the_model_judges_them():
    """The construction of the device test ``test_items_at_every_residue_and_the_uploads_last_byte``, checked
    without a device: for every count form the probe's first item meets all eight residues and the upload ends at
    the same residue, the host walk reads the probe as the model's walk does, and the model gives the states the
    construction is meant to provoke."""
    from tests.test_gpu_inv import model_check_invs, py_walk
    assert {len(count) for _, count, _ in RESIDUE_FORMS} == RESIDUE_ITEM_OFFSETS
    a, b = item(90000), item(90001)
    for form in RESIDUE_FORMS:
        seen = set()
        for r in range(8):
            payloads, kinds = residue_case(r, form, a, b)
            at, end = residue_layout(payloads, kinds)
            assert at == end == r, (form[0], r)
            seen.add(at)
            # B twice in one call: at residue 1 in the filler, at residue r in the probe, ending the upload
            assert payloads[0][1:33] == b and payloads[1][-32:] == b and len(payloads[0]) % 8 == (r - len(form[1])) % 8
            for p, k in zip(payloads, kinds):
                got = inventory.walk(p, k)
                status, items = py_walk(p, k, False)
                assert (got.status, got.n_items) == (status, len(items)), (form[0], r)
            for preloaded in (False, True):
                m_missing = {b: 1} if preloaded else {}
                pkts, states, firsts = model_check_invs(payloads, kinds, {a}, m_missing, 1700000000)
                want_pkts, want_states = residue_expected(form, preloaded)
                assert [(s, n) for s, _, n in pkts] == want_pkts and states == want_states, (form[0], r, preloaded)
                again = [j for j, s in enumerate(states) if s == inventory.NEW_AGAIN]
                assert firsts == [0 if j in again else j for j in range(len(states))]
                assert m_missing == {b: 1 if preloaded else 1700000000}
        assert seen == set(range(8)), form[0]


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
