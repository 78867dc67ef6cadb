"""The inventory sets on the GPU (``pybitmessage_amd.inventory``) against a plain dict model written here, and
against the reference-made fixture ``tests/golden/inv_kats.json`` (tests/golden/make_inv_golden.py): the golden
packets through ``check_invs``, items at every byte residue of the upload and on its last byte, constructed probe clusters, equal keys racing inside one call, growth, sweep and
list, ``admit`` behind a real intake and behind ``check_buffers``, and a set's life across a re-selection.
Every malformed input here is a defined status: nothing provokes a fault."""
import hashlib
import random
import struct
import threading

import numpy as np
import pytest

from pybitmessage_amd import _lib, intake, inventory, packets
from pybitmessage_amd.inventory import ABSENT, ADDED, DUP, PRESENT
from tests.golden.make_intake_golden import regen as regen_object
from tests.golden.make_inv_golden import item, regen_payload, runs_to_ids
from tests.test_inv import RESIDUE_FORMS, residue_case, residue_expected, residue_layout

pytestmark = pytest.mark.gpu

KIND = {'inv': inventory.INV, 'dinv': inventory.DINV, 'getdata': inventory.GETDATA}


# ---- the model: the reference's sequential semantics over dicts ----

def py_walk(payload, kind, dandelion):
    """(status, items) as decode_payload_content("l32s") and the handlers' first checks give them."""
    if not payload:
        value, used = 0, 0
    elif payload[0] < 253:
        value, used = payload[0], 1
    else:
        used = {253: 3, 254: 5, 255: 9}[payload[0]]
        if len(payload) < used:
            return inventory.MALFORMED, []
        value = int.from_bytes(payload[1:used], 'big')
        if value < {3: 253, 5: 65536, 9: 1 << 32}[used]:
            return inventory.MALFORMED, []
    count = max(value, 1)
    if kind != inventory.GETDATA:
        if count > inventory.MAX_OBJECT_COUNT:
            return inventory.TOO_MANY, []
        if kind == inventory.DINV and not dandelion:
            return inventory.IGNORED, []
    avail = len(payload) - used
    shown = min(count, (avail + 31) // 32 + 1)  # the full ones, the short one, the first empty one
    return inventory.OK, [payload[used + 32 * k:used + 32 * k + 32] for k in range(shown)]


def model_check_invs(payloads, kinds, have, missing, now, dandelion=False):
    """Per packet (status, first_item, n_items); per item (state, first).  have: dict or set; missing: dict."""
    pkts, states, firsts, first_seen = [], [], [], {}
    for payload, kind in zip(payloads, kinds):
        status, items = py_walk(payload, kind, dandelion)
        pkts.append((status, len(states), len(items)))
        for it in items:
            j = len(states)
            firsts.append(j)
            if len(it) < 32:
                states.append(inventory.SHORT)
            elif it in have:
                states.append(inventory.HAVE)
            elif kind == inventory.GETDATA:
                states.append(inventory.NOT_HAVE)
            elif it in first_seen:
                states.append(inventory.NEW_AGAIN)
                firsts[j] = first_seen[it]
            elif it in missing:
                states.append(inventory.KNOWN)
            else:
                states.append(inventory.NEW)
                first_seen[it] = j
                missing[it] = now
    return pkts, states, firsts


def model_add(model, keys, values):
    state, first, seen = [], [], {}
    for i, k in enumerate(keys):
        if k in seen:
            state.append(DUP), first.append(seen[k])
        elif k in model:
            state.append(PRESENT), first.append(i)
        else:
            state.append(ADDED), first.append(i)
            seen[k] = i
    for k, i in seen.items():
        model[k] = values[i]
    return state, first


def set_keys(s, stream=0, now=0):
    return sorted(bytes(k) for k in s.unexpired_hashes_by_stream(stream, now))


def check_result(res, want):
    pkts, states, firsts = want
    assert [(int(s), int(f), int(n)) for s, f, n in zip(res.status, res.first_item, res.n_items)] == pkts
    assert res.item_state.tolist() == states
    assert res.item_first.tolist() == firsts


@pytest.fixture(scope='module')
def kats(golden):
    return golden('inv_kats.json')


@pytest.fixture(scope='module')
def intake_kats(golden):
    return golden('intake_kats.json')


# ---- 1. the golden cases ----

def test_golden_cases_through_check_invs(gpulib, kats):
    now = 1700000000
    with inventory.InventorySet(64, seed=11) as have, inventory.InventorySet(64, seed=12) as missing:
        for case in kats['cases']:
            have.clear(), missing.clear()
            have0 = [item(k) for k in runs_to_ids(case['have'])]
            missing0 = [item(k) for k in runs_to_ids(case['missing'])]
            if have0:
                have.add(have0, expires=now + 5, stream=1)
            if missing0:
                missing.add(missing0, expires=1)
            payloads = [regen_payload(p) for p in case['packets']]
            kinds = [KIND[p['kind']] for p in case['packets']]
            m_missing = dict.fromkeys(missing0, 1)
            want = model_check_invs(payloads, kinds, set(have0), m_missing, now, case['dandelion'])
            res = inventory.check_invs(payloads, kinds, have, missing, now, dandelion=case['dandelion'])
            check_result(res, want)
            for p, pkt in enumerate(case['packets']):
                if pkt['item_lengths'] is not None:
                    assert int(res.count[p]) == sum(c for _, c in pkt['item_lengths']), case['name']
            # the reference's final missingObjects: its 32-byte keys (a shorter item is never stored here)
            final = sorted([item(k) for k in runs_to_ids(case['missing_final_runs'])] +
                           [bytes.fromhex(h) for h in case['missing_final_other'] if len(h) == 64])
            assert sorted(m_missing) == final, case['name']      # the model restates the reference
            assert set_keys(missing) == final, case['name']      # and the device holds the same
            assert len(missing) == len(final) and len(have) == len(have0)
            for j in np.flatnonzero(res.item_state == inventory.NEW)[:5]:
                assert res.item(int(j)) in m_missing
        big = next(c for c in kats['cases'] if c['name'] == 'inv_50000')
        assert len(runs_to_ids(big['missing_final_runs'])) == 50000 - 107


# ---- 1b. items at every residue of the upload ----

def test_items_at_every_residue_and_the_uploads_last_byte(gpulib):
    """``ivf::load_key`` on the device at every ``off mod 8`` (the aligned branch, the funnel with its fifth word)
    and ``load_word``'s byte-by-byte read of the upload's partial last word, in lookup, claim and finalize: per
    case one ``check_invs`` call of tests/test_inv.py's ``residue_case`` -- A (in ``have``) at residue r, and B
    twice, at residue 1 and at residue r where it ends the upload, so whichever row takes the slot the other
    compares with an input row at another residue.  8 residues x 5 count forms x (B new | B in ``missing``)."""
    now = 1700000000
    layouts = {form[0]: set() for form in RESIDUE_FORMS}
    with inventory.InventorySet(64, seed=41) as have, inventory.InventorySet(64, seed=42) as missing:
        n = 0
        for preloaded in (False, True):
            for form in RESIDUE_FORMS:
                for r in range(8):
                    a, b, n = item(90000 + 2 * n), item(90001 + 2 * n), n + 1
                    payloads, kinds = residue_case(r, form, a, b)
                    at, end = residue_layout(payloads, kinds)
                    assert at == end == r
                    layouts[form[0]].add(at)
                    have.clear(), missing.clear()
                    have.add([a], expires=now + 5, stream=1)
                    m_missing = {}
                    if preloaded:
                        missing.add([b], expires=1)
                        m_missing[b] = 1
                    want = model_check_invs(payloads, kinds, {a}, m_missing, now)
                    want_pkts, want_states = residue_expected(form, preloaded)
                    assert [(s, k) for s, _, k in want[0]] == want_pkts and want[1] == want_states
                    res = inventory.check_invs(payloads, kinds, have, missing, now)
                    where = (form[0], r, preloaded)
                    assert res.status.tolist() == [s for s, _ in want_pkts], where
                    assert res.item_state.tolist() == want[1] and res.item_first.tolist() == want[2], where
                    check_result(res, want)
                    assert [res.item(j) for j in range(len(res))] == ([b, a, b, b''][:len(res)]), where
                    # the key finalize stored is the right 32 bytes, under the value the model holds
                    assert set_keys(missing) == sorted(m_missing) == [b], where
                    found, vals = missing.contains([b, a], values=True)
                    assert found.tolist() == [True, False] and int(vals['expires'][0]) == m_missing[b], where
                    assert m_missing[b] == (1 if preloaded else now)
                    assert set_keys(have, 1) == [a] and len(have) == 1 and len(missing) == 1
                    if kinds[1] == inventory.GETDATA:  # the getdata itself left `missing` alone: T came with the filler
                        alone = inventory.check_invs(payloads[1:], kinds[1:], have, missing, now)
                        assert alone.item_state.tolist() == want[1][1:] and set_keys(missing) == [b], where
                        assert int(missing.contains([b], values=True)[1]['expires'][0]) == m_missing[b]
    assert all(seen == set(range(8)) for seen in layouts.values()), layouts


# ---- 2. constructed clusters ----

def test_constructed_clusters_tombstones_and_equal_tags(gpulib):
    seed, log2 = 0xC0FFEE, 6
    crowd, wrap, k = [], [], 0
    while len(crowd) < 20 or len(wrap) < 5:
        key, k = item(1000 + k), k + 1
        s = inventory.slot_of(seed, log2, key)
        if s == 17 and len(crowd) < 20:
            crowd.append(key)
        elif s == 62 and len(wrap) < 5:
            wrap.append(key)  # 62, 63, 0, 1, 2: the run wraps past the last slot
    # the tag is mixed from the first 16 bytes only: same head, other tails, one start slot
    head, twins, k = item(7)[:16], [], 0
    while len(twins) < 3:
        key, k = head + hashlib.sha256(b'tail%d' % k).digest()[:16], k + 1
        if inventory.slot_of(seed, log2, key) == 40:
            twins.append(key)
    keys = crowd + wrap + twins
    values = {key: (100 + i, i % 3, i) for i, key in enumerate(keys)}

    def check_values(s, present):
        found, vals = s.contains(keys, values=True)
        assert found.tolist() == [key in present for key in keys]
        for i, key in enumerate(keys):
            if key in present:
                assert (int(vals['expires'][i]), int(vals['stream'][i]), int(vals['aux'][i])) == values[key]

    with inventory.InventorySet(64, seed=seed) as s:
        assert s.stats()['slots'] == 64 and s.stats()['seed'] == seed
        state, first = s.add(keys, [v[0] for v in values.values()], [v[1] for v in values.values()],
                             [v[2] for v in values.values()])
        assert state.tolist() == [ADDED] * 28 and first.tolist() == list(range(28))
        st = s.stats()
        assert st['slots'] == 64 and st['rebuilds'] == 0 and st['longest_probe'] >= 20
        check_values(s, set(keys))
        strangers = [item(5000 + i) for i in range(40)]
        assert not s.contains(strangers).any()
        # out of the middle of each cluster; equal rows all say present
        gone = crowd[3:12] + [wrap[1]] + [twins[1]]
        was = s.discard(gone + [crowd[3], strangers[0]])
        assert was.tolist() == [True] * 11 + [True, False]
        assert len(s) == 17 and s.stats()['tombstones'] == 11
        check_values(s, set(keys) - set(gone))  # the rest is found across the tombstones
        assert s.discard(gone).tolist() == [False] * 11 and s.stats()['tombstones'] == 11
        # back in beside the tombstones: live 17 + tombstones 11 + 4 rows = 32 = half the slots, no rebuild
        state, _ = s.add(gone[:4], [values[key][0] for key in gone[:4]], [values[key][1] for key in gone[:4]],
                         [values[key][2] for key in gone[:4]])
        assert state.tolist() == [ADDED] * 4
        st = s.stats()
        assert st['rebuilds'] == 0 and st['tombstones'] == 11 and st['live'] == 21
        check_values(s, set(keys) - set(gone[4:]))
        # the rest: the bound now asks for a purge first
        state, _ = s.add(gone[4:], [values[key][0] for key in gone[4:]], [values[key][1] for key in gone[4:]],
                         [values[key][2] for key in gone[4:]])
        assert state.tolist() == [ADDED] * 7
        st = s.stats()
        assert st['rebuilds'] == 1 and st['tombstones'] == 0 and st['live'] == 28 and st['slots'] == 64
        check_values(s, set(keys))
        state, first = s.add(keys[:5] + [keys[2]])
        assert state.tolist() == [PRESENT] * 6 and first.tolist() == list(range(6))


# ---- 3. races ----

def race_rows(shape, rng):
    if shape == 'three':
        distinct = [item(20000 + k) for k in range(3)]
        rows = [distinct[rng.randrange(3)] for _ in range(8192)]
    else:
        distinct = [item(30000 + k) for k in range(4096)]
        rows = distinct + distinct
        rng.shuffle(rows)
    return distinct, rows


@pytest.mark.parametrize('preload', [False, True], ids=['empty', 'half_held'])
@pytest.mark.parametrize('shape', ['three', 'pairs'])
def test_equal_keys_inside_one_call(gpulib, shape, preload):
    rng = random.Random('%s%s' % (shape, preload))
    distinct, rows = race_rows(shape, rng)
    model = {}
    with inventory.InventorySet(64, seed=rng.getrandbits(63) | 1) as s:
        if preload:
            held = distinct[:max(len(distinct) // 2, 1)]
            s.add(held, expires=7, stream=9, aux=np.arange(len(held)) + 100000)
            model.update((key, (7, 9, 100000 + i)) for i, key in enumerate(held))
        values = [(1000 + i, i % 5, i) for i in range(len(rows))]
        want_state, want_first = model_add(model, rows, values)
        state, first = s.add(rows, [v[0] for v in values], [v[1] for v in values], [v[2] for v in values])
        assert state.tolist() == want_state
        assert first.tolist() == want_first
        assert len(s) == len(model) == len(distinct)
        found, vals = s.contains(distinct, values=True)
        assert found.all()
        got = list(zip(vals['expires'].tolist(), vals['stream'].tolist(), vals['aux'].tolist()))
        assert got == [model[key] for key in distinct]  # the lowest row's value


# ---- 4. growth, sweep, list ----

def test_growth_sweep_and_list(gpulib):
    keys = [item(40000 + k) for k in range(5000)]
    expires = [100 + k for k in range(5000)]
    stream = [k % 3 for k in range(5000)]
    with inventory.InventorySet(16, seed=77) as s:
        assert s.stats()['slots'] == 16
        for a in range(0, 5000, 700):
            state, _ = s.add(keys[a:a + 700], expires[a:a + 700], stream[a:a + 700], list(range(a, min(a + 700, 5000))))
            assert (state == ADDED).all()
        st = s.stats()
        assert len(s) == 5000 and st['slots'] >= 10000 and st['rebuilds'] >= 3
        found, vals = s.contains(keys, values=True)
        assert found.all() and vals['aux'].tolist() == list(range(5000)) and vals['expires'].tolist() == expires
        assert not s.contains([item(50000 + k) for k in range(100)]).any()
        model = {key: (e, t) for key, e, t in zip(keys, expires, stream)}
        for t in range(3):
            want = sorted(key for key, (e, tt) in model.items() if tt == t and e > 3000)
            assert set_keys(s, t, 3000) == want
            some, count = s.unexpired_hashes_by_stream(t, 3000, cap=10)
            assert count == len(want) and len(some) == 10 and {bytes(k) for k in some} <= set(want)
        assert len(s.unexpired_hashes_by_stream(3, 0)) == 0
        left = s.sweep(2600)
        model = {key: v for key, v in model.items() if v[0] >= 2600}
        assert left == len(model) == len(s) == 5000 - 2500
        assert s.contains(keys).tolist() == [key in model for key in keys]
        assert s.clean(2600 + 3 * 3600) == len(model)  # expirestime < now - 3 h: the same bound
        assert s.clean(5100 + 3 * 3600) == 0 and len(s) == 0
        s.add(keys[:10])
        assert len(s) == 10
        s.clear()
        assert len(s) == 0 and not s.contains(keys[:10]).any()


# ---- 5. admit behind a real intake ----

def model_admit(status, invs, have, missing, acceptmismatch=False):
    reach = (intake.OK, intake.INVALID_STREAM, intake.UNWANTED_STREAM, intake.INVALID_FOR_TYPE)
    stored = (intake.OK, intake.INVALID_FOR_TYPE) + ((intake.UNWANTED_STREAM,) if acceptmismatch else ())
    already, state, seen = [], [], set()
    for st, inv in zip(status, invs):
        if st not in reach:
            already.append(False), state.append(ABSENT)
            continue
        already.append(inv in have)
        missing.pop(inv, None)
        if st not in stored:
            state.append(ABSENT)
        elif inv in have:
            state.append(PRESENT)
        elif inv in seen:
            state.append(DUP)
        else:
            state.append(ADDED)
            seen.add(inv)
    have.update(seen)
    return already, state


@pytest.mark.parametrize('acceptmismatch', [False, True])
def test_admit_behind_a_real_intake(gpulib, intake_kats, acceptmismatch):
    groups = {}
    for k in intake_kats['kats']:
        c = k['checks'][0]
        groups.setdefault((c['now'], tuple(c['streams'])), []).append(k)
    announced = [bytes.fromhex(k['fields']['inv']) for k in intake_kats['kats'] if k['fields'] is not None]
    announced = sorted(set(announced)) + [item(60000 + k) for k in range(5)]
    m_have, m_missing, statuses = set(), dict.fromkeys(announced, 1), set()
    with inventory.InventorySet(64, seed=5) as have, inventory.InventorySet(64, seed=6) as missing:
        missing.add(announced, expires=1)
        for pass_ in range(2):
            for (now, streams), group in sorted(groups.items()):
                objs = [regen_object(k) for k in group] * (2 if pass_ == 0 else 1)  # every object twice in one batch
                res = intake.check_objects(objs, streams=streams, now=now)
                invs = [res.inventory_hash(i) for i in range(len(res))]
                statuses.update(res.status.tolist())
                want_already, want_state = model_admit(res.status.tolist(), invs, m_have, m_missing, acceptmismatch)
                got = inventory.admit(res, have, missing, acceptmismatch=acceptmismatch)
                assert got.already.tolist() == want_already
                assert got.state.tolist() == want_state
                if pass_ == 1:  # everything stored is already had
                    assert got.already[got.stored].all() and not (got.state == ADDED).any()
                for i in got.added():
                    found, vals = have.contains([invs[i]], values=True)
                    assert found[0] and int(vals['expires'][0]) == int(res.expiresTime[i]) and int(vals['aux'][0]) == i
            assert len(have) == len(m_have) and set_keys(missing) == sorted(m_missing)
        assert len(m_have) > 3 and len(m_missing) >= 5 and len(m_missing) < len(announced)
        assert {intake.OK, intake.INSUFFICIENT_POW, intake.INVALID_STREAM, intake.UNWANTED_STREAM,
                intake.INVALID_FOR_TYPE} <= statuses


# ---- 6. through packets ----

def packet(command, payload):
    return struct.pack('!L12sL4s', 0xE9BEB4D9, command, len(payload), hashlib.sha512(payload).digest()[:4]) + payload


def inv_payload(hashes, cut=None):
    n = len(hashes)
    head = bytes([n]) if n < 253 else b'\xfd' + struct.pack('>H', n)
    data = head + b''.join(hashes)
    return data if cut is None else data[:cut]


def test_inv_and_object_packets_through_check_buffers(gpulib, intake_kats):
    now = intake_kats['now']
    by_name = {k['name']: regen_object(k) for k in intake_kats['kats']}
    objs = [by_name[n] for n in ('msg_ok', 'pubkey_ok', 'broadcast_ok')]
    obj_inv = [hashlib.sha512(hashlib.sha512(o).digest()).digest()[:32] for o in objs]
    fresh = [item(70000 + k) for k in range(300)]
    bufs = [
        packet(b'inv', inv_payload(obj_inv + fresh[:100])) + packet(b'object', objs[0]) + packet(b'ping', b'x' * 5) +
        packet(b'getdata', inv_payload(fresh[:4] + obj_inv[:1])),
        packet(b'object', objs[1]) + packet(b'inv', inv_payload(fresh[50:300])) + packet(b'dinv', inv_payload(fresh[:9])) +
        packet(b'inv', inv_payload(fresh[:3], cut=1 + 70)) + packet(b'object', objs[0]),
        packet(b'INV', inv_payload([fresh[299], item(1)])) + packet(b'object', objs[2]),
    ]
    res = packets.check_buffers(bufs, now=now)
    assert (res.status == packets.OK).all() and len(res) == 11
    with inventory.InventorySet(64, seed=21) as have, inventory.InventorySet(64, seed=22) as missing:
        have.add([obj_inv[1]], expires=now + 9, stream=1)
        m_have, m_missing = {obj_inv[1]}, {}
        for round_ in range(2):
            names = [res.command_name(i).lower().decode() for i in range(len(res))]
            rows = [i for i, nm in enumerate(names) if nm in ('inv', 'dinv', 'getdata')]
            got = inventory.check_invs(res, None, have, missing, now)
            assert got.packet_index.tolist() == rows
            want = model_check_invs([res.payload(i) for i in rows], [KIND[names[i]] for i in rows], m_have, m_missing, now)
            check_result(got, want)
            if round_ == 0:
                assert got.item(0) == obj_inv[0] and got.item(3) == fresh[0] and got.item(len(got) - 1) == item(1)
                short = np.flatnonzero(got.item_state == inventory.SHORT)
                assert [got.item(int(j)) for j in short] == [fresh[2][:6]]
                assert sorted(got.item(int(j)) for j in got.new_items()) == sorted(m_missing)
            assert set_keys(missing) == sorted(m_missing)
            adm = inventory.admit(res, have, missing)
            recs = res.intake
            invs = [recs.inventory_hash(i) for i in range(len(res))]
            # a packet of another command carries a zeroed record and takes no part: MALFORMED in the model
            status = [int(recs.status[i]) if names[i] == 'object' else intake.MALFORMED for i in range(len(res))]
            want_already, want_state = model_admit(status, invs, m_have, m_missing)
            assert adm.already.tolist() == want_already and adm.state.tolist() == want_state
            obj_rows = [i for i, nm in enumerate(names) if nm == 'object']
            if round_ == 0:
                assert [want_state[i] for i in obj_rows] == [ADDED, PRESENT, DUP, ADDED]
                assert len(have) == 3 and bytes(32) not in have
            assert have.contains(obj_inv).all() and not missing.contains(obj_inv).any()


# ---- 7. lifecycle ----

def test_a_set_across_other_calls_threads_and_a_reselection(gpulib):
    keys = [item(80000 + k) for k in range(2000)]
    a, b = inventory.InventorySet(64, seed=31), inventory.InventorySet(64, seed=32)
    a.add(keys[:100], expires=5)
    objs = [bytes(8) + b'x' * n for n in (8, 120, 1000)]
    assert intake.inventory_hashes(objs) == [hashlib.sha512(hashlib.sha512(o).digest()).digest()[:32] for o in objs]
    assert a.contains(keys[:200]).tolist() == [True] * 100 + [False] * 100
    errors = []

    def work(s, mine):
        try:
            model = {}
            for r in range(6):
                part = mine[r * 150:r * 150 + 200]  # overlaps the previous part by 50
                want, _ = model_add(model, part, [None] * len(part))
                state, _ = s.add(part)
                assert state.tolist() == want
                assert s.contains(mine).tolist() == [key in model for key in mine]
            assert len(s) == len(model)
        except Exception as e:  # noqa: BLE001 -- reported by the main thread
            errors.append(e)

    a.clear()
    threads = [threading.Thread(target=work, args=(a, keys[:1000])), threading.Thread(target=work, args=(b, keys[1000:]))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    _lib.reset()
    _lib.get()
    try:
        for call in (lambda: len(a), lambda: a.add(keys[:3]), lambda: a.contains(keys[:3]), lambda: a.discard(keys[:3]),
                     lambda: a.sweep(0), lambda: a.unexpired_hashes_by_stream(0, 0, cap=4), a.clear, a.stats,
                     lambda: inventory.check_invs([inv_payload(keys[:2])], inventory.INV, a, b, 1)):
            with pytest.raises(_lib.BmpowError) as err:
                call()
            assert err.value.code == _lib.E_STATE
    finally:
        a.close(), b.close()
    a.close()  # twice is fine
    with inventory.InventorySet(64, seed=33) as c:  # and a set of the new selection works
        assert c.add(keys[:3])[0].tolist() == [ADDED] * 3 and len(c) == 3
