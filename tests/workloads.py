"""Small exact workloads, one per entry point of the library, for the tests that run the entry points
together (tests/test_gpu_together.py, the soak, the lifecycle test).  Not a test module and not a conftest.

A workload has a name and three parts: ``run()`` makes the library call(s) on inputs built from the committed
fixtures (tens to a few hundred rows: a call alone takes milliseconds); ``check(result)`` holds the result
against the fixture's own expectation, row by row, with the checkers of the per-subsystem GPU tests --
imported, never copied -- or, where that test compares with the fixture directly, by the same comparison;
``canon(result)`` is the result's canonical bytes.  Calling the workload gives ``canon(run())``.

``baseline()`` runs every workload once with the engine idle, checks it, and keeps its canonical bytes; every
later comparison -- beside a busy service, after an abort, under another shard layout -- is byte equality
with that.  The chain is fixture -> existing checker -> baseline bytes -> equality; nothing here invents an
expectation.  No workload reads a ``*_stats()`` delta: the counters are process-wide and mean nothing while
other threads call the library.  A workload that needs an object bound to the device selection (an
``InventorySet``, a ``Dispatcher``) makes it inside ``run()`` in a ``with`` block and never keeps it: the
workloads run across re-selections and under an abort that may land between two of their calls.  Beside a
busy service every library call waits for the lock, so a workload makes few of them.
"""
import hashlib
import itertools
import random
import threading

import numpy as np

from tests.conftest import load_golden

U64 = (1 << 64) - 1


def _plain(fixture):
    """The function under a pytest fixture (the GPU tests keep their shared inputs in module fixtures)."""
    return getattr(fixture, '__wrapped__', fixture)


def _canon(x):
    """Canonical bytes of a result made of bytes, numbers, None, sequences and numpy arrays."""
    if x is None:
        return b'N'
    if isinstance(x, (bytes, bytearray)):
        return b'B%d:' % len(x) + bytes(x)
    if isinstance(x, np.ndarray):
        return b'A' + _canon(np.ascontiguousarray(x).tobytes())
    if isinstance(x, (bool, int, np.integer)):
        return b'I%d;' % int(x)
    if isinstance(x, str):
        return b'S' + _canon(x.encode())
    if isinstance(x, (list, tuple)):
        return b'L%d[' % len(x) + b''.join(_canon(y) for y in x) + b']'
    raise TypeError('no canonical form for %r' % type(x))


class Workload(object):
    def __init__(self, name, run, check, canon):
        self.name, self.run, self.check, self.canon = name, run, check, canon

    def __call__(self):
        return self.canon(self.run())


# ------------------------------------------------------------------ intake
def _intake():
    from pybitmessage_amd import intake
    from tests import test_gpu_intake as t
    kats = load_golden('intake_kats.json')
    groups = {}
    for k in kats['kats']:
        for c in k['checks']:
            groups.setdefault((c['now'], tuple(c['streams'])), []).append(k)
    calls = [(now, streams, [t.regen(k) for k in items]) for (now, streams), items in groups.items()]
    hashed = [t.regen(k) for k in kats['kats'] if k['L'] >= 8]

    def run():
        return ([intake.check_objects(objs, streams=streams, now=now) for now, streams, objs in calls],
                intake.inventory_hashes(hashed))

    def canon(res):
        return _canon([r.records for r in res[0]] + [res[1]])

    def check(res):
        # test_check_objects_reproduces_the_fixture is the checker: it makes these very calls, so it is run
        # with check_objects recording what it returned, and what it accepted row by row must be these bytes
        seen, real = [], intake.check_objects

        def recording(*a, **kw):
            seen.append(real(*a, **kw))
            return seen[-1]
        intake.check_objects = recording
        try:
            t.test_check_objects_reproduces_the_fixture(None, kats)
        finally:
            intake.check_objects = real
        assert len(seen) == len(calls)
        assert _canon([r.records for r in seen]) == _canon([r.records for r in res[0]])
        assert res[1] == [t.inv_hash(o) for o in hashed]
    return Workload('intake', run, check, canon)


# ------------------------------------------------------------------ verify
def _verify():
    from pybitmessage_amd import targets, verify
    from tests.golden.make_intake_golden import regen
    kats = load_golden('intake_kats.json')
    now = kats['now']
    rng = random.Random(512)
    objs = [rng.randbytes(8) + (now + rng.randint(-3600, 30000)).to_bytes(8, 'big') + rng.randbytes(rng.randint(6, 1000))
            for _ in range(512)]
    # ... and the intake fixture's objects among them: those carry nonces that satisfy the network's difficulty
    objs += [o for o in (regen(k) for k in kats['kats'] if k['fields'] is not None) if len(o) <= 1 << 18]
    rng.shuffle(objs)

    def run():
        return verify.pow_values(objs), verify.isProofOfWorkSufficient_batch(objs, 0, 0, now)

    def check(res):
        assert res[0] == [targets.pow_value(o) for o in objs]
        assert res[1] == [targets.isProofOfWorkSufficient(o, 0, 0, now) for o in objs]
        assert 0 < sum(res[1]) < len(objs)
    return Workload('verify', run, check, lambda res: _canon([res[0], [bool(v) for v in res[1]]]))


# ------------------------------------------------------------------ sig
def _sig():
    from oracle import ecdsa_oracle as eo
    from pybitmessage_amd import signatures
    from tests import test_gpu_sig as t, test_gpu_sig_constructed as tc
    triples = _plain(t.triples)(load_golden('sig_kats.json'))
    comb = list(itertools.islice(eo.comb_cases(), 130))
    rows = tc.digest_rows([c.case for c in comb])

    def run():
        return t.run(triples), signatures.ecdsa_verify_digest(*rows)

    def check(res):
        assert not t.mismatches(triples, res[0])
        assert sorted(set(res[0])) == [0, 1, 2]
        assert not tc.wrong(comb, res[1])
        assert len(set(res[1])) == 2
    return Workload('sig', run, check, lambda res: _canon([list(res[0]), [bool(v) for v in res[1]]]))


# ------------------------------------------------------------------ ecies
def _ecies():
    from pybitmessage_amd import ecies
    ek = load_golden('ecies_kats.json')
    verdicts = ek['verdict_kats']
    rows = [verdicts[i % len(verdicts)] for i in range(130)]
    blobs = [bytes.fromhex(v['blob']) for v in rows]
    keys = [(7).to_bytes(32, 'big'), bytes.fromhex(ek['verdict_key'])]

    def check(got):  # tests/test_gpu_seal.py test_verdict_kats_repeated_in_one_decrypt_batch, its comparison
        assert len(got) == len(rows)
        for v, g in zip(rows, got):
            assert g == ((1, bytes.fromhex(v['plaintext'])) if v['outcome'] == 'decrypted' else None), v['name']
        assert any(g is None for g in got) and any(g is not None for g in got)
    return Workload('ecies', lambda: ecies.decrypt_batch(blobs, keys), check,
                    lambda got: _canon([None if g is None else list(g) for g in got]))


# ------------------------------------------------------------------ ident
def _ident():
    from pybitmessage_amd import addresses
    from tests import test_gpu_ident as t
    keyrows = _plain(t.keyrows)(load_golden('ident_kats.json'))
    versions = [(2, 3, 4, 1, 5)[i % 5] for i in range(len(keyrows))]
    streams = [(1, 2, 300, 70000, 2 ** 40)[i % 5] for i in range(len(keyrows))]
    pub_s, pub_e = [k[0] for k in keyrows], [k[1] for k in keyrows]
    return Workload('ident', lambda: addresses.derive_batch(pub_s, pub_e, versions, streams),
                    lambda res: t.check(res, [(v, s, k[2]) for v, s, k in zip(versions, streams, keyrows)]),
                    lambda res: _canon(res.recs))


# ------------------------------------------------------------------ the receive side
def _rx():
    from pybitmessage_amd import receive
    from tests import test_gpu_rxopen as t
    msgs = [m for m in load_golden('rx_kats.json')['msgs'] if m['line'] != 478]
    args = ([bytes.fromhex(m['obj']) for m in msgs], [bytes.fromhex(m['plaintext']) for m in msgs],
            [bytes.fromhex(m['toRipe']) for m in msgs])

    def check(res):
        assert len(res) == len(msgs)
        for i, m in enumerate(msgs):
            t.check_msg_result(m, res, i)  # check_row_against_fixture, the digest and the result
        assert res.accepted() == [i for i, m in enumerate(msgs) if m['line'] is None]
    return Workload('rx', lambda: receive.open_msgs(*args), check, lambda res: _canon(res.recs))


def _rxobj():
    from pybitmessage_amd import receive
    from tests.test_rxobj import BROADCAST, check_row_against_fixture, device_rows
    rows = device_rows(load_golden('rxobj_kats.json'))
    args = ([r[0] for r in rows], [r[2] for r in rows], [r[3] for r in rows], [r[4] for r in rows])

    def check(res):  # as tests/test_gpu_rxobj.py test_both_fixtures_in_one_call holds its own fixture's rows
        assert len(res) == len(rows)
        for i, (kind, e, _obj, _plain_, _expect) in enumerate(rows):
            check_row_against_fixture(kind, e, res, i, final=True)
            assert int(res.recs[i]['digest']) == e['digest'], e['name']
            if e['result'] is not None:
                assert (res.fromAddress(i), res.ripe(i).hex()) == (e['result']['fromAddress'], e['result']['ripe']), e['name']
                if kind == BROADCAST:
                    assert res.sigHash(i).hex() == e['result']['sigHash'], e['name']
                else:
                    assert res.storedData(i).hex() == e['result']['storedData'], e['name']
        assert any(e['result'] is not None for _k, e, _o, _p, _x in rows)
    return Workload('rxobj', lambda: receive.open_objects(*args), check, lambda res: _canon(res.recs))


def _rxsealed():
    from pybitmessage_amd import receive
    from tests import test_gpu_rxopen as t
    kats = load_golden('rx_kats.json')
    keys = {bytes.fromhex(k['ripe']): bytes.fromhex(k['privkey']) for k in kats['recipients']}
    objs = [bytes.fromhex(m['obj']) for m in kats['msgs']]

    def check(res):
        assert len(res) == len(objs)
        for i, m in enumerate(kats['msgs']):
            t.check_sealed_row(m, res, i)
        assert res.accepted() == [i for i, m in enumerate(kats['msgs']) if m['line'] is None]
    return Workload('rxsealed', lambda: receive.open_sealed_msgs(objs, keys), check,
                    lambda res: _canon([res.recs, np.asarray(res.match), list(res.plaintexts)]))


# ------------------------------------------------------------------ the send side
def _send():
    from pybitmessage_amd import sender
    kats = load_golden('send_kats.json')
    pubs = [bytes.fromhex(k) for k in kats['recipient_pubs']]
    signs = [[k for k in kats['sign_kats'] if k['digest'] == alg] for alg in ('sha1', 'sha256')]
    enc = kats['encrypt_kats']
    points = kats['pointmult_kats']

    def run():
        sigs = [sender.sign_batch([bytes.fromhex(k['msg']) for k in rows], [bytes.fromhex(k['priv']) for k in rows], alg,
                                  nonces=[bytes.fromhex(k['nonce']) for k in rows])
                for alg, rows in zip(('sha1', 'sha256'), signs)]
        blobs = sender.encrypt_batch([bytes.fromhex(k['plaintext']) for k in enc], [pubs[k['recipient']] for k in enc],
                                     ephemeral=[bytes.fromhex(k['ephemeral']) for k in enc],
                                     ivs=[bytes.fromhex(k['iv']) for k in enc])
        return sigs, blobs, sender.priv_to_pub([bytes.fromhex(k['priv']) for k in points])

    def check(res):  # the comparisons of tests/test_gpu_send.py and test_gpu_seal.py with send_kats.json
        for rows, got in zip(signs, res[0]):
            assert len(rows) >= 14 and got == [bytes.fromhex(k['sig']) for k in rows]
        assert res[1] == [bytes.fromhex(k['blob']) for k in enc]
        assert res[2] == [bytes.fromhex(k['pub']) for k in points]
    return Workload('send', run, check, lambda res: _canon([res[0], res[1], res[2]]))


def _tx():
    from pybitmessage_amd import outgoing, sender
    kats = load_golden('tx_kats.json')['objects']
    by_alg = [(alg, [k for k in kats if k['digest'] == alg]) for alg in ('sha1', 'sha256')]

    def build(alg, rows):
        sealed = [k['kind'] == 'sealed' for k in rows]
        return outgoing.build_objects(
            [outgoing.SEALED if s else outgoing.CLEAR for s in sealed], [bytes.fromhex(k['head']) for k in rows],
            [bytes.fromhex(k['body']) for k in rows], [bytes.fromhex(k['priv']) for k in rows],
            [bytes.fromhex(k['recipient_pub']) if s else None for k, s in zip(rows, sealed)], alg,
            nonces=[bytes.fromhex(k['nonce']) for k in rows],
            ephemeral=[bytes.fromhex(k['ephemeral']) if s else None for k, s in zip(rows, sealed)],
            ivs=[bytes.fromhex(k['iv']) if s else None for k, s in zip(rows, sealed)])

    def check(res):  # the comparisons of tests/test_gpu_tx.py test_reference_fixture_bit_for_bit
        for (alg, rows), built in zip(by_alg, res):
            assert rows and built.accepted() == list(range(len(rows)))
            for i, k in enumerate(rows):
                assert built.payload(i).hex() == k['payload'], k['name']
                assert built.initial_hash(i).hex() == k['initial_hash'], k['name']
                assert built.signature(i).hex() == k['signature'], k['name']
                assert built.recs[i]['digest'] == sender.DIGESTS[alg] and built.recs[i]['kind'] == (k['kind'] != 'sealed')
    return Workload('tx', lambda: [build(alg, rows) for alg, rows in by_alg], check,
                    lambda res: _canon([[b.recs, [b.payload(i) for i in range(len(b))]] for b in res]))


# ------------------------------------------------------------------ addr
def _addr():
    from pybitmessage_amd import addressgen
    from tests.test_addressgen import SAMPLE_DET_RIPE, SAMPLE_SEED
    points = load_golden('addr_kats.json')['pointmult_kats']
    privs = [bytes.fromhex(k['priv']) for k in points]

    def run():
        g = addressgen.deterministic_addresses(SAMPLE_SEED, 1, 1)[0]  # one null byte: the 16-bit comb table
        return [g['k'], g['ripe'], g['address'], g['pubSigningKey'], g['pubEncryptionKey']], addressgen.pubkeys(privs)

    def check(res):
        assert (res[0][0], res[0][1].hex()) == (21, SAMPLE_DET_RIPE)
        assert [p.hex() for p in res[1]] == [k['pub'] for k in points]
    return Workload('addr', run, check, lambda res: _canon([res[0], res[1]]))


# ------------------------------------------------------------------ aes
def _aes():
    from pybitmessage_amd import ecies
    from tests import test_gpu_seal as t
    published = [(t.C3_KEY, bytes(16), t.C3_PLAIN, None), (t.F25_KEY, t.F25_IV, t.F25_PLAIN, t.F25_CIPHER)]
    rows = published + _plain(t.raw_cases)()  # (key, iv, plaintext, libcrypto's ciphertext) per length
    keys, ivs, plains = [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]

    def run():
        enc = ecies.aes_cbc_batch(keys, ivs, plains)
        return enc, ecies.aes_cbc_batch(keys, ivs, enc, decrypt=True)

    def check(res):
        enc, dec = res
        assert enc[0][:16] == t.C3_CIPHER and len(enc[0]) == 32  # the published block, then the padding block
        assert enc[1:] == [r[3] for r in rows[1:]]
        assert dec == plains
    return Workload('aes', run, check, lambda res: _canon([res[0], res[1]]))


# ------------------------------------------------------------------ the network side
def _packets():
    from pybitmessage_amd import packets
    from tests import test_gpu_packets as t
    kats = load_golden('packet_kats.json')
    intake_objects = _plain(t.intake_objects)(load_golden)
    groups = {}
    for case in kats['connections']:
        groups.setdefault((case['now'], tuple(case['streams'])), []).append(case)
    calls = [(now, streams, [t.regen_buffer(c, intake_objects) for c in cases], [c['established'] for c in cases],
              [c['datagram'] for c in cases]) for (now, streams), cases in groups.items()]
    acks = [t.regen_buffer(a, intake_objects) for a in kats['acks']]

    def run():
        framed = [packets.check_buffers(bufs, established, datagram, streams=streams, now=now)
                  for now, streams, bufs, established, datagram in calls]
        return framed, packets.check_acks(acks, now=t.NOW)

    def canon(res):
        framed, (valid, recs) = res
        return _canon([[r.records, r.consumed, r.close] for r in framed] + [valid, recs.records])

    def check(res):
        # test_the_fixture_is_reproduced_record_for_record and test_check_acks_agrees_... are the checkers: they
        # make these very calls (and one buffer alone, and the acks once more through receive.check_opened_acks),
        # so they run with both entry points recording what they returned, and what they accepted is these bytes
        seen, seen_acks, real, real_acks = [], [], packets.check_buffers, packets.check_acks

        def recording(*a, **kw):
            seen.append(real(*a, **kw))
            return seen[-1]

        def recording_acks(*a, **kw):
            seen_acks.append(real_acks(*a, **kw))
            return seen_acks[-1]
        packets.check_buffers, packets.check_acks = recording, recording_acks
        try:
            t.test_the_fixture_is_reproduced_record_for_record(None, kats, intake_objects)
            t.test_check_acks_agrees_with_the_host_check_on_every_fixture_ack(None, kats, intake_objects)
        finally:
            packets.check_buffers, packets.check_acks = real, real_acks
        assert len(seen) == len(calls) + 1 and len(seen_acks) == 2
        assert canon((seen[:len(calls)], seen_acks[0])) == canon(res)
    return Workload('packets', run, check, canon)


def _set_keys(s, streams, cap):
    """The set's keys of the given streams (at most ``cap`` of each) as one (m, 32) array in byte order: one
    library call per stream."""
    keys = np.concatenate([s.unexpired_hashes_by_stream(stream, 0, cap=cap)[0] for stream in streams])
    words = np.ascontiguousarray(keys).view('>u8').reshape(-1, 4)
    return keys[np.lexsort((words[:, 3], words[:, 2], words[:, 1], words[:, 0]))]


def _inv():
    from pybitmessage_amd import intake, inventory
    from tests import test_gpu_inv as t
    kats = load_golden('inv_kats.json')
    intake_kats = load_golden('intake_kats.json')
    now = 1700000000
    # Every golden case's packets, in the fixture's order, as one check_invs call per dandelion setting (the flag
    # is the call's) against the union of the cases' initial sets: beside a busy service every library call waits
    # for the lock, so a call per case -- and the two clears, two adds and two lists around it -- is what
    # tests/test_gpu_inv.py does once, not what a workload repeats.  The cases then meet inside a call (one case's
    # announcement is another's NEW_AGAIN), which the model follows.
    cases = kats['cases']
    flood = []
    for dandelion in (False, True):
        mine = [c for c in cases if c['dandelion'] == dandelion]
        pkts = [p for c in mine for p in c['packets']]
        flood.append((dandelion, sorted(set(t.item(k) for c in mine for k in t.runs_to_ids(c['have']))),
                      sorted(set(t.item(k) for c in mine for k in t.runs_to_ids(c['missing']))),
                      [t.regen_payload(p) for p in pkts], [t.KIND[p['kind']] for p in pkts]))
    most = sum(len(p) // 32 + 1 for f in flood for p in f[3]) + sum(len(f[2]) for f in flood)
    # the groups, the doubled batches and the announced hashes of test_admit_behind_a_real_intake
    groups = {}
    for k in intake_kats['kats']:
        c = k['checks'][0]
        groups.setdefault((c['now'], tuple(c['streams'])), []).append(k)
    groups = [(key, [t.regen_object(k) for k in group] * 2) for key, group in sorted(groups.items())]
    announced = sorted(set(bytes.fromhex(k['fields']['inv']) for k in intake_kats['kats'] if k['fields'] is not None))
    announced += [t.item(60000 + k) for k in range(5)]
    stored_streams = sorted(set(min(s, 0xffffffff) for (_, streams), _ in groups for s in streams))

    def run():
        judged, admitted = [], []
        with inventory.InventorySet(64, seed=11) as have, inventory.InventorySet(64, seed=12) as missing:
            for dandelion, have0, missing0, payloads, kinds in flood:
                have.add(have0, expires=now + 5, stream=1)
                missing.add(missing0, expires=1)
                res = inventory.check_invs(payloads, kinds, have, missing, now, dandelion=dandelion)
                judged.append((res, _set_keys(missing, (0,), most), _set_keys(have, (1,), 4096)))
                have.clear(), missing.clear()
            missing.add(announced, expires=1)
            for (at, streams), objs in groups:
                recs = intake.check_objects(objs, streams=streams, now=at)
                admitted.append((recs, inventory.admit(recs, have, missing)))
            return judged, admitted, _set_keys(missing, (0,), 4096), _set_keys(have, stored_streams, 4096)

    def canon(res):
        judged, admitted, missing_keys, have_keys = res
        return _canon([[r.item_state, r.item_first, r.packets, m, h] for r, m, h in judged] +
                      [[recs.records, a.already, a.state] for recs, a in admitted] + [missing_keys, have_keys])

    def rows(keys):
        return [bytes(k) for k in keys]

    def check(res):  # the models and comparisons of tests/test_gpu_inv.py, on what run() kept of the sets
        judged, admitted, missing_keys, have_keys = res
        assert len(judged) == 2 and len(admitted) == len(groups)
        for case in cases:  # the model restates the reference case by case, as in test_golden_cases_through_check_invs
            m_missing = dict.fromkeys([t.item(k) for k in t.runs_to_ids(case['missing'])], 1)
            t.model_check_invs([t.regen_payload(p) for p in case['packets']], [t.KIND[p['kind']] for p in case['packets']],
                               set(t.item(k) for k in t.runs_to_ids(case['have'])), m_missing, now, case['dandelion'])
            final = sorted([t.item(k) for k in t.runs_to_ids(case['missing_final_runs'])] +
                           [bytes.fromhex(x) for x in case['missing_final_other'] if len(x) == 64])
            assert sorted(m_missing) == final, case['name']
        seen, statuses = set(), set()
        for (dandelion, have0, missing0, payloads, kinds), (r, m, h) in zip(flood, judged):  # ... and the device the model
            m_missing = dict.fromkeys(missing0, 1)
            t.check_result(r, t.model_check_invs(payloads, kinds, set(have0), m_missing, now, dandelion))
            assert rows(m) == sorted(m_missing) and rows(h) == have0
            seen.update(r.item_state.tolist())
            statuses.update(r.status.tolist())
        assert seen == {inventory.NOT_HAVE, inventory.HAVE, inventory.KNOWN, inventory.NEW, inventory.NEW_AGAIN,
                        inventory.SHORT}
        assert statuses == {inventory.OK, inventory.MALFORMED, inventory.TOO_MANY, inventory.IGNORED}
        m_have, m_missing = set(), dict.fromkeys(announced, 1)
        for (_, objs), (recs, a) in zip(groups, admitted):
            assert len(recs) == len(objs)
            invs = [recs.inventory_hash(i) for i in range(len(recs))]
            want_already, want_state = t.model_admit(recs.status.tolist(), invs, m_have, m_missing)
            assert a.already.tolist() == want_already and a.state.tolist() == want_state
        assert rows(missing_keys) == sorted(m_missing) and rows(have_keys) == sorted(m_have)
        assert len(m_have) > 3 and 5 <= len(m_missing) < len(announced)
    return Workload('inv', run, check, canon)


def _proc():
    from tests import test_gpu_proc as t
    from tests.proc_expect import objects
    kats = load_golden('proc_kats.json')
    objs, types = objects(kats)
    watched = [bytes.fromhex(k) for k in kats['watch']]

    def run():
        with t.fixture_dispatcher(kats) as d:
            res = d.dispatch(objs, types, now=kats['now'], rows_per_launch=16)
            n = len(d)
            # the keys still watched, asked in one call (every call waits for the library's lock): the dispatcher
            # is closed behind this line, so taking them out is as good as asking
            left = d.unwatch(watched)
            return res, sorted(k for k, there in zip(kats['watch'], left) if there), n

    class Left(object):  # what check_fixture asks of the dispatcher, from what run() kept of it
        def __init__(self, left, n):
            self.left, self.n = left, n

        def watching(self, key):
            return key.hex() in self.left

        def __len__(self):
            return self.n

    def check(res):
        t.check_fixture(kats, Left(res[1], res[2]), res[0])
        assert len(res[0]) == len(objs)
    return Workload('proc', run, check, lambda res: _canon([res[0].records, res[1], res[2]]))


_MAKERS = (_intake, _verify, _sig, _ecies, _ident, _rx, _rxobj, _rxsealed, _send, _tx, _addr, _aes, _packets, _inv, _proc)
_lock = threading.Lock()
_workloads = None
_baseline = None


def workloads():
    """Every workload, in a fixed order; the inputs are built once per process."""
    global _workloads
    with _lock:
        if _workloads is None:
            _workloads = [make() for make in _MAKERS]
        return _workloads


def baseline():
    """{name: canonical bytes} of every workload, each run once and checked against its fixture.  Call it first
    from one thread while nothing else uses the library; later calls return the same dict."""
    global _baseline
    if _baseline is None:
        base = {}
        for w in workloads():
            res = w.run()
            w.check(res)
            base[w.name] = w.canon(res)
            assert w() == base[w.name], '%s: two idle calls differ' % w.name
        _baseline = base
    return _baseline


def digest(name):
    """A short name for a workload's baseline bytes, for messages."""
    return hashlib.sha256(baseline()[name]).hexdigest()[:12]


def round_equals_baseline():
    """One call of every workload, each equal to its baseline; the names that differ."""
    base = baseline()
    return [w.name for w in workloads() if w() != base[w.name]]
