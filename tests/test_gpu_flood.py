"""One node's loop over a flood, on the GPU, on objects this library made: ``worker.send_msgs_built`` /
``send_broadcasts`` / ``send_pubkeys`` and a getpubkey put on the wire as two connections' read buffers, then
``packets.check_buffers`` -> ``inventory.check_invs`` -> ``inventory.admit`` -> ``Dispatcher.dispatch`` ->
``receive.open_sealed_msgs`` / ``open_sealed_objects``, the recovered acks back in as a third connection through
``check_buffers`` -> ``admit`` -> ``dispatch_packets``, and the same flood once more against the sets as they
stand.  The seams are what is under test: ``packet_index`` / ``source_index``, the zeroed records of packets that
are no valid object, the rows ``admit`` skips, copies of one object on two connections, the types taken from the
intake record, and the ack that is itself a packet.

Every expectation comes from the inputs (texts, keys, ack data, addresses, the list of packets written here), from
hashlib, or from the models the per-subsystem tests already have (``model_check_invs``, ``model_admit``,
``processor.walk``).  The signing nonces and ephemeral keys are drawn inside the library; ``now``, the rngs the
send side takes and the sets' seeds are fixed.  Every malformed input is a defined status: nothing provokes a
fault."""
import hashlib
import random
import struct

import numpy as np
import pytest

from pybitmessage_amd import intake, inventory, outgoing, packets, processor as P, proofofwork, receive, targets, worker
from pybitmessage_amd.inventory import ABSENT, ADDED, DUP, PRESENT
from tests.golden.make_inv_golden import item
from tests.test_gpu_inv import KIND, check_result, inv_payload, model_admit, model_check_invs, set_keys
from tests.test_gpu_packets import packet, sum4
from tests.test_gpu_tx import people  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

NOW = 1760000000
MSG_TTL, BROADCAST_TTL = 6 * 3600, 2 * 24 * 3600
NO_ACK = (P.NOT_WATCHED, 0, P.NO_ROW)


def inv_hash(obj):
    return hashlib.sha512(hashlib.sha512(obj).digest()).digest()[:32]


def ack_columns(res):
    return list(zip(res.ack.tolist(), res.ack_aux.tolist(), res.ack_first.tolist()))


@pytest.fixture(scope='module')
def traffic(gpulib, people):  # noqa: F811
    """Eight objects a peer (the v4 identity) sends to a node that holds the v3 and the v2 identity, and what the
    node knows: its keys, its address table, the ack data the peer watches for."""
    me, a, b = people['v4'], people['v3'], people['v2']
    rng = random.Random(20261021)
    ackdata = {0: b'\x00\x00\x00\x02\x01\x01' + rng.randbytes(32), 2: b'\x00\x00\x00\x02\x01\x01' + rng.randbytes(32)}
    texts = [b'Subject:flood\nBody:' + name * 9 for name in (b'first ', b'second ', b'third ')]
    to = [a, b, b]
    full_acks = {}

    def build_plain(job, ack):
        full_acks[job] = ack
        plain = worker.msg_plaintext(me.version, me.stream, worker.get_bitfield(), me.pub_s, me.pub_e, to[job].ripe, 2,
                                     texts[job], ack)
        return plain, me.priv_s, to[job].pub_e, to[job].version, 1, MSG_TTL, None, None

    msgs = worker.send_msgs_built([(ackdata.get(job), MSG_TTL, job) for job in range(3)], build_plain,
                                  rng=random.Random(1), now=NOW)
    casters = [a, me]  # a v4 broadcast (trial decryption) and a v5 one (by its tag)
    casts = [b'Subject:s\nBody:' + p.address.encode() for p in casters]
    broadcasts = worker.send_broadcasts(
        [(outgoing.BroadcastFields(None, p.version, p.stream, p.ripe, worker.get_bitfield(), p.pub_s, p.pub_e, 2, text, None,
                                   None, p.priv_s), BROADCAST_TTL) for p, text in zip(casters, casts)],
        rng=random.Random(2), now=NOW)
    pubkeys = worker.send_pubkeys([outgoing.PubkeyFields(None, p.version, p.stream, p.ripe, worker.get_bitfield(), p.pub_s,
                                                         p.pub_e, None, None, p.priv_s) for p in casters],
                                  rng=random.Random(3), now=NOW)
    ask = worker.getpubkey_object(a.version, a.stream, a.ripe, rng=random.Random(4), now=NOW)
    _trial, nonce = proofofwork.run(ask.target, ask.initial_hash)
    objs = msgs + broadcasts + pubkeys + [struct.pack('>Q', nonce) + ask.payload]
    assert all(o is not None for o in objs) and len(set(objs)) == 8
    for o in objs:  # before anything goes on the wire
        assert targets.isProofOfWorkSufficient(o, recvTime=NOW)
    assert sorted(full_acks) == [0, 1, 2] and full_acks[1] == b''
    for job in (0, 2):  # a whole `object` packet around nonce, time and the ack data
        assert receive.ack_has_valid_header(full_acks[job]) and full_acks[job][24 + 16:] == ackdata[job]
    return {
        'objs': objs, 'types': [P.OBJECT_MSG] * 3 + [P.OBJECT_BROADCAST] * 2 + [P.OBJECT_PUBKEY] * 2 + [P.OBJECT_GETPUBKEY],
        'me': me, 'to': to, 'texts': texts, 'casters': casters, 'casts': casts, 'ackdata': ackdata, 'full_acks': full_acks,
        'keys': {a.ripe: a.priv_e, b.ripe: b.priv_e},
        'table': P.address_rows([(a.version, a.stream, a.ripe, False, 0), (b.version, b.stream, b.ripe, False, 0)]),
        'asked': a,
    }


def wire(traffic):
    """The two connections' packets as ``(connection, command, payload, spoiled)`` in wire order, the buffers, and
    the three announced hashes that are never sent."""
    objs = traffic['objs']
    hashes = [inv_hash(o) for o in objs]
    never = [item(95000 + k) for k in range(3)]
    order = [5, 0, 7, 2, 6, 1, 4, 3]
    parts = [(0, b'inv', inv_payload(hashes + never), False)] + [(0, b'object', o, False) for o in objs] + [(0, b'ping', b'', False)]
    parts += [(1, b'object', objs[k], False) for k in order]
    parts += [(1, b'getdata', inv_payload([hashes[1], hashes[4]]), False), (1, b'object', objs[2], True)]
    bufs = [b''.join(packet(cmd, p, spoil=bad) for c, cmd, p, bad in parts if c == conn) for conn in (0, 1)]
    return parts, bufs, hashes, never


def framed_as_written(res, parts, bufs):
    """check_buffers against the packets written: every checksum is hashlib's, only the spoiled packet fails, and a
    spoiled last packet is recorded, closes its connection and stays in the read buffer."""
    assert len(res) == len(parts)
    assert res.conn.tolist() == [c for c, _, _, _ in parts]
    assert [bytes(res.payload(i)) for i in range(len(res))] == [p for _, _, p, _ in parts]
    assert [res.command_name(i) for i in range(len(res))] == [cmd for _, cmd, _, _ in parts]
    assert res.computed.tolist() == [sum4(p) for _, _, p, _ in parts]
    assert res.status.tolist() == [packets.BAD_CHECKSUM if bad else packets.OK for _, _, _, bad in parts]
    spoiled = [sum(24 + len(p) for c, _, p, bad in parts if bad and c == conn) for conn in range(len(bufs))]
    assert res.count.tolist() == [sum(1 for c, _, _, _ in parts if c == conn) for conn in range(len(bufs))]
    assert res.consumed.tolist() == [len(buf) - cut for buf, cut in zip(bufs, spoiled)]
    assert res.close.tolist() == [packets.INVALID_COMMAND if cut else packets.OPEN for cut in spoiled]
    valid = [i for i, (_, cmd, _, bad) in enumerate(parts) if cmd == b'object' and not bad]
    assert res.objects().tolist() == valid  # every intake check passed
    others = np.setdiff1d(np.arange(len(res)), valid)
    assert not res.records['intake'][others].tobytes().strip(b'\x00')
    assert [res.intake.inventory_hash(i) for i in valid] == [inv_hash(parts[i][2]) for i in valid]
    return valid


def judged_and_admitted(res, parts, valid, have, missing, m_have, m_missing):
    """check_invs and admit on a framed flood against the models, which carry ``m_have`` / ``m_missing`` along."""
    rows = [i for i, (_, cmd, _, _) in enumerate(parts) if cmd in (b'inv', b'getdata')]
    judged = inventory.check_invs(res, None, have, missing, NOW)
    assert judged.packet_index.tolist() == rows
    check_result(judged, model_check_invs([parts[i][2] for i in rows], [KIND[parts[i][1].decode()] for i in rows],
                                          m_have, m_missing, NOW))
    assert set_keys(missing) == sorted(m_missing)
    # a packet that is no valid object carries a zeroed record and takes no part: MALFORMED in the model
    status = [intake.OK if i in valid else intake.MALFORMED for i in range(len(parts))]
    invs = [inv_hash(p) if i in valid else bytes(32) for i, (_, _, p, _) in enumerate(parts)]
    want_already, want_state = model_admit(status, invs, m_have, m_missing)
    admitted = inventory.admit(res, have, missing)
    assert admitted.already.tolist() == want_already and admitted.state.tolist() == want_state
    assert admitted.stored.tolist() == [i in valid for i in range(len(parts))]
    assert set_keys(missing) == sorted(m_missing) and len(have) == len(m_have) and bytes(32) not in have
    return judged, admitted


def round_one(traffic, have, missing, d):
    """The flood against empty sets; returns what the later rounds need and the results' bytes."""
    objs, types, me = traffic['objs'], traffic['types'], traffic['me']
    parts, bufs, hashes, never = wire(traffic)
    res = packets.check_buffers(bufs, now=NOW)
    valid = framed_as_written(res, parts, bufs)
    assert valid == list(range(1, 9)) + list(range(10, 18)) and len(parts) == 20
    m_have, m_missing = set(), {}
    judged, admitted = judged_and_admitted(res, parts, valid, have, missing, m_have, m_missing)
    assert judged.item_state.tolist() == [inventory.NEW] * 11 + [inventory.NOT_HAVE] * 2
    assert [judged.item(j) for j in range(len(judged))] == hashes + never + [hashes[1], hashes[4]]
    assert admitted.state.tolist() == [ABSENT] + [ADDED] * 8 + [ABSENT] + [DUP] * 8 + [ABSENT] * 2
    assert not admitted.already.any()
    assert set_keys(missing) == sorted(never) and sorted(m_have) == sorted(hashes)
    found, vals = have.contains(hashes, values=True)
    assert found.all() and vals['expires'].tolist() == [struct.unpack('>Q', o[8:16])[0] for o in objs]
    assert vals['stream'].tolist() == [1] * 8 and vals['aux'].tolist() == list(range(1, 9))  # the first copy's row

    # the objects stored by this call go to the object processor, with the types the intake read
    added = [int(i) for i in res.objects() if admitted.state[i] == ADDED]
    assert added == list(range(1, 9))
    assert res.intake.objectType[added].tolist() == types
    out = d.dispatch([res.payload(i) for i in added], res.intake.objectType[added], now=NOW)
    assert out.route.tolist() == [P.MSG] * 3 + [P.BROADCAST] * 2 + [P.PUBKEY] * 2 + [P.GETPUBKEY]
    assert ack_columns(out) == [NO_ACK] * 8 and len(d) == 2
    want = P.walk(P.OBJECT_GETPUBKEY, objs[7], traffic['table'], now=NOW)
    assert out.status.tolist() == [P.NONE] * 7 + [P.SEND_V3] and int(want['status']) == P.SEND_V3
    fields = [f for f in P.REC_DTYPE.names if not f.startswith('ack')]  # the walk leaves the ack fields alone
    assert [int(out.records[7][f]) for f in fields] == [int(want[f]) for f in fields]
    assert int(out.address[7]) == 0 and out.requested_key(7) == traffic['asked'].ripe
    assert out.pubkey_requests() == [(7, 'sendOutOrStoreMyV3Pubkey', traffic['asked'].ripe)]

    # ... and are opened
    assert out.msgs().tolist() == [0, 1, 2]
    opened = receive.open_sealed_msgs([bytes(res.payload(added[i])) for i in out.msgs()], traffic['keys'])
    assert opened.status.tolist() == [receive.OK] * 3
    for i in range(3):
        assert opened.message(i) == traffic['texts'][i] and opened.fromAddress(i) == me.address
        assert opened.toRipe(i) == traffic['to'][i].ripe and opened.ackData(i) == traffic['full_acks'][i]
    rest = out.broadcasts().tolist() + out.pubkeys().tolist()
    assert rest == [3, 4, 5, 6]
    casters = traffic['casters']
    others = receive.open_sealed_objects([receive.KIND_BROADCAST] * 2 + [receive.KIND_PUBKEY] * 2,
                                         [bytes(res.payload(added[i])) for i in rest], [p.address for p in casters],
                                         {p.tag: p.address for p in casters if p.version >= 4})
    assert others.status.tolist() == [receive.OBJ_OK] * 4
    assert [others.fromAddress(i) for i in range(4)] == [p.address for p in casters] * 2
    assert [others.ripe(i) for i in range(4)] == [p.ripe for p in casters] * 2
    assert [others.message(i) for i in range(2)] == traffic['casts']
    seen = b''.join([res.records.tobytes(), res.connections.tobytes(), judged.packets.tobytes(), judged.item_state.tobytes(),
                     judged.item_first.tobytes(), admitted.already.tobytes(), admitted.state.tobytes(), out.records.tobytes(),
                     opened.recs.tobytes(), others.recs.tobytes()])
    return {'bufs': bufs, 'parts': parts, 'valid': valid, 'hashes': hashes, 'never': never, 'opened': opened,
            'm_have': m_have, 'm_missing': m_missing, 'bytes': seen}


def fresh(traffic):
    have, missing = inventory.InventorySet(64, seed=71), inventory.InventorySet(64, seed=72)
    d = P.Dispatcher(seed=73)
    assert d.watch([traffic['ackdata'][0], traffic['ackdata'][2]], aux=[0, 2]).all()
    d.set_addresses(traffic['table'])
    return have, missing, d


def test_a_flood_from_socket_bytes_to_the_last_verdict(gpulib, shards, traffic):
    ackdata = traffic['ackdata']
    have, missing, d = fresh(traffic)
    with have, missing, d:
        first = round_one(traffic, have, missing, d)
        m_have, m_missing = first['m_have'], first['m_missing']

        # ---- round 2: the acks come back, each a whole packet, as a third connection's buffer ----
        opened = first['opened']
        rows, ok, recs = receive.check_opened_acks(opened, now=NOW)
        assert rows == [0, 1, 2] and ok.tolist() == [True, False, True]
        assert recs.status[ok].tolist() == [intake.OK] * 2
        acks = [opened.ackData(i) for i, good in zip(rows, ok) if good]
        parts = [(0, b'object', a[24:], False) for a in acks]
        assert [p[16:] for _, _, p, _ in parts] == [ackdata[0], ackdata[2]]
        res = packets.check_buffers([b''.join(acks)], now=NOW)
        assert framed_as_written(res, parts, [b''.join(acks)]) == [0, 1]
        status, invs = [intake.OK] * 2, [inv_hash(p) for _, _, p, _ in parts]
        want_already, want_state = model_admit(status, invs, m_have, m_missing)
        admitted = inventory.admit(res, have, missing)
        assert admitted.already.tolist() == want_already == [False] * 2
        assert admitted.state.tolist() == want_state == [ADDED] * 2 and len(have) == len(m_have) == 10
        out = d.dispatch_packets(res, now=NOW)
        assert out.source_index.tolist() == [0, 1] and out.route.tolist() == [P.MSG] * 2
        assert ack_columns(out) == [(P.FOUND, 0, 0), (P.FOUND, 2, 1)]
        assert out.acks().tolist() == [0, 1] and [out.ack_key(i) for i in range(2)] == [ackdata[0], ackdata[2]]
        assert len(d) == 0 and not d.watching(ackdata[0]) and not d.watching(ackdata[2])

        # ---- round 3: the same flood again, against the sets as they stand ----
        parts, bufs, hashes, never = first['parts'], first['bufs'], first['hashes'], first['never']
        res = packets.check_buffers(bufs, now=NOW)
        assert framed_as_written(res, parts, bufs) == first['valid']
        judged, admitted = judged_and_admitted(res, parts, first['valid'], have, missing, m_have, m_missing)
        assert judged.item_state.tolist() == [inventory.HAVE] * 8 + [inventory.KNOWN] * 3 + [inventory.HAVE] * 2
        assert admitted.already[first['valid']].all() and admitted.already.sum() == 16
        assert admitted.state.tolist() == [ABSENT] + [PRESENT] * 8 + [ABSENT] + [PRESENT] * 8 + [ABSENT] * 2
        assert [int(i) for i in res.objects() if admitted.state[i] == ADDED] == []  # nothing goes to the processor
        assert set_keys(missing) == sorted(never) and len(have) == 10

    # ---- round 1 under three shards on the one device: byte-equal per packet, per item and per object ----
    shards([0, 0, 0])
    have, missing, d = fresh(traffic)
    with have, missing, d:
        assert round_one(traffic, have, missing, d)['bytes'] == first['bytes']
