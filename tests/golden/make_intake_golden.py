#!/usr/bin/env python3
"""Generate tests/golden/intake_kats.json -- object-intake fixtures judged by the REFERENCE's own code
(needs a read-only checkout of the reference; its ``src`` directory is named by PYBITMESSAGE_SRC):

    PYBITMESSAGE_SRC=<reference>/src BITMESSAGE_HOME=$(mktemp -d) PYTHONDONTWRITEBYTECODE=1 \\
        python tests/golden/make_intake_golden.py

Executed from the reference, per case:

* the varints: ``addresses.decodeVarint`` on the bytes after ``>QQI`` (``varintDecodeError`` ->
  MALFORMED);
* ``network.bmobject.BMObject(...)``: ``inventoryHash`` (``addresses.calculateInventoryHash``) and
  ``tag``;
* ``BMObject.checkProofOfWorkSufficient`` (``protocol.isProofOfWorkSufficient`` at its defaults),
  ``checkEOLSanity``, ``checkStream`` (over ``state.streamsInWhichIAmParticipating``) and
  ``checkObjectByType``, in ``bm_command_object``'s order, with ``time.time`` fixed per check.

``network.bmobject`` imports ``inventory`` and ``network.dandelion`` for ``checkAlreadyHave`` only
(not part of the intake); both are stubbed in ``sys.modules`` before the import.

Restated here, because ``network.bmproto`` does not import outside a running node:

* ``decode_payload_content("QQIvv")``'s fixed part as ``struct.unpack('>QQI', data[:20])`` and its
  varint step ``value, n = decodeVarint(payload[offset:]); offset += n``
  (src/network/bmproto.py:164-169, :206-224, :380-381); ``struct.error`` -> MALFORMED;
* ``payload_len = len(payload) - payloadOffset; payload_len > MAX_OBJECT_PAYLOAD_SIZE`` ->
  TOO_LARGE (src/network/bmproto.py:386-391; the constant is imported from network/constants.py);
* the order of the checks (src/network/bmproto.py:393-415);
* which of ``checkEOLSanity``'s two ``BMObjectExpiredError`` raises it was: FUTURE when
  ``expiresTime - now > 0``, else PAST (src/network/bmobject.py:82, :89).

Objects are regenerated in the tests by :func:`regen` from (seed, L, header fields); ``sha512_obj`` pins
the bytes.  The nonce search (the C oracle) only produces inputs.
"""
import hashlib
import json
import os
import random
import struct
import sys
import types
from struct import pack

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 20250301
NOW = 1700000000
MAX_TTL = 28 * 24 * 60 * 60 + 10800
MIN_TTL = -3600

OK, MALFORMED, TOO_LARGE, INSUFFICIENT_POW, EXPIRED_FUTURE, EXPIRED_PAST, INVALID_STREAM, UNWANTED_STREAM, \
    INVALID_FOR_TYPE = range(9)


def varint(v):
    """The shortest encoding (addresses.encodeVarint's)."""
    if v < 253:
        return pack('>B', v)
    if v < 65536:
        return b'\xfd' + pack('>H', v)
    if v < 4294967296:
        return b'\xfe' + pack('>I', v)
    return b'\xff' + pack('>Q', v)


def body_of(kat):
    """object[8:]: expires, type, the raw bytes after them (``tail``: the varints as the case spells
    them), then seeded random bytes up to L bytes in all (nonce included); cut short where L says so."""
    tail = bytes.fromhex(kat['tail'])
    head = (pack('>QI', kat['expires'], kat['type']) + tail)[:max(kat['L'] - 8, 0)]
    rest = kat['L'] - 8 - len(head)
    return head + (random.Random(kat['seed']).randbytes(rest) if rest > 0 else b'')


def regen(kat):
    """Rebuild a fixture object (shared with the tests)."""
    obj = (pack('>Q', kat['nonce']) + body_of(kat))[:kat['L']]
    assert len(obj) == kat['L'] and hashlib.sha512(obj).hexdigest() == kat['sha512_obj'], kat['name']
    return obj


def main():
    ref_src = os.environ['PYBITMESSAGE_SRC']
    sys.path.insert(0, ref_src)
    import time
    inv_stub = types.ModuleType('inventory')
    inv_stub.Inventory = lambda: ()
    sys.modules['inventory'] = inv_stub
    import network  # noqa: F401  (the package, before its stubbed submodule)
    dan_stub = types.ModuleType('network.dandelion')
    dan_stub.Dandelion = lambda: None
    sys.modules['network.dandelion'] = dan_stub
    import addresses
    import protocol
    import state
    from network import bmobject
    from network.constants import MAX_OBJECT_PAYLOAD_SIZE
    sys.path.insert(0, os.path.join(HERE, '..', '..'))
    from oracle.oracle import COracle
    co = COracle()
    assert bmobject.BMObject.maxTTL == MAX_TTL and bmobject.BMObject.minTTL == MIN_TTL

    def judge(data, now, streams):
        """bm_command_object's checks over data at time now -> (status, fields or None, pow_ok or None)."""
        time.time = lambda: float(now)
        state.streamsInWhichIAmParticipating = list(streams)
        try:
            nonce, expires, otype = struct.unpack('>QQI', data[:20])
            off = 20
            version, n = addresses.decodeVarint(data[off:])
            off += n
            stream, n = addresses.decodeVarint(data[off:])
            off += n
        except (struct.error, addresses.varintDecodeError):
            return MALFORMED, None, None
        obj = bmobject.BMObject(nonce, expires, otype, version, stream, data, off)
        fields = {'nonce': nonce, 'expires': expires, 'type': otype, 'version': version, 'stream': stream,
                  'payloadOffset': off, 'inv': bytes(obj.inventoryHash).hex(), 'tag': bytes(obj.tag).hex()}
        pow_ok = bool(protocol.isProofOfWorkSufficient(data))
        if len(data) - off > MAX_OBJECT_PAYLOAD_SIZE:
            return TOO_LARGE, fields, pow_ok
        try:
            obj.checkProofOfWorkSufficient()
        except bmobject.BMObjectInsufficientPOWError:
            assert not pow_ok
            return INSUFFICIENT_POW, fields, pow_ok
        assert pow_ok
        try:
            obj.checkEOLSanity()
        except bmobject.BMObjectExpiredError:
            return (EXPIRED_FUTURE if expires - now > 0 else EXPIRED_PAST), fields, pow_ok
        try:
            obj.checkStream()
        except bmobject.BMObjectInvalidError:
            return INVALID_STREAM, fields, pow_ok
        except bmobject.BMObjectUnwantedStreamError:
            return UNWANTED_STREAM, fields, pow_ok
        try:
            obj.checkObjectByType()
        except bmobject.BMObjectInvalidError:
            return INVALID_FOR_TYPE, fields, pow_ok
        return OK, fields, pow_ok

    kats = []

    def case(name, L, otype=2, version=1, stream=1, expires=NOW + 300, tail=None, solve_ttl=300, checks=((NOW, (1,)),),
             nonce_delta=0, seed=None):
        """One object and its verdicts.  solve_ttl: the TTL whose target the nonce is searched for (None:
        nonce 1, unsolved)."""
        kat = {'name': name, 'seed': SEED * 1000 + len(kats) if seed is None else seed, 'L': L, 'expires': expires, 'type': otype,
               'tail': (varint(version) + varint(stream) if tail is None else tail).hex(), 'nonce': 1}
        body = body_of(kat)
        if solve_ttl is not None:
            ln = len(body) + 8 + 1000
            target = int(2 ** 64 / (1000 * (ln + ((max(solve_ttl, 300) * ln) / (2 ** 16)))))
            (_, nonce), _ = co.search_mt(hashlib.sha512(body).digest(), target, 1, 1 << 44,
                                         threads=min(os.cpu_count() or 8, 16))
            kat['nonce'] = nonce + nonce_delta
        obj = (pack('>Q', kat['nonce']) + body)[:L]
        kat['sha512_obj'] = hashlib.sha512(obj).hexdigest()
        assert regen(kat) == obj
        kat['fields'] = None
        kat['checks'] = []
        for now, streams in checks:
            status, fields, pow_ok = judge(obj, now, streams)
            kat['fields'] = fields
            kat['checks'].append({'now': now, 'streams': list(streams), 'status': status, 'pow_ok': pow_ok})
        kats.append(kat)
        print('%-28s L=%-7d nonce=%-12d %s' % (name, L, kat['nonce'], [c['status'] for c in kat['checks']]))
        return kat

    def expect(kat, *statuses):
        assert [c['status'] for c in kat['checks']] == list(statuses), (kat['name'], kat['checks'])

    # every object type, accepted; and the same objects one nonce on
    for name, otype, L, version in [('getpubkey', 0, 100, 4), ('pubkey', 1, 200, 4), ('msg', 2, 300, 1),
                                    ('broadcast', 3, 250, 5), ('onionpeer', 0x746f72, 120, 3)]:
        ok = case(name + '_ok', L, otype, version)
        expect(ok, OK)
        case(name + '_next_nonce', L, otype, version, nonce_delta=1, seed=ok['seed'])  # the same object, one nonce on
    # EOL edges (bmobject.py:78-94): exactly maxTTL / minTTL pass, one second past each does not
    expect(case('eol_future_edge', 160, expires=NOW + MAX_TTL, solve_ttl=MAX_TTL + 1,
                checks=((NOW, (1,)), (NOW - 1, (1,)))), OK, EXPIRED_FUTURE)
    expect(case('eol_past_edge', 160, expires=NOW + MIN_TTL, checks=((NOW, (1,)), (NOW + 1, (1,)), (NOW + 10 ** 6, (1,)))),
           OK, EXPIRED_PAST, EXPIRED_PAST)
    # streams (bmobject.py:96-107)
    expect(case('stream_0', 150, stream=0), INVALID_STREAM)
    expect(case('stream_max', 150, stream=2 ** 63 - 1, checks=((NOW, (2 ** 63 - 1,)), (NOW, (1,)))), OK, UNWANTED_STREAM)
    expect(case('stream_2_63', 150, stream=2 ** 63, checks=((NOW, (2 ** 63,)),)), INVALID_STREAM)
    expect(case('stream_2', 150, stream=2, checks=((NOW, (1,)), (NOW, (1, 2)), (NOW, ()))), UNWANTED_STREAM, OK,
           UNWANTED_STREAM)
    expect(case('stream_300_version_70000', 150, version=70000, stream=300, checks=((NOW, (300,)),)), OK)
    # per-type sizes (bmobject.py:138-163)
    expect(case('getpubkey_41', 41, 0, 4), INVALID_FOR_TYPE)
    expect(case('getpubkey_42', 42, 0, 4), OK)
    expect(case('pubkey_145', 145, 1, 4), INVALID_FOR_TYPE)
    expect(case('pubkey_146', 146, 1, 4), OK)
    expect(case('pubkey_440', 440, 1, 4), OK)
    expect(case('pubkey_441', 441, 1, 4), INVALID_FOR_TYPE)
    expect(case('broadcast_179', 179, 3, 5), INVALID_FOR_TYPE)
    expect(case('broadcast_180', 180, 3, 5), OK)
    expect(case('broadcast_v1', 200, 3, 1), INVALID_FOR_TYPE)
    # the size limit after the header (bmproto.py:386-391): 22 header bytes here
    expect(case('payload_2_18', 22 + 2 ** 18), OK)
    expect(case('payload_2_18_plus_1', 22 + 2 ** 18 + 1, solve_ttl=None), TOO_LARGE)
    # headers that do not decode, and the shortest ones that do
    fd, fe, ff = b'\xfd', b'\xfe', b'\xff'
    for name, L, tail in [('version_fd_nonminimal', 100, fd + pack('>H', 252) + b'\x01'),
                          ('version_fe_nonminimal', 100, fe + pack('>I', 65535) + b'\x01'),
                          ('stream_ff_nonminimal', 100, b'\x01' + ff + pack('>Q', 4294967295)),
                          ('stream_fd_truncated', 23, b'\x01' + fd + b'\x01'),
                          ('version_ff_truncated', 28, ff + pack('>Q', 2 ** 40)),
                          ('stream_fe_truncated', 25, b'\x01' + fe + pack('>I', 70000)),
                          ('len_19', 19, b''), ('len_8', 8, b''), ('len_0', 0, b'')]:
        expect(case(name, L, tail=tail, solve_ttl=None), MALFORMED)
    # decodeVarint of no bytes is (0, 0): these decode, with version / stream 0
    case('len_20_empty_varints', 20, tail=b'', solve_ttl=None)
    case('len_21_empty_stream', 21, tail=b'\x03', solve_ttl=None)
    assert kats[-2]['fields']['payloadOffset'] == 20 and kats[-1]['fields'] == dict(kats[-1]['fields'], version=3, stream=0)
    case('unsolved_msg', 400, solve_ttl=None)

    with open(os.path.join(HERE, 'intake_kats.json'), 'w') as f:
        json.dump({'source': 'reference addresses.decodeVarint / calculateInventoryHash, protocol.isProofOfWorkSufficient '
                             'and network.bmobject.BMObject checks; objects regenerated by make_intake_golden.regen',
                   'now': NOW, 'status_names': ['OK', 'MALFORMED', 'TOO_LARGE', 'INSUFFICIENT_POW', 'EXPIRED_FUTURE',
                                                'EXPIRED_PAST', 'INVALID_STREAM', 'UNWANTED_STREAM', 'INVALID_FOR_TYPE'],
                   'kats': kats}, f, indent=1)
    print('wrote intake_kats.json (%d cases)' % len(kats))


if __name__ == '__main__':
    main()
