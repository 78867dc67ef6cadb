#!/usr/bin/env python3
"""Generate tests/golden/packet_kats.json -- packet-framing fixtures judged by the REFERENCE's own code where
it can be executed (needs a read-only checkout of the reference; its ``src`` directory is named by
PYBITMESSAGE_SRC, the environment of make_intake_golden.py):

    PYBITMESSAGE_SRC=<reference>/src BITMESSAGE_HOME=$(mktemp -d) PYTHONDONTWRITEBYTECODE=1 \\
        python tests/golden/make_packet_golden.py

Executed from the reference:

* ``protocol.CreatePacket`` builds every packet (a part that spells out another magic, length or checksum is
  re-packed with ``protocol.Header.pack`` over CreatePacket's own fields); ``protocol.Header.unpack`` reads
  every header in the walk; ``network.constants.MAX_MESSAGE_SIZE`` is the length limit;
* ``objectProcessor.ackDataHasAValidHeader`` judges every ack: the function's statements are lifted from
  src/class_objectProcessor.py with ``ast`` (the module imports a node's worth of state) and run against the
  reference's ``protocol`` and ``hashlib``; ``Header.unpack``'s command is handed over as the ``str`` Python 2
  saw, which is what its ``rstrip('\\x00')`` and ``!= 'object'`` are written for;
* the verdicts of the ``object`` packets' payloads are those ``judge`` of make_intake_golden.py reached with
  ``network.bmobject`` (tests/golden/intake_kats.json, each object under its first check).

Restated here, because ``network.bmproto`` does not import outside a running node -- the state machine of
src/network/bmproto.py:85-156, each rule beside the line it restates in :func:`walk`.

Payloads are regenerated in the tests by :func:`regen_buffer` from (seed, length) and pinned by their SHA-512;
no payload bytes are stored.
"""
import hashlib
import json
import os
import random
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 20250412
MAGIC = 0xE9BEB4D9
HEADER = struct.Struct('!L12sL4s')  # protocol.Header (asserted equal in main)
OK, TOO_LONG, BAD_CHECKSUM, NOT_ESTABLISHED = 0, 1, 2, 4
OPEN, BAD_MAGIC, INVALID_COMMAND, HANDSHAKE = 0, 1, 2, 3
# the bm_command_* methods of BMProto (src/network/bmproto.py), in the order of bmpow_packets.h's ids from 1
HANDLERS = ['error', 'getdata', 'inv', 'dinv', 'object', 'addr', 'portcheck', 'ping', 'pong', 'verack', 'version']


def payload_of(spec, intake_objects):
    """A part's payload: seeded random bytes, or an object of intake_kats.json by name."""
    if 'intake' in spec:
        return intake_objects[spec['intake']]
    data = random.Random(spec['seed']).randbytes(spec['len'])
    assert hashlib.sha512(data).hexdigest() == spec['sha512'], spec
    return data


def regen_buffer(case, intake_objects):
    """Rebuild a fixture buffer from its parts (shared with the tests): packets are header || payload with the
    checksum of the payload unless the part spoils it, ``junk`` parts are seeded bytes; ``cut`` keeps a prefix,
    ``zeros`` appends that many NULs."""
    out = []
    for part in case['parts']:
        if 'junk' in part:
            out.append(random.Random(part['junk']['seed']).randbytes(part['junk']['len']))
            continue
        data = payload_of(part['payload'], intake_objects)
        checksum = hashlib.sha512(data).digest()[:4]
        if part.get('spoil'):
            checksum = bytes([checksum[0] ^ 0x40]) + checksum[1:]
        out.append(HEADER.pack(part.get('magic', MAGIC), part['command'].encode('latin-1'), part.get('claim', len(data)),
                               checksum) + data)
    buf = b''.join(out)
    if 'cut' in case:
        buf = buf[:case['cut']]
    return buf + bytes(case.get('zeros', 0))


def main():
    ref_src = os.environ['PYBITMESSAGE_SRC']
    sys.path.insert(0, ref_src)
    import ast
    import protocol
    from network.constants import MAX_MESSAGE_SIZE
    sys.path.insert(0, HERE)  # (the reference has a ``tests`` package of its own)
    from make_intake_golden import regen as regen_object
    assert protocol.Header.format == HEADER.format and protocol.Header.size == 24
    with open(os.path.join(HERE, 'intake_kats.json')) as f:
        intake = json.load(f)
    intake_objects = {k['name']: regen_object(k) for k in intake['kats']}

    # ---- ackDataHasAValidHeader, lifted (src/class_objectProcessor.py:1019-1054) ----
    tree = ast.parse(open(os.path.join(ref_src, 'class_objectProcessor.py')).read())
    fn = next(n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == 'ackDataHasAValidHeader')
    fn.decorator_list = []
    module = ast.Module(body=[fn], type_ignores=[])

    class Py2Header(object):
        """protocol.Header, its command as the str Python 2's struct gave."""
        size = protocol.Header.size

        @staticmethod
        def unpack(data):
            magic, command, length, checksum = protocol.Header.unpack(data)
            return magic, command.decode('latin-1'), length, checksum

    class Quiet(object):
        def info(self, *args):
            pass

    scope = {'protocol': type('protocol', (), {'Header': Py2Header}), 'hashlib': hashlib, 'logger': Quiet()}
    exec(compile(module, 'class_objectProcessor.py', 'exec'), scope)
    ack_valid = scope['ackDataHasAValidHeader']

    def build(case):
        """The buffer from the reference's CreatePacket, and the same bytes from regen_buffer."""
        out = []
        for part in case['parts']:
            if 'junk' in part:
                out.append(random.Random(part['junk']['seed']).randbytes(part['junk']['len']))
                continue
            data = payload_of(part['payload'], intake_objects)
            pkt = protocol.CreatePacket(part['command'].encode('latin-1'), data)
            magic, command, length, checksum = protocol.Header.unpack(pkt[:24])
            assert magic == MAGIC and length == len(data) and pkt[24:] == data
            if part.get('spoil'):
                checksum = bytes([checksum[0] ^ 0x40]) + checksum[1:]
            out.append(protocol.Header.pack(part.get('magic', magic), command, part.get('claim', length), checksum) + data)
        buf = b''.join(out)
        if 'cut' in case:
            buf = buf[:case['cut']]
        buf += bytes(case.get('zeros', 0))
        assert buf == regen_buffer(case, intake_objects), case['name']
        return buf

    def walk(buf, established, datagram, check_sums):
        """state_bm_header / state_bm_command over a read buffer -> (records, consumed, close).  check_sums
        False: every checksum taken for good (what the host-only frame call answers)."""
        at, records = 0, []
        while True:
            if len(buf) - at < protocol.Header.size:                  # expectBytes = protocol.Header.size (:82)
                return records, at, OPEN
            magic, command, length, checksum = protocol.Header.unpack(buf[at:at + protocol.Header.size])  # :87-88
            command = command.rstrip(b'\x00')                         # :89
            if magic != 0xE9BEB4D9:                                   # :90
                if not datagram:                                      # :95-98 "Bad magic", close
                    return records, at, BAD_MAGIC
                at += 1                                               # :92 skip 1 byte in order to sync
                continue
            status = OK
            if length > MAX_MESSAGE_SIZE:                             # :99-100
                status |= TOO_LONG
            if len(buf) - at - protocol.Header.size < length:         # :101-103 expectBytes=self.payloadLength
                return records, at, OPEN
            payload = buf[at + 24:at + 24 + length]                   # :108
            computed = hashlib.sha512(payload).digest()[0:4]
            if check_sums and checksum != computed:                   # :109-111
                status |= BAD_CHECKSUM
            if not established and command not in (b'error', b'version', b'verack'):  # :113-118
                status |= NOT_ESTABLISHED
            name = command.decode('latin-1').lower()                  # :121-122 "bm_command_" + ...lower()
            handler = HANDLERS.index(name) + 1 if name in HANDLERS else 0  # AttributeError: unimplemented (:123-125)
            rec = {'offset': at, 'length': length, 'command': handler,
                   'exact': int(handler != 0 and command.decode('latin-1') == name),
                   'checksum': struct.unpack('>I', checksum)[0], 'computed': struct.unpack('>I', computed)[0],
                   'status': status}
            records.append(rec)
            if status != OK:                                          # :119, :144-151
                if not datagram:
                    return records, at, INVALID_COMMAND               # "Invalid command", close
            elif handler in (HANDLERS.index('version') + 1, HANDLERS.index('verack') + 1):
                return records, at + 24 + length, HANDSHAKE           # :498-560 change the connection's state
            at += 24 + length                                         # :152-154

    counter = [0]

    def rnd(length):
        counter[0] += 1
        seed = SEED * 1000 + counter[0]
        return {'seed': seed, 'len': length, 'sha512': hashlib.sha512(random.Random(seed).randbytes(length)).hexdigest()}

    def pkt(command, length=0, **kw):
        return dict({'command': command, 'payload': rnd(length)}, **kw)

    def obj(name, command='object', **kw):
        return dict({'command': command, 'payload': {'intake': name}}, **kw)

    conns = []

    def conn(name, parts, established=True, datagram=False, now=intake['now'], streams=(1,), **kw):
        case = dict({'name': name, 'established': established, 'datagram': datagram, 'now': now, 'streams': list(streams),
                     'parts': parts}, **kw)
        buf = build(case)
        case['len'] = len(buf)
        case['sha512'] = hashlib.sha512(buf).hexdigest()
        for key, sums in (('frame', False), ('batch', True)):
            records, consumed, close = walk(buf, established, datagram, sums)
            if not sums:
                for r in records:
                    del r['computed']
            case[key] = {'records': records, 'consumed': consumed, 'close': close}
        conns.append(case)
        print('%-34s len=%-8d frame=%d/%d batch=%d/%d consumed=%d' % (
            name, len(buf), len(case['frame']['records']), case['frame']['close'], len(case['batch']['records']),
            case['batch']['close'], case['batch']['consumed']))
        return case

    def expect(case, n, close, key='batch'):
        assert (len(case[key]['records']), case[key]['close']) == (n, close), (case['name'], case[key])

    # fewer than 24 bytes; a buffer cut inside a header and inside a payload
    expect(conn('header_23_bytes', [pkt('ping')], cut=23), 0, OPEN)
    expect(conn('empty', [], cut=0), 0, OPEN)
    expect(conn('cut_in_second_header', [pkt('ping', 5), pkt('pong', 40)], cut=29 + 11), 1, OPEN)
    expect(conn('cut_in_second_payload', [pkt('ping', 5), pkt('addr', 40)], cut=29 + 24 + 39), 1, OPEN)
    expect(conn('whole_second_payload', [pkt('ping', 5), pkt('addr', 40)]), 2, OPEN)
    # magic
    expect(conn('bad_magic_stream', [pkt('ping'), pkt('pong', 9, magic=0xE9BEB4D8), pkt('ping')]), 1, BAD_MAGIC)
    expect(conn('bad_magic_datagram', [{'junk': {'seed': SEED, 'len': 5}}, pkt('ping', 3), pkt('pong', 9, magic=0xD9B4BEE9),
                                       pkt('ping', 1)], datagram=True), 2, OPEN)
    # MAX_MESSAGE_SIZE and one above
    expect(conn('length_1600100', [pkt('ping', 2), pkt('inv', MAX_MESSAGE_SIZE), pkt('pong', 7)]), 3, OPEN)
    expect(conn('length_1600101_stream', [pkt('ping', 2), pkt('inv', MAX_MESSAGE_SIZE + 1), pkt('pong', 7)]), 2, INVALID_COMMAND)
    expect(conn('length_1600101_datagram', [pkt('ping', 2), pkt('inv', MAX_MESSAGE_SIZE + 1), pkt('pong', 7)], datagram=True),
           3, OPEN)
    expect(conn('too_long_waits_for_its_bytes', [pkt('ping', 2), pkt('inv', 100, claim=MAX_MESSAGE_SIZE + 1)]), 1, OPEN)
    # three packets, the second with a spoiled checksum
    c = conn('spoiled_second_stream', [pkt('ping', 10), pkt('addr', 200, spoil=True), pkt('pong', 10)])
    expect(c, 2, INVALID_COMMAND)
    expect(c, 3, OPEN, 'frame')
    expect(conn('spoiled_second_datagram', [pkt('ping', 10), pkt('addr', 200, spoil=True), pkt('pong', 10)], datagram=True),
           3, OPEN)
    # commands
    expect(conn('object_in_capitals', [obj('msg_ok', 'OBJECT'), pkt('Ping', 4)]), 2, OPEN)
    expect(conn('command_12_bytes_no_nul', [pkt('abcdefghijkl', 30), pkt('ping')]), 2, OPEN)
    expect(conn('object_nul_x', [obj('msg_ok', 'object\x00x'), pkt('ping')]), 2, OPEN)
    expect(conn('every_handler', [pkt(h, 13 * i) for i, h in enumerate(HANDLERS[:9])] + [pkt('getbiginv', 4), pkt('', 2)]),
           11, OPEN)
    # the handshake and the connections that are not fully established
    expect(conn('established_version', [pkt('ping', 1), pkt('version', 90), pkt('ping', 2)]), 2, HANDSHAKE)
    expect(conn('unestablished_verack_inv', [pkt('verack'), pkt('inv', 33)], established=False), 1, HANDSHAKE)
    expect(conn('unestablished_inv', [pkt('inv', 33), pkt('ping')], established=False), 1, INVALID_COMMAND)
    expect(conn('unestablished_error_object', [pkt('error', 12), obj('msg_ok')], established=False), 2, INVALID_COMMAND)
    expect(conn('unestablished_VERSION_capitals', [pkt('VERSION', 90)], established=False), 1, INVALID_COMMAND)
    c = conn('spoiled_version_datagram', [pkt('version', 90, spoil=True), pkt('ping', 6)], datagram=True)
    expect(c, 2, OPEN)
    expect(c, 1, HANDSHAKE, 'frame')
    expect(conn('unestablished_datagram', [pkt('ping', 6), pkt('verack')], established=False, datagram=True), 2, HANDSHAKE)
    # the objects of intake_kats.json as packets, each under its first check; a spoiled one on a datagram socket
    groups = {}
    for k in intake['kats']:
        chk = k['checks'][0]
        groups.setdefault((chk['now'], tuple(chk['streams'])), []).append(k)
    for (now, streams), kats in sorted(groups.items()):
        parts = [obj(k['name']) for k in kats]
        case = conn('intake_now_%d_streams_%s' % (now, '_'.join(map(str, streams)) or 'none'), parts, now=now, streams=streams)
        expect(case, len(kats), OPEN)
        case['intake_status'] = [k['checks'][0]['status'] for k in kats]
    case = conn('spoiled_object_datagram', [obj('msg_ok'), obj('pubkey_ok', spoil=True), obj('broadcast_ok')], datagram=True)
    expect(case, 3, OPEN)

    acks = []

    def ack(name, parts, **kw):
        case = dict({'name': name, 'parts': parts}, **kw)
        buf = build(case)
        case['len'] = len(buf)
        case['sha512'] = hashlib.sha512(buf).hexdigest()
        case['valid'] = bool(ack_valid(buf))
        acks.append(case)
        print('ack %-30s len=%-6d valid=%s' % (name, len(buf), case['valid']))
        return case

    full = 24 + len(intake_objects['msg_ok'])
    assert ack('valid', [obj('msg_ok')])['valid']
    assert ack('valid_unsolved', [obj('unsolved_msg')])['valid']
    assert not ack('one_byte_short', [obj('msg_ok')], cut=full - 1)['valid']
    assert not ack('one_byte_long', [obj('msg_ok')], zeros=1)['valid']
    assert not ack('OBJECT', [obj('msg_ok', 'OBJECT')])['valid']
    assert not ack('wrong_checksum', [obj('msg_ok', spoil=True)])['valid']
    assert not ack('23_bytes', [obj('msg_ok')], cut=23)['valid']
    assert not ack('bad_magic', [obj('msg_ok', magic=0xE9BEB4D8)])['valid']
    assert not ack('ping', [pkt('ping', 30)])['valid']
    assert not ack('empty', [], cut=0)['valid']
    assert ack('valid_malformed_object', [pkt('object', 12)])['valid']

    with open(os.path.join(HERE, 'packet_kats.json'), 'w') as f:
        json.dump({'source': 'reference protocol.CreatePacket / Header, network.constants.MAX_MESSAGE_SIZE, '
                             'objectProcessor.ackDataHasAValidHeader (lifted); bmproto.py:85-156 restated by '
                             'make_packet_golden.walk; buffers regenerated by make_packet_golden.regen_buffer',
                   'max_message_size': MAX_MESSAGE_SIZE, 'handlers': HANDLERS, 'connections': conns, 'acks': acks},
                  f, indent=1)
    print('wrote packet_kats.json (%d connections, %d acks)' % (len(conns), len(acks)))


if __name__ == '__main__':
    main()
