#!/usr/bin/env python3
"""Generate tests/golden/proc_kats.json -- a queue of the object processor judged by the REFERENCE's own code
(needs a read-only checkout of the reference; its ``src`` directory is named by PYBITMESSAGE_SRC, the
environment of make_intake_golden.py):

    PYBITMESSAGE_SRC=<reference>/src BITMESSAGE_HOME=$(mktemp -d) PYTHONDONTWRITEBYTECODE=1 \\
        python tests/golden/make_proc_golden.py

Executed from the reference: ``checkackdata``, ``processgetpubkey`` and ``processonion`` are lifted out of
src/class_objectProcessor.py with ``ast`` (the module imports a node's worth of state), ``checkIPAddress``,
``checkIPv4Address`` and ``checkIPv6Address`` out of src/protocol.py the same way, and run against the reference's
own ``addresses.decodeVarint`` / ``decodeAddress`` / ``encodeAddress``, with stand-ins for ``state``, ``shared``,
``config``, ``queues``, ``knownnodes``, ``sqlExecute``, ``time.time`` and the logger.  The branch of
``objectProcessor.run`` (:72-95) is restated in :func:`main`: the handlers of the three other types need a node.

Two things of Python 2 that the lifted code relies on: ``base64.b32encode`` gives ``str`` there (the stand-in
decodes it), so that ``... .lower() + ".onion"`` works; everything else runs on ``bytes`` as it stands.

The file holds data only: my addresses, the watched keys, and per row of the queue the object's type and bytes
and what the reference did with it: whether a watched key left the dict, the first words of the handler's last
log line, the queued worker command, the ``addKnownNode`` arguments, and the class name of an exception that
escapes to the run loop.  The rows are one queue, run in order against one dict.
"""
import hashlib
import json
import os
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
NOW = 1700000000
INTERVAL = 2419200
GETPUBKEY, PUBKEY, MSG, BROADCAST, ONIONPEER = 0, 1, 2, 3, 0x746f72
LOG_WORDS = 14
MAPPED = bytes(10) + b'\xff\xff'
ONION = bytes.fromhex('fd87d87eeb43')


def blob(name, n):
    """n bytes named by a string."""
    out = b''
    k = 0
    while len(out) < n:
        out += hashlib.sha256(b'proc-kat' + name.encode() + struct.pack('>I', k)).digest()
        k += 1
    return out[:n]


def varint(v):
    if v < 253:
        return struct.pack('>B', v)
    if v < 65536:
        return b'\xfd' + struct.pack('>H', v)
    if v < 4294967296:
        return b'\xfe' + struct.pack('>I', v)
    return b'\xff' + struct.pack('>Q', v)


def head(object_type, name='h'):
    """nonce, expiry time and object type: the 20 bytes every handler skips."""
    return blob(name, 8) + struct.pack('>Q', NOW + 3600) + struct.pack('>I', object_type & 0xffffffff)


def tag_of(version, stream, ripe):
    return hashlib.sha512(hashlib.sha512(varint(version) + varint(stream) + ripe).digest()).digest()[32:]


def main():
    ref_src = os.environ['PYBITMESSAGE_SRC']
    sys.path.insert(0, ref_src)
    import ast
    import binascii
    import base64
    import collections
    import socket
    import threading
    import addresses

    def lift(path, names):
        tree = ast.parse(open(os.path.join(ref_src, path)).read())
        fns = [n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name in names]
        assert sorted(f.name for f in fns) == sorted(names), (path, [f.name for f in fns])
        for f in fns:
            f.decorator_list = []
        return ast.Module(body=fns, type_ignores=[])

    class Log(object):
        def __init__(self):
            self.lines = []

        def debug(self, fmt, *args, **kw):
            self.lines.append(' '.join(fmt.split()[:LOG_WORDS]))
        info = warning = error = critical = debug

    log = Log()

    class Base64Py2(object):
        @staticmethod
        def b32encode(data):
            return base64.b32encode(data).decode('ascii')

    ip_scope = {'socket': socket, 'base64': Base64Py2, 'logger': Log()}
    exec(compile(lift('protocol.py', ['checkIPAddress', 'checkIPv4Address', 'checkIPv6Address']), 'protocol.py', 'exec'),
         ip_scope)

    watch, by_hash, by_tag, settings = {}, {}, {}, {}
    commands, peers = [], []

    class Queue(object):
        def __init__(self, sink):
            self.sink = sink

        def put(self, item):
            self.sink.append(item)

    class Config(object):
        @staticmethod
        def safeGetBoolean(section, key):
            return bool(settings[section][key])

        @staticmethod
        def safeGetInt(section, key):
            return int(settings[section][key])

    class KnownNodes(object):
        knownNodesLock = threading.Lock()

        @staticmethod
        def addKnownNode(stream, peer, is_self=None):
            peers.append([stream, peer.host, peer.port])

    class Translated(object):
        def arg(self, *a):
            return self

    scope = {
        'decodeVarint': addresses.decodeVarint, 'decodeAddress': addresses.decodeAddress,
        'hexlify': binascii.hexlify, 'logger': log,
        'state': type('state', (), {'ackdataForWhichImWatching': watch, 'ownAddresses': {}}),
        'shared': type('shared', (), {'myAddressesByHash': by_hash, 'myAddressesByTag': by_tag}),
        'config': Config, 'queues': type('queues', (), {'workerQueue': Queue(commands), 'UISignalQueue': Queue([])}),
        'knownnodes': KnownNodes, 'Peer': collections.namedtuple('Peer', ['host', 'port']),
        'protocol': type('protocol', (), {'checkIPAddress': staticmethod(ip_scope['checkIPAddress'])}),
        'sqlExecute': lambda *a: None, 'time': type('time', (), {'time': staticmethod(lambda: float(NOW))}),
        '_translate': lambda *a: Translated(), 'l10n': type('l10n', (), {'formatTimestamp': staticmethod(lambda: '')}),
    }
    exec(compile(lift('class_objectProcessor.py', ['checkackdata', 'processgetpubkey', 'processonion']),
                 'class_objectProcessor.py', 'exec'), scope)

    # ---- my addresses (shared.reloadMyAddressHashes, src/shared.py:124-138: both dicts, every version) ----
    addr_rows = []
    for name, version, stream, chan, last in [
            ('a_v2', 2, 1, False, 0), ('a_v3', 3, 1, False, 0), ('a_v4', 4, 1, False, NOW - INTERVAL - 5),
            ('a_v4_chan', 4, 1, True, 0), ('a_v3_recent', 3, 1, False, NOW - INTERVAL + 1),
            ('a_v4_edge', 4, 1, False, NOW - INTERVAL), ('a_v3_s2', 3, 2, False, 0)]:
        ripe = b'\x5a' + blob(name, 19)
        address = addresses.encodeAddress(version, stream, ripe)
        assert addresses.decodeAddress(address) == ('success', version, stream, ripe), name
        by_hash[ripe] = address
        by_tag[tag_of(version, stream, ripe)] = address
        settings[address] = {'chan': chan, 'lastpubkeysendtime': last}
        addr_rows.append({'name': name, 'address': address, 'version': version, 'stream': stream, 'ripe': ripe.hex(),
                          'tag': tag_of(version, stream, ripe).hex(), 'chan': chan, 'last': last})
    A = {r['name']: r for r in addr_rows}

    def ripe(name):
        return bytes.fromhex(A[name]['ripe'])

    def tag(name):
        return bytes.fromhex(A[name]['tag'])

    def getpubkey(body, name='gp'):
        return head(GETPUBKEY, name) + body

    def onion(host, stream=1, port=8444, version=3, name='on'):
        return head(ONIONPEER, name) + varint(version) + varint(stream) + varint(port) + host

    def v4(a, b, c, d):
        return MAPPED + bytes([a, b, c, d])

    def v6(text):
        return socket.inet_pton(socket.AF_INET6, text)

    rows = []

    def row(name, object_type, data):
        rows.append((name, object_type, data))

    # ---- acks, part one ----
    ack38 = head(MSG, 'ack38') + blob('ack38', 34)            # a 54-byte ack object: the legacy 38-byte key
    ack16 = head(MSG, 'ack16') + blob('ack16', 12)            # 32 bytes: a tail of exactly 16
    short31 = head(MSG, 'short31') + blob('short31', 11)      # 31 bytes: never checked, though its tail is watched
    triple = head(MSG, 'triple') + blob('triple', 50)
    prefix_short = head(MSG, 'prefix') + blob('prefix', 20)   # tail 24
    prefix_long = prefix_short + blob('prefix-more', 8)       # tail 32, of which the first 24 are the other key
    last_a = head(BROADCAST, 'last') + blob('last', 33) + b'\x01'
    last_b = last_a[:-1] + b'\x02'
    last_c = last_a[:-1] + b'\x03'                            # not watched
    gp_ack = getpubkey(varint(3) + varint(1) + blob('gp-ack', 20), 'gp-ack')  # not mine, and a watched ack
    unknown_ack = head(7, 'unknown') + blob('unknown', 30)
    pubkey_ack = head(PUBKEY, 'pubkey-ack') + blob('pubkey-ack', 44)
    watched = [ack38[16:], ack16[16:], short31[16:], triple[16:], prefix_short[16:], prefix_long[16:], last_a[16:],
               last_b[16:], gp_ack[16:], unknown_ack[16:], pubkey_ack[16:], blob('never-seen', 38), blob('tiny', 5)]

    row('ack_triple_first', MSG, triple)
    row('ack_38', MSG, ack38)
    row('ack_38_again', MSG, ack38)
    row('ack_16_byte_tail', MSG, ack16)
    row('ack_31_byte_object', MSG, short31)
    row('ack_prefix_long', MSG, prefix_long)
    row('ack_prefix_short', MSG, prefix_short)
    row('ack_last_byte_c', BROADCAST, last_c)
    row('ack_last_byte_b', BROADCAST, last_b)
    row('ack_last_byte_a', BROADCAST, last_a)
    row('ack_not_watched_38', MSG, head(MSG, 'nw') + blob('nw', 34))
    row('ack_on_getpubkey', GETPUBKEY, gp_ack)
    row('ack_on_unknown_type', 7, unknown_ack)
    row('ack_on_pubkey', PUBKEY, pubkey_ack)
    row('unknown_type_i2p', 0x493250, head(0x493250, 'i2p') + blob('i2p', 40))

    # ---- getpubkeys ----
    row('gp_v2_send', GETPUBKEY, getpubkey(varint(2) + varint(1) + ripe('a_v2')))
    row('gp_v3_send', GETPUBKEY, getpubkey(varint(3) + varint(1) + ripe('a_v3')))
    row('gp_v3_send_again', GETPUBKEY, getpubkey(varint(3) + varint(1) + ripe('a_v3'), 'gp2'))
    row('gp_v4_send', GETPUBKEY, getpubkey(varint(4) + varint(1) + tag('a_v4')))
    row('gp_v4_last_on_the_edge', GETPUBKEY, getpubkey(varint(4) + varint(1) + tag('a_v4_edge')))
    row('gp_v3_last_one_above', GETPUBKEY, getpubkey(varint(3) + varint(1) + ripe('a_v3_recent')))
    row('gp_v4_chan', GETPUBKEY, getpubkey(varint(4) + varint(1) + tag('a_v4_chan')))
    row('gp_v3_stream_2_for_stream_1', GETPUBKEY, getpubkey(varint(3) + varint(2) + ripe('a_v3')))
    row('gp_v3_stream_2_send', GETPUBKEY, getpubkey(varint(3) + varint(2) + ripe('a_v3_s2')))
    row('gp_v3_stream_300', GETPUBKEY, getpubkey(varint(3) + varint(300) + ripe('a_v3')))
    row('gp_v3_for_v4_ripe', GETPUBKEY, getpubkey(varint(3) + varint(1) + ripe('a_v4')))
    row('gp_v4_for_v3_tag', GETPUBKEY, getpubkey(varint(4) + varint(1) + tag('a_v3')))
    row('gp_v2_for_v3_ripe', GETPUBKEY, getpubkey(varint(2) + varint(1) + ripe('a_v3')))
    row('gp_v3_not_mine', GETPUBKEY, getpubkey(varint(3) + varint(1) + blob('stranger', 20)))
    row('gp_v4_not_mine', GETPUBKEY, getpubkey(varint(4) + varint(1) + blob('stranger', 32)))
    row('gp_v4_ripe_where_a_tag_goes', GETPUBKEY, getpubkey(varint(4) + varint(1) + ripe('a_v4') + bytes(12)))
    body = varint(3) + varint(1) + ripe('a_v3')
    row('gp_len_200', GETPUBKEY, getpubkey(body + bytes(200 - 20 - len(body))))
    row('gp_len_201', GETPUBKEY, getpubkey(body + bytes(201 - 20 - len(body))))
    row('gp_len_201_bad_varint', GETPUBKEY, getpubkey(b'\xfd\x00\x03' + bytes(201 - 23)))
    row('gp_hash_cut_to_19', GETPUBKEY, getpubkey(body[:-1]))
    row('gp_tag_cut_to_31', GETPUBKEY, getpubkey(varint(4) + varint(1) + tag('a_v4')[:31]))
    row('gp_hash_cut_to_0', GETPUBKEY, getpubkey(varint(3) + varint(1)))
    row('gp_version_only', GETPUBKEY, getpubkey(varint(3)))
    row('gp_version_nonminimal_fd', GETPUBKEY, getpubkey(b'\xfd\x00\x03' + varint(1) + ripe('a_v3')))
    row('gp_version_nonminimal_ff', GETPUBKEY, getpubkey(b'\xff' + struct.pack('>Q', 3) + varint(1) + ripe('a_v3')))
    row('gp_version_truncated_fd', GETPUBKEY, getpubkey(b'\xfd\x01'))
    row('gp_version_truncated_ff', GETPUBKEY, getpubkey(b'\xff' + bytes(7)))
    row('gp_stream_nonminimal_fe', GETPUBKEY, getpubkey(varint(3) + b'\xfe\x00\x00\x00\x01' + ripe('a_v3')))
    row('gp_stream_truncated_fe', GETPUBKEY, getpubkey(varint(3) + b'\xfe\x00\x01'))
    row('gp_version_0', GETPUBKEY, getpubkey(varint(0) + varint(1) + ripe('a_v3')))
    row('gp_version_1', GETPUBKEY, getpubkey(varint(1) + varint(1) + ripe('a_v3')))
    row('gp_version_5', GETPUBKEY, getpubkey(varint(5) + varint(1) + tag('a_v4')))
    row('gp_version_253', GETPUBKEY, getpubkey(varint(253) + varint(1) + tag('a_v4')))
    row('gp_version_max', GETPUBKEY, getpubkey(varint(2 ** 64 - 1) + varint(1) + tag('a_v4')))
    row('gp_version_0_bad_stream', GETPUBKEY, getpubkey(varint(0) + b'\xfd\x00\x01'))
    row('gp_empty', GETPUBKEY, b'')
    row('gp_10_bytes', GETPUBKEY, head(GETPUBKEY)[:10])
    row('gp_20_bytes', GETPUBKEY, head(GETPUBKEY))
    row('ack_triple_second', MSG, triple)

    # ---- onionpeers ----
    for name, host in [('127_0_0_1', v4(127, 0, 0, 1)), ('10_1_2_3', v4(10, 1, 2, 3)), ('192_168_1_1', v4(192, 168, 1, 1)),
                       ('192_169_1_1', v4(192, 169, 1, 1)), ('172_15_0_1', v4(172, 15, 0, 1)), ('172_16_0_1', v4(172, 16, 0, 1)),
                       ('172_31_255_255', v4(172, 31, 255, 255)), ('172_32_0_1', v4(172, 32, 0, 1)),
                       ('8_8_8_8', v4(8, 8, 8, 8)), ('0_0_0_0', v4(0, 0, 0, 0))]:
        row('on_v4_' + name, ONIONPEER, onion(host))
    for name, text in [('loopback', '::1'), ('zero', '::'), ('fe80', 'fe80::1'), ('febf', 'febf::1'), ('fec0', 'fec0::1'),
                       ('fc00', 'fc00::1'), ('fd00', 'fd00::1'), ('fe00', 'fe00::1'), ('global', '2001:db8::1'),
                       ('almost_mapped', '::fffe:808:808')]:
        row('on_v6_' + name, ONIONPEER, onion(v6(text)))
    row('on_onion_6', ONIONPEER, onion(ONION))
    row('on_onion_16', ONIONPEER, onion(ONION + blob('onion', 10)))
    row('on_onion_40', ONIONPEER, onion(ONION + blob('onion3', 34)))
    row('on_onion_prefix_cut_to_5', ONIONPEER, onion(ONION[:5]))
    row('on_mapped_3_tail_bytes', ONIONPEER, onion(MAPPED + b'\x08\x08\x08'))
    row('on_mapped_5_tail_bytes', ONIONPEER, onion(MAPPED + b'\x08\x08\x08\x08\x08'))
    row('on_mapped_no_tail', ONIONPEER, onion(MAPPED))
    row('on_mapped_prefix_cut_to_11', ONIONPEER, onion(MAPPED[:11]))
    row('on_empty_host', ONIONPEER, onion(b''))
    row('on_host_15', ONIONPEER, onion(v6('2001:db8::1')[:15]))
    row('on_host_17', ONIONPEER, onion(v6('2001:db8::1') + b'\x00'))
    row('on_port_9_byte_varint', ONIONPEER, onion(v4(8, 8, 8, 8), port=2 ** 32 + 8444))
    row('on_port_max', ONIONPEER, onion(v6('2001:db8::2'), port=2 ** 64 - 1))
    row('on_stream_3_byte_varint', ONIONPEER, onion(v4(9, 9, 9, 9), stream=1000, version=70000))
    row('on_ends_behind_stream', ONIONPEER, head(ONIONPEER) + varint(3) + varint(1))
    row('on_20_bytes', ONIONPEER, head(ONIONPEER))
    row('on_empty', ONIONPEER, b'')
    row('on_version_nonminimal', ONIONPEER, head(ONIONPEER) + b'\xfd\x00\x03' + varint(1) + varint(8444) + v4(8, 8, 8, 8))
    row('on_stream_truncated', ONIONPEER, head(ONIONPEER) + varint(3) + b'\xfd\x01')
    row('on_port_nonminimal', ONIONPEER, head(ONIONPEER) + varint(3) + varint(1) + b'\xfe\x00\x00\x20\xfc' + v4(8, 8, 8, 8))
    row('on_port_truncated', ONIONPEER, head(ONIONPEER) + varint(3) + varint(1) + b'\xff\x00\x00\x00\x01')
    row('on_long_onion_host', ONIONPEER, onion(ONION + blob('long', 300)))
    row('ack_triple_third', MSG, triple)

    # ---- the run (objectProcessor.run, src/class_objectProcessor.py:64-110) ----
    watch.update((k, i) for i, k in enumerate(watched))
    out = []
    for name, object_type, data in rows:
        before = len(watch)
        del log.lines[:], commands[:], peers[:]
        scope['checkackdata'](data)
        rec = {'name': name, 'type': object_type, 'data': data.hex(), 'ack_left': len(watch) < before,
               'ack_log': log.lines[-1] if log.lines else None, 'log': None, 'command': None, 'peer': None,
               'exception': None}
        del log.lines[:]
        try:
            if object_type == GETPUBKEY:
                scope['processgetpubkey'](data)
            elif object_type == ONIONPEER:
                scope['processonion'](data)
            elif object_type not in (PUBKEY, MSG, BROADCAST):
                log.info("Don't know how to handle object type 0x%08X", object_type)  # :88-91
        except addresses.varintDecodeError:
            rec['exception'] = 'varintDecodeError'
        except Exception as e:  # the run loop's last handler (:106-109)
            rec['exception'] = type(e).__name__
        rec['log'] = log.lines[-1] if log.lines else None
        if commands:
            (command, arg), = commands
            rec['command'] = [command, arg.hex() if isinstance(arg, bytes) else arg]
        if peers:
            rec['peer'], = peers
        out.append(rec)
        print('%-34s ack=%-5s %s' % (name, rec['ack_left'], rec['command'] or rec['peer'] or rec['exception'] or rec['log']))
    assert len(out) > 64

    with open(os.path.join(HERE, 'proc_kats.json'), 'w') as f:
        top = {'source': 'reference checkackdata / processgetpubkey / processonion (class_objectProcessor.py) and '
                         'checkIPAddress / checkIPv4Address / checkIPv6Address (protocol.py), lifted; '
                         'addresses.decodeVarint / decodeAddress / encodeAddress',
               'now': NOW, 'log_words': LOG_WORDS, 'addresses': addr_rows, 'watch': [k.hex() for k in watched],
               'watch_left': sorted(k.hex() for k in watch)}
        f.write(json.dumps(top)[:-1] + ', "rows": [\n')  # one row per line
        f.write(',\n'.join(json.dumps(r, separators=(',', ':')) for r in out) + '\n]}\n')
    print('wrote proc_kats.json (%d rows)' % len(out))


if __name__ == '__main__':
    main()
