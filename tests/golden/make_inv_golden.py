#!/usr/bin/env python3
"""Generate tests/golden/inv_kats.json -- `inv` / `dinv` / `getdata` fixtures judged by the REFERENCE's own code
(needs a read-only checkout of the reference; its ``src`` directory is named by PYBITMESSAGE_SRC, the
environment of make_intake_golden.py):

    PYBITMESSAGE_SRC=<reference>/src BITMESSAGE_HOME=$(mktemp -d) PYTHONDONTWRITEBYTECODE=1 \\
        python tests/golden/make_inv_golden.py

Executed from the reference: ``decode_payload_content``, ``decode_payload_varint``, ``_command_inv`` and
``bm_command_getdata`` are lifted out of src/network/bmproto.py with ``ast`` (the module imports a node's worth
of state), ``handleReceivedInventory`` out of src/network/objectracker.py the same way, and run as methods of a
bare object against the reference's own ``addresses.decodeVarint`` and ``network.constants.MAX_OBJECT_COUNT``,
with stand-ins for ``Inventory()``, ``Dandelion()``, ``state`` and ``missingObjects``.  The payloads are
``bytes``; ``str`` in the lifted code, which Python 2 applied to a byte string, is the identity here.

The file holds data only: per case the payloads' specs, the initial contents of both sets, and from the
reference the items' lengths, the exception's name and the final ``missingObjects`` keys.  Items are named by
number: item k is ``SHA256(b'inv-kat' || SEED || k)`` (:func:`item`); runs of them are ``[first, count]``,
the final keys included.
"""
import hashlib
import json
import os
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 20250620
KINDS = ('inv', 'dinv', 'getdata')


def item(k):
    return hashlib.sha256(b'inv-kat' + struct.pack('>QQ', SEED, k)).digest()


def runs_to_ids(runs):
    return [k for first, count in runs for k in range(first, first + count)]


def regen_payload(pkt):
    """A packet's payload from its spec (shared with the tests): the count's bytes as spelled, the items, then
    ``extra`` zero bytes; ``cut`` keeps a prefix."""
    data = bytes.fromhex(pkt['head']) + b''.join(item(k) for k in runs_to_ids(pkt['items'])) + bytes(pkt.get('extra', 0))
    return data if pkt.get('cut') is None else data[:pkt['cut']]


def ids_to_runs(ids):
    """Sorted distinct item numbers as ``[first, count]`` runs (:func:`runs_to_ids` undoes it)."""
    out = []
    for k in ids:
        if out and out[-1][0] + out[-1][1] == k:
            out[-1][1] += 1
        else:
            out.append([k, 1])
    return out


def lengths_to_runs(lens):
    out = []
    for n in lens:
        if out and out[-1][0] == n:
            out[-1][1] += 1
        else:
            out.append([n, 1])
    return out


def varint(v):
    if v < 253:
        return struct.pack('>B', v)
    if v < 65536:
        return b'\xfd' + struct.pack('>H', v)
    if v < 4294967296:
        return b'\xfe' + struct.pack('>I', v)
    return b'\xff' + struct.pack('>Q', v)


def main():
    ref_src = os.environ['PYBITMESSAGE_SRC']
    sys.path.insert(0, ref_src)
    import ast
    import threading
    import time
    import addresses
    from network.constants import MAX_OBJECT_COUNT

    def lift(path, names):
        tree = ast.parse(open(os.path.join(ref_src, path)).read())
        fns = [n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name in names]
        assert sorted(f.name for f in fns) == sorted(names), (path, [f.name for f in fns])
        for f in fns:
            f.decorator_list = []
        return ast.Module(body=fns, type_ignores=[])

    class BMProtoInsufficientDataError(Exception):
        pass

    class BMProtoExcessiveDataError(Exception):
        pass

    class Quiet(object):
        def debug(self, *args):
            pass
        error = info = debug

    class Stem(object):
        """Dandelion(): no stem objects."""
        def hasHash(self, h):
            return False

        def addHash(self, h, source):
            pass

    have, missing = set(), {}
    state = type('state', (), {'dandelion': 0})
    scope = {'addresses': addresses, 'struct': struct, 'time': time, 'logger': Quiet(), 'state': state,
             'Inventory': lambda: have, 'Dandelion': Stem, 'missingObjects': missing, 'haveBloom': False,
             'MAX_OBJECT_COUNT': MAX_OBJECT_COUNT, 'BMProtoInsufficientDataError': BMProtoInsufficientDataError,
             'BMProtoExcessiveDataError': BMProtoExcessiveDataError, 'str': bytes}
    exec(compile(lift('network/bmproto.py', ['decode_payload_content', 'decode_payload_varint', '_command_inv',
                                             'bm_command_getdata']), 'bmproto.py', 'exec'), scope)
    exec(compile(lift('network/objectracker.py', ['handleReceivedInventory']), 'objectracker.py', 'exec'), scope)
    decode = scope['decode_payload_content']
    seen = []

    def recording_decode(self, pattern='v'):
        items = decode(self, pattern)
        seen.append(items)
        return items

    Proto = type('Proto', (object,), {
        'decode_payload_content': recording_decode, 'decode_payload_varint': scope['decode_payload_varint'],
        '_command_inv': scope['_command_inv'], 'bm_command_getdata': scope['bm_command_getdata'],
        'handleReceivedInventory': scope['handleReceivedInventory']})

    cases = []

    def case(name, pkts, have0=(), missing0=(), dandelion=False):
        have.clear(), missing.clear()
        have.update(item(k) for k in runs_to_ids(have0))
        missing.update((item(k), 0.0) for k in runs_to_ids(missing0))
        state.dandelion = 1 if dandelion else 0
        out = []
        for pkt in pkts:
            payload = regen_payload(pkt)
            p = Proto()
            p.payload, p.payloadOffset, p.payloadLength = payload, 0, len(payload)
            p.skipUntil, p.pendingUpload = 0, {}
            p.objectsNewToThem, p.objectsNewToMe, p.objectsNewToThemLock = {}, {}, threading.RLock()
            del seen[:]
            exc = None
            try:
                {'inv': lambda: p._command_inv(False), 'dinv': lambda: p._command_inv(True),
                 'getdata': p.bm_command_getdata}[pkt['kind']]()
            except (addresses.varintDecodeError, BMProtoExcessiveDataError, BMProtoInsufficientDataError) as e:
                exc = type(e).__name__
            rec = dict(pkt, len=len(payload), sha512=hashlib.sha512(payload).hexdigest(), exception=exc,
                       item_lengths=lengths_to_runs([len(i) for i in seen[0]]) if seen else None)
            if pkt['kind'] == 'getdata':
                rec['pending_upload'] = len(p.pendingUpload)
            out.append(rec)
        ids = {item(k): k for pkt in pkts for k in runs_to_ids(pkt['items'])}
        ids.update((item(k), k) for k in runs_to_ids(missing0))
        final = sorted(missing)
        cases.append({'name': name, 'dandelion': bool(dandelion), 'have': [list(r) for r in have0],
                      'missing': [list(r) for r in missing0], 'packets': out,
                      'missing_final_runs': ids_to_runs(sorted(ids[k] for k in final if k in ids)),
                      'missing_final_other': [k.hex() for k in final if k not in ids]})  # short items, padding
        print('%-34s %s -> %d missing' % (name, ' '.join('%s:%s/%s' % (
            r['kind'], r['exception'], sum(c for _, c in r['item_lengths']) if r['item_lengths'] else '-') for r in out),
            len(final)))
        return cases[-1]

    def pkt(kind, runs, head=None, **kw):
        n = sum(c for _, c in runs)
        return dict({'kind': kind, 'head': (varint(n) if head is None else head).hex(), 'items': [list(r) for r in runs]},
                    **kw)

    # every varint width (minimal), counts 0 and 1
    for kind in KINDS:
        case('%s_count_0' % kind, [pkt(kind, [])], dandelion=True)
        case('%s_count_1' % kind, [pkt(kind, [[1, 1]])], dandelion=True)
    case('inv_empty_payload', [pkt('inv', [], head=b'')])
    case('getdata_empty_payload', [pkt('getdata', [], head=b'')])
    case('inv_count_0_trailing', [pkt('inv', [], extra=40)])
    case('inv_width_1_252', [pkt('inv', [[10, 252]])])
    case('inv_width_3_253', [pkt('inv', [[10, 253]])])
    case('inv_width_3_300', [pkt('inv', [[10, 300]])])
    case('inv_width_5_65536_claimed', [pkt('inv', [[10, 3]], head=varint(65536))])
    case('getdata_width_5_65537_claimed', [pkt('getdata', [[10, 3]], head=b'\xfe\x00\x01\x00\x01')])
    # (a minimal 9-byte count is 2^32 at least: the reference's parser would cut that many items; the 9-byte
    # width is read by the non-minimal and the truncated cases below)
    # the limit
    case('inv_50000', [pkt('inv', [[1000, 50000]])], have0=[[1000, 7], [30000, 100]], missing0=[[2000, 50]])
    for kind in KINDS:
        case('%s_50001' % kind, [pkt(kind, [[1000, 50001]])], dandelion=True)
    case('dinv_50001_dandelion_off', [pkt('dinv', [[1000, 50001]])])
    # every cut length of a 3-item payload
    for cut in range(0, 1 + 96 + 1):
        case('inv_3_items_cut_%d' % cut, [pkt('inv', [[1, 3]], cut=cut)])
    for cut in (0, 1, 2, 3, 34, 35, 36):
        case('inv_300_claimed_cut_%d' % cut, [pkt('inv', [[1, 2]], head=varint(300), cut=cut)])
    # non-minimal and truncated varints
    case('inv_nonminimal_fd', [pkt('inv', [[1, 3]], head=b'\xfd\x00\x03')])
    case('inv_nonminimal_fe', [pkt('inv', [[1, 3]], head=b'\xfe\x00\x00\x01\x00')])
    case('getdata_nonminimal_ff', [pkt('getdata', [[1, 3]], head=b'\xff\x00\x00\x00\x00\x00\x00\x00\x03')])
    case('dinv_nonminimal_dandelion_off', [pkt('dinv', [[1, 3]], head=b'\xfd\x00\x03')])
    case('inv_truncated_fd', [pkt('inv', [], head=b'\xfd\x01')])
    case('inv_truncated_ff', [pkt('inv', [], head=b'\xff\x00\x00\x01')])
    # trailing bytes
    case('inv_trailing_bytes', [pkt('inv', [[1, 3]], extra=17)])
    case('getdata_trailing_item', [pkt('getdata', [[1, 4]], head=varint(3))])
    # dinv with dandelion off and on
    case('dinv_dandelion_off', [pkt('dinv', [[1, 5]])], have0=[[2, 1]])
    case('dinv_dandelion_on', [pkt('dinv', [[1, 5]])], have0=[[2, 1]], dandelion=True)
    # repeated, had and missing items
    case('inv_repeat_inside', [pkt('inv', [[1, 3], [2, 1], [1, 1], [7, 1], [1, 1]])])
    case('inv_repeat_across', [pkt('inv', [[1, 4]]), pkt('inv', [[3, 4]]), pkt('getdata', [[1, 9]]),
                               pkt('dinv', [[6, 3]])], have0=[[4, 1], [8, 1]], dandelion=True)
    case('inv_had_and_missing', [pkt('inv', [[1, 10]])], have0=[[2, 2], [9, 1]], missing0=[[3, 3], [20, 2]])
    case('mixed_flood', [pkt('inv', [[100, 40]]), pkt('inv', [[120, 40]], cut=1 + 32 * 30 + 5), pkt('getdata', [[90, 30]]),
                         pkt('dinv', [[150, 20]]), pkt('inv', [[1, 2]], head=b'\xfd\x00\x02'), pkt('inv', [[130, 60]])],
         have0=[[95, 10], [170, 5]], missing0=[[110, 5]])

    with open(os.path.join(HERE, 'inv_kats.json'), 'w') as f:
        head = {'source': 'reference decode_payload_content / decode_payload_varint / _command_inv / bm_command_getdata '
                          '(bmproto.py) and handleReceivedInventory (objectracker.py), lifted; addresses.decodeVarint; '
                          'network.constants.MAX_OBJECT_COUNT; payloads regenerated by make_inv_golden.regen_payload',
                'seed': SEED, 'max_object_count': MAX_OBJECT_COUNT}
        f.write(json.dumps(head)[:-1] + ', "cases": [\n')  # one case per line
        f.write(',\n'.join(json.dumps(c, separators=(',', ':')) for c in cases) + '\n]}\n')
    print('wrote inv_kats.json (%d cases)' % len(cases))


if __name__ == '__main__':
    main()
