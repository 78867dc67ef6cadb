"""Msgs, broadcasts and v4 pubkeys from bytes to a final verdict, with no per-object cryptography in Python.

``class_objectProcessor.processmsg`` (``src/class_objectProcessor.py:435-747``) walks a decrypted msg's
fields, checks its signature, and hashes the sender's keys into the ripe and the address.  Behind the
decryption that is one call on the device (:func:`open_msgs`, ``bmpow_rx_msgs``, ``include/bmpow_rx.h``): the
walk, the signed data, both digests, the curve equation, the ripe, the address and ``sigHash`` give one
record per msg whose status names the first line of ``processmsg`` that returns; :func:`process_msgs` puts
:func:`ecies.process_msgs` in front of it.  :func:`open_sealed_msgs` / :func:`process_sealed_msgs` do both in one
library call (``bmpow_rx_sealed_msgs``, ``include/bmpow_rxopen.h``): the matched ciphertexts are decrypted where
the MAC kernel hashed them, into the pool the walk reads, so no ciphertext crosses the bus twice, ``key_e``
never reaches the host and a plaintext crosses once, downwards.

``class_objectProcessor.processbroadcast`` (``src/class_objectProcessor.py:749-973``) and
``protocol.decryptAndCheckPubkeyPayload`` (``src/protocol.py:401-518``) decrypt an object with a key derived
from an address, check its signature, hash the sender's keys into the ripe and compare the ripe (or the tag
made from it) with what the object was encrypted for.  Here each of those steps is one batched call on the
device: :func:`addresses.address_keys`, :func:`ecies.decrypt_batch`, :func:`signatures.verify_batch`,
:func:`addresses.derive_batch`; what stays on the host is slicing and comparing bytes.  No CPU fallback.

The same two functions, and ``processpubkey`` (``src/class_objectProcessor.py:270-433``) for clear v2 / v3
pubkeys, also run behind their decryption as one call on the device (:func:`open_objects`,
``bmpow_rx_objects``), as msgs do: :func:`open_broadcasts` and :func:`open_pubkeys` give one record per object
whose status names the reference line that returns, so "not for me" and "forged" can be told apart.
"""
import collections
import ctypes
import hashlib
import struct

import numpy as np

from . import _lib, addresses, ecies, signatures
from .ecies import _varint

Broadcast = collections.namedtuple('Broadcast', signatures.BroadcastParts._fields + ('fromAddress', 'ripe', 'sigHash'))

# ``processmsg``'s returning lines as ``bmpow_rx_msgs`` names them (BMPOW_RX_*, include/bmpow_rx.h)
OK, MSG_VERSION, NOT_MINE, SENDER_VERSION_0, SENDER_VERSION_HIGH = 0, 1, 2, 3, 4
TOO_SHORT, SENDER_STREAM_0, WRONG_TO_RIPE, VARINT, BAD_SIGNATURE = 5, 6, 7, 8, 9
STATUS_LINES = {OK: None, MSG_VERSION: 444, NOT_MINE: 478, SENDER_VERSION_0: 492, SENDER_VERSION_HIGH: 496,
                TOO_SHORT: 500, SENDER_STREAM_0: 506, WRONG_TO_RIPE: 531, VARINT: 'varint', BAD_SIGNATURE: 566}

MSG_REC = np.dtype([('sender_version', np.uint64), ('sender_stream', np.uint64), ('ntpb', np.uint64),
                    ('extra', np.uint64), ('encoding', np.uint64), ('claimed_stream', np.uint64),
                    ('end_of_pubkey', np.uint32), ('msg_off', np.uint32), ('msg_len', np.uint32),
                    ('ack_off', np.uint32), ('ack_len', np.uint32), ('sig_off', np.uint32), ('sig_len', np.uint32),
                    ('bottom', np.uint32), ('status', np.int32), ('ripe', np.uint8, 20), ('sig_hash', np.uint8, 32),
                    ('addr_len', np.uint8), ('addr', 'S63'), ('behaviour', np.uint8, 4), ('digest', np.uint8),
                    ('prefix_len', np.uint8), ('reserved', np.uint8, 2)])
assert MSG_REC.itemsize == ctypes.sizeof(_lib.BmpowRxMsgRec) == 208

Msg = collections.namedtuple('Msg', [
    'toRipe', 'senderVersion', 'senderStream', 'behaviour', 'nonceTrialsPerByte', 'extraBytes', 'encoding', 'message',
    'ackData', 'signature', 'digest', 'pubkeyData', 'fromAddress', 'ripe', 'sigHash'])


def _decrypt_grouped(payloads, keys):
    """Per payload the plaintext under its own key (``keys[i]``), or None: one ``decrypt_batch`` per
    distinct key, each over the payloads that key is for."""
    groups = collections.OrderedDict()
    for i, k in enumerate(keys):
        groups.setdefault(k, []).append(i)
    out = [None] * len(payloads)
    for key, idx in groups.items():
        for i, r in zip(idx, ecies.decrypt_batch([payloads[i] for i in idx], [key])):
            if r is not None:
                out[i] = r[1]
    return out


def process_broadcasts(objects, subscriptions):
    """``processbroadcast`` for a batch: per object None, or a :class:`Broadcast` -- the fields of
    :func:`signatures.broadcast_signed_parts` with ``fromAddress``, ``ripe`` and ``sigHash =
    sha512(sha512(signature))[32:]`` -- where the reference would go on to store the sender's pubkey and
    the message.  ``subscriptions`` are the address strings of ``reloadBroadcastSendersForWhichImWatching``
    (``src/shared.py:150-184``); one that does not decode is skipped.

    None where the reference returns: a broadcast version other than 4 or 5 (``:760``), a v4 broadcast no
    v2 / v3 subscription key decrypts (``:801``), a v5 tag that is not subscribed (``:810``) or whose key
    does not decrypt (``:820``), the extractor's refusals, a ripe (``:882``) or tag (``:893``) that is not
    the one the broadcast was encrypted for, or a signature that does not verify (``:916``)."""
    objs = [bytes(o) for o in objects]
    by_ripe, by_tag = collections.OrderedDict(), {}
    for status, version, _stream, _ripe, lookup, priv in addresses.address_keys(subscriptions):
        if status == 'success':
            (by_ripe if version <= 3 else by_tag).setdefault(lookup, priv)
    heads = [signatures.broadcast_header(o) for o in objs]
    plain = [None] * len(objs)
    to_ripe = [None] * len(objs)
    # v5: the tag names the one key
    v5 = [i for i, h in enumerate(heads) if h is not None and h[0] == 5 and h[2] in by_tag]
    for i, p in zip(v5, _decrypt_grouped([objs[i][heads[i][3]:] for i in v5], [by_tag[heads[i][2]] for i in v5])):
        plain[i] = p
    # v4: every v2 / v3 key against every payload; the key that opens it names the ripe
    v4 = [i for i, h in enumerate(heads) if h is not None and h[0] == 4]
    if v4 and by_ripe:
        ripes = list(by_ripe)
        for i, r in zip(v4, ecies.decrypt_batch([objs[i][heads[i][3]:] for i in v4], [by_ripe[r] for r in ripes])):
            if r is not None:
                to_ripe[i], plain[i] = ripes[r[0]], r[1]
    parts = [signatures.broadcast_signed_parts(o, p) if p is not None else None for o, p in zip(objs, plain)]
    # a key slice cut short by the end of the plaintext: the reference hashes the short bytes into a ripe
    # that is not the subscribed one, and returns at :882 / :893
    live = [i for i, p in enumerate(parts)
            if p is not None and len(p.pubSigningKey64) == 64 and len(p.pubEncryptionKey64) == 64]
    out = [None] * len(objs)
    if not live:
        return out
    ok = signatures.verify_batch([parts[i].signedData for i in live], [parts[i].signature for i in live],
                                 [parts[i].pubSigningKey64 for i in live])
    ident = addresses.derive_batch([parts[i].pubSigningKey64 for i in live], [parts[i].pubEncryptionKey64 for i in live],
                                   [parts[i].senderVersion for i in live], [parts[i].senderStream for i in live])
    for j, i in enumerate(live):
        ripe = ident.ripe[j].tobytes()
        if heads[i][0] == 4:
            same = to_ripe[i] == ripe
        else:
            same = ident.tag[j].tobytes() == heads[i][2]
        if same and ok[j]:
            sig_hash = hashlib.sha512(hashlib.sha512(parts[i].signature).digest()).digest()[32:]
            out[i] = Broadcast(*(tuple(parts[i]) + (ident.address(j), ripe, sig_hash)))
    return out


def check_pubkeys_v4(objects, addrs):
    """``decryptAndCheckPubkeyPayload(data, address)`` for pairs: per pair the ``storedData`` the reference
    inserts into its pubkeys table (``src/protocol.py:421``, ``:477``), or None where it returns
    ``'failed'``: an address version or stream other than the object's (``:423``, ``:428``), a tag that is
    not the address's (the reference finds no such entry in ``neededPubkeys``, or one for another address,
    ``:442-454``; an address below version 4 has no tag), a payload its key does not decrypt (``:457``), a
    varint that raises, a signature that does not verify (``:484``), or keys whose ripe is not the
    address's (``:497``)."""
    objs = [bytes(o) for o in objects]
    if len(objs) != len(addrs):
        raise ValueError('one address per object')
    keys = addresses.address_keys(addrs)
    heads = [signatures.pubkey_v4_header(o) for o in objs]  # (addressVersion, stream, tag, payloadOffset)
    want = [i for i, (h, k) in enumerate(zip(heads, keys))
            if h is not None and k[0] == 'success' and k[1] >= 4 and k[1] == h[0] and k[2] == h[1] and h[2] == k[4]]
    plain = _decrypt_grouped([objs[i][heads[i][3]:] for i in want], [keys[i][5] for i in want])
    parts = {i: signatures.pubkey_v4_signed_parts(objs[i], p) for i, p in zip(want, plain) if p is not None}
    live = [i for i in want if parts.get(i) is not None and len(parts[i].pubSigningKey64) == 64 and
            len(parts[i].pubEncryptionKey64) == 64]
    out = [None] * len(objs)
    if not live:
        return out
    ok = signatures.verify_batch([parts[i].signedData for i in live], [parts[i].signature for i in live],
                                 [parts[i].pubSigningKey64 for i in live])
    ident = addresses.derive_batch([parts[i].pubSigningKey64 for i in live], [parts[i].pubEncryptionKey64 for i in live],
                                   [keys[i][1] for i in live], [keys[i][2] for i in live])
    for j, i in enumerate(live):
        if ok[j] and ident.ripe[j].tobytes() == keys[i][3]:
            out[i] = parts[i].storedData
    return out


def _encryption_key(signed, key64):
    """The 64 bytes behind the signing key in the signed data of a msg (``obj[8:20] || varint(1) ||
    varint(stream) || varint(senderVersion) || varint(senderStream) || behaviour || keys``) or a v2 / v3
    pubkey (``obj[8:20] || varint(version) || varint(stream) || behaviour || keys``)."""
    pos = 12
    for walked in range(4):
        v = _varint(signed[pos:pos + 10])
        if v is None:
            break
        pos += v[1]
        if walked in (1, 3) and signed[pos + 4:pos + 68] == key64:
            return signed[pos + 68:pos + 132]
    raise ValueError('not the signed data of a msg or a pubkey with this signing key')


def identify(parts, versions, streams):
    """``(fromAddress, ripe)`` per ``(signedData, signature, pubSigningKey64)`` as
    :func:`signatures.msg_signed_parts` / :func:`signatures.pubkey_v3_signed_parts` return them, for the
    sender's address version and stream (``src/class_objectProcessor.py:311-314``, ``:376-379``,
    ``:586-589``): the encryption key is read behind the signing key in the signed data, the rest is
    :func:`addresses.derive_batch`."""
    parts = list(parts)
    ident = addresses.derive_batch([p[2] for p in parts], [_encryption_key(p[0], p[2]) for p in parts], versions, streams)
    return [(ident.address(i), ident.ripe[i].tobytes()) for i in range(len(parts))]


class OpenedMsgs(object):
    """A batch's records (``bmpow_rx_msg_rec``) beside the plaintexts they index.  The columns ``status``,
    ``digest``, ``senderVersion``, ``senderStream``, ``encoding``, ``nonceTrialsPerByte``, ``extraBytes``,
    ``claimedStream`` and ``behaviour`` are numpy arrays; the accessors slice row ``i``'s plaintext.  The
    walked fields of a row are filled as far as ``processmsg`` gets before it returns; ``ripe``,
    ``fromAddress`` and ``sigHash`` belong to rows whose status is ``OK``."""

    def __init__(self, recs, plaintexts, match=None, ripes=None):
        self.recs, self.plaintexts = recs, plaintexts
        # :func:`open_sealed_msgs` only: per row the index of the key whose MAC verified (-1: none), and the
        # ripes those indices name
        self.match, self._ripes = match, ripes
        self.status, self.digest = recs['status'], recs['digest']
        self.senderVersion, self.senderStream = recs['sender_version'], recs['sender_stream']
        self.encoding, self.behaviour = recs['encoding'], recs['behaviour']
        self.nonceTrialsPerByte, self.extraBytes = recs['ntpb'], recs['extra']
        self.claimedStream = recs['claimed_stream']

    def __len__(self):
        return len(self.recs)

    def _cut(self, i, off, length):
        r = self.recs[i]
        return self.plaintexts[i][int(r[off]):int(r[off]) + int(r[length])]

    def message(self, i):
        return self._cut(i, 'msg_off', 'msg_len')

    def ackData(self, i):
        return self._cut(i, 'ack_off', 'ack_len')

    def signature(self, i):
        return self._cut(i, 'sig_off', 'sig_len')

    def pubkeyData(self, i):
        """``decryptedData[:endOfThePublicKeyPosition]``: what ``:595-601`` stores in the pubkeys table."""
        return self.plaintexts[i][:int(self.recs[i]['end_of_pubkey'])]

    def fromAddress(self, i):
        r = self.recs[i]
        return 'BM-' + bytes(r['addr'])[:int(r['addr_len'])].decode('ascii')

    def ripe(self, i):
        return self.recs[i]['ripe'].tobytes()

    def sigHash(self, i):
        return self.recs[i]['sig_hash'].tobytes()

    def toRipe(self, i):
        """The ripe of the key that opened row ``i`` (``:471``), None where no key's MAC verified; for batches
        of :func:`open_sealed_msgs`."""
        if self.match is None:
            raise ValueError('only a batch of open_sealed_msgs knows its keys')
        return self._ripes[int(self.match[i])] if self.match[i] >= 0 else None

    def accepted(self):
        """The rows ``processmsg`` would go on with at ``:582``."""
        return [int(i) for i in np.flatnonzero(self.status == OK)]


def _msg_inputs(objects, plaintexts, to_ripes):
    objs = [o if type(o) is bytes else bytes(o) for o in objects]
    plains = [p if type(p) is bytes else bytes(p) for p in plaintexts]
    ripes = [r if type(r) is bytes else bytes(r) for r in to_ripes]
    if not (len(objs) == len(plains) == len(ripes)):
        raise ValueError('one plaintext and one toRipe per object')
    if any(len(r) != 20 for r in ripes):
        raise ValueError('a toRipe is 20 bytes')
    return objs, plains, ripes


def open_msgs(objects, plaintexts, to_ripes):
    """``processmsg`` from ``:441`` to ``:591`` for decrypted msgs, in one call on the device
    (``bmpow_rx_msgs``): per (object, plaintext, ripe of the key that decrypted it) the field walk, the
    signature check over ``data[8:20] + varint(1) + varint(stream) + plaintext[:bottomOfAckData]``, the
    sender's ripe and address and ``sigHash``, as an :class:`OpenedMsgs`.  ``status`` is the first line
    that returns (``STATUS_LINES``)."""
    objs, plains, ripes = _msg_inputs(objects, plaintexts, to_ripes)
    n = len(objs)
    recs = np.zeros(n, dtype=MSG_REC)
    if n == 0:
        return OpenedMsgs(recs, plains)
    lib = _lib.get()
    op = (ctypes.c_char_p * n)(*objs)
    pp = (ctypes.c_char_p * n)(*plains)
    ol = np.fromiter(map(len, objs), dtype=np.uint64, count=n)
    pl = np.fromiter(map(len, plains), dtype=np.uint64, count=n)
    _lib.check(lib, lib.bmpow_rx_msgs(n, ctypes.cast(op, ctypes.c_void_p), ol.ctypes.data_as(signatures._P64),
                                      ctypes.cast(pp, ctypes.c_void_p), pl.ctypes.data_as(signatures._P64),
                                      b''.join(ripes), recs.ctypes.data), 'bmpow_rx_msgs')
    return OpenedMsgs(recs, plains)


def walk_msg(obj, plaintext, to_ripe):
    """The walk alone for one msg, on the host by the code the kernel is built from
    (``bmpow_rx_walk_msg``): ``(record, verifiable)`` -- a one-row :class:`OpenedMsgs` whose status is the
    walk's (``OK`` where it reaches ``:566``; no verdict, ripe, address or ``sigHash``), and whether the
    signature is canonical DER with r and s in range and the key's coordinates are below p."""
    objs, plains, ripes = _msg_inputs([obj], [plaintext], [to_ripe])
    lib = _lib.host()
    rec = _lib.BmpowRxMsgRec()
    rc = _lib.check(lib, lib.bmpow_rx_walk_msg(objs[0], len(objs[0]), plains[0], len(plains[0]), ripes[0],
                                                ctypes.byref(rec)), 'bmpow_rx_walk_msg')
    return OpenedMsgs(np.frombuffer(bytes(rec), dtype=MSG_REC).copy(), plains), rc == 1


def process_msgs(objects, keys_by_ripe):
    """``processmsg`` for a batch of msg objects: :func:`ecies.process_msgs` (the decryption loop,
    ``:459-483``), then :func:`open_msgs`.  Per object None, or a :class:`Msg` where the reference reaches
    ``:582``.  ``keys_by_ripe`` maps the ripe of each of the user's addresses to its private encryption key.

    Not done here: the recipient's own higher proof-of-work demand (``:615-629``, needs the config and the
    address book), black and white lists, ``MsgDecode``; see :func:`ack_has_valid_header` for ``:725``."""
    objs = [bytes(o) for o in objects]
    opened = ecies.process_msgs(objs, keys_by_ripe)
    live = [i for i, r in enumerate(opened) if r is not None]
    out = [None] * len(objs)
    if not live:
        return out
    res = open_msgs([objs[i] for i in live], [opened[i][1] for i in live], [opened[i][0] for i in live])
    for j in res.accepted():
        r = res.recs[j]
        out[live[j]] = Msg(opened[live[j]][0], int(r['sender_version']), int(r['sender_stream']), r['behaviour'].tobytes(),
                           int(r['ntpb']), int(r['extra']), int(r['encoding']), res.message(j), res.ackData(j),
                           res.signature(j), int(r['digest']), res.pubkeyData(j), res.fromAddress(j), res.ripe(j),
                           res.sigHash(j))
    return out


class _ArenaPlaintexts(object):
    """The plaintexts of :func:`open_sealed_msgs` as a sequence of bytes, each cut from the call's arena when it
    is asked for; ``b''`` for a row without one."""

    def __init__(self, arena, offs, lens):
        self._arena, self._offs, self._lens = arena, offs, lens

    def __len__(self):
        return len(self._lens)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(len(self)))]
        off, n = int(self._offs[i]), int(self._lens[i])
        return self._arena[off:off + n].tobytes()

    def __iter__(self):
        return (self[i] for i in range(len(self)))

    def __eq__(self, other):
        return list(self) == list(other)

    def __ne__(self, other):
        return not self == other


def _sealed_keys(keys_by_ripe):
    """``(ripes, 32-byte keys)`` of a mapping ripe -> private encryption key, or of a pair ``(ripes, privkeys)``
    of equally long sequences (which may try one key under two ripes)."""
    if hasattr(keys_by_ripe, 'keys'):
        ripes = list(keys_by_ripe)
        privs = [keys_by_ripe[r] for r in ripes]
    else:
        ripes, privs = keys_by_ripe
        ripes, privs = list(ripes), list(privs)
    if len(ripes) != len(privs):
        raise ValueError('one ripe per private key')
    ripes = [r if type(r) is bytes else bytes(r) for r in ripes]
    if any(len(r) != 20 for r in ripes):
        raise ValueError('a ripe is 20 bytes')
    return ripes, [ecies._key32(k) for k in privs]


def open_sealed_msgs(objects, keys_by_ripe):
    """``processmsg`` from ``:441`` to ``:591`` for msg objects as they came off the wire, in one call on the
    device (``bmpow_rx_sealed_msgs``, ``include/bmpow_rxopen.h``): the trial decryption against every key, the
    AES pass of the rows whose MAC verified and everything of :func:`open_msgs` behind it, with no ciphertext
    uploaded twice and no key or plaintext on the host in between.  ``keys_by_ripe`` as for
    :func:`process_msgs` (or a pair ``(ripes, privkeys)``).  Gives an :class:`OpenedMsgs` over every object:
    ``status`` is ``MSG_VERSION`` where the head refuses, ``NOT_MINE`` where no key opens it (``:478``), else
    what :func:`open_msgs` says; ``match[i]`` is the index of the key whose MAC verified (-1: none),
    ``toRipe(i)`` its ripe, ``plaintexts[i]`` the decrypted payload (``b''`` where there is none)."""
    objs = [o if type(o) is bytes else bytes(o) for o in objects]
    ripes, privs = _sealed_keys(keys_by_ripe)
    n = len(objs)
    recs = np.zeros(n, dtype=MSG_REC)
    match = np.full(n, -1, dtype=np.int32)
    offs, lens = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    if n == 0:
        return OpenedMsgs(recs, [], match, ripes)
    lib = _lib.get()
    op = (ctypes.c_char_p * n)(*objs)
    ol = np.fromiter(map(len, objs), dtype=np.uint64, count=n)
    arena = np.empty(max(int(ol.sum()), 1), dtype=np.uint8)  # untouched pages cost nothing
    _lib.check(lib, lib.bmpow_rx_sealed_msgs(n, ctypes.cast(op, ctypes.c_void_p), ol.ctypes.data_as(signatures._P64),
                                             len(privs), b''.join(privs), b''.join(ripes), recs.ctypes.data,
                                             match.ctypes.data, arena.ctypes.data, arena.size, offs.ctypes.data,
                                             lens.ctypes.data), 'bmpow_rx_sealed_msgs')
    return OpenedMsgs(recs, _ArenaPlaintexts(arena, offs, lens), match, ripes)


def process_sealed_msgs(objects, keys_by_ripe):
    """:func:`process_msgs` by way of :func:`open_sealed_msgs`: the same list of :class:`Msg` / None."""
    res = open_sealed_msgs(objects, keys_by_ripe)
    out = [None] * len(res)
    for j in res.accepted():
        r = res.recs[j]
        out[j] = Msg(res.toRipe(j), int(r['sender_version']), int(r['sender_stream']), r['behaviour'].tobytes(),
                     int(r['ntpb']), int(r['extra']), int(r['encoding']), res.message(j), res.ackData(j),
                     res.signature(j), int(r['digest']), res.pubkeyData(j), res.fromAddress(j), res.ripe(j),
                     res.sigHash(j))
    return out


def sealed_plan(obj):
    """What :func:`open_sealed_msgs` does with one object before any key is tried, on the host
    (``bmpow_rx_sealed_plan``): ``(openable, reason, payload_off, body_off, clen)`` with ``reason`` one of
    ``PLAN_OK``, ``PLAN_HEAD`` (the head refuses), ``PLAN_PAYLOAD`` (malformed payload) and ``PLAN_CIPHER`` (the
    ciphertext is empty or no multiple of 16 bytes)."""
    lib = _lib.host()
    obj = obj if type(obj) is bytes else bytes(obj)
    po, bo, cl = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
    reason = ctypes.c_int(0)
    rc = _lib.check(lib, lib.bmpow_rx_sealed_plan(obj, len(obj), ctypes.byref(po), ctypes.byref(bo), ctypes.byref(cl),
                                                  ctypes.byref(reason)), 'bmpow_rx_sealed_plan')
    return rc == 1, reason.value, po.value, bo.value, cl.value


PLAN_OK, PLAN_HEAD, PLAN_PAYLOAD, PLAN_CIPHER = 0, 1, 2, 3


def sealed_stats():
    """The counters of ``bmpow_rx_sealed_msgs`` (``bmpow_rx_sealed_stats``) as a dict."""
    lib = _lib.get()
    st = _lib.BmpowRxSealedStats()
    _lib.check(lib, lib.bmpow_rx_sealed_get_stats(ctypes.byref(st)), 'bmpow_rx_sealed_get_stats')
    return {f: getattr(st, f) for f, _ in st._fields_}


def sealed_reset_stats():
    _lib.get().bmpow_rx_sealed_reset_stats()


def ack_has_valid_header(ackData):
    """``objectProcessor.ackDataHasAValidHeader`` (``src/class_objectProcessor.py:1020-1054``), on the host:
    whether a msg's ackData is one well-formed ``object`` packet, which is what ``:725-731`` asks before the
    acknowledgement is sent on.  One ack at a time, with hashlib; :func:`pybitmessage_amd.packets.check_acks` is
    the same answer for a batch in one device call, and :func:`check_opened_acks` feeds it a batch's acks."""
    ackData = bytes(ackData)
    if len(ackData) < 24:
        return False
    magic, command, length, checksum = struct.unpack('!L12sL4s', ackData[:24])
    if magic != 0xE9BEB4D9:
        return False
    payload = ackData[24:]
    if len(payload) != length or length > 1600100:
        return False
    if checksum != hashlib.sha512(payload).digest()[:4]:
        return False
    return command.rstrip(b'\x00') == b'object'


def check_opened_acks(opened, **intake_parameters):
    """The acknowledgements of a batch's accepted rows through :func:`pybitmessage_amd.packets.check_acks` in one
    call: ``(rows, valid, IntakeResult)`` with ``rows`` = ``opened.accepted()`` (an :class:`OpenedMsgs`), ``valid[j]``
    what ``ackDataHasAValidHeader`` says to row ``rows[j]``'s ackData, and the intake record of the object it
    carries: what ``bm_command_object`` will find when the ack is sent on (``:725-731``)."""
    from . import packets
    rows = opened.accepted()
    valid, res = packets.check_acks([opened.ackData(i) for i in rows], **intake_parameters)
    return rows, valid, res


# ---------------------------------------------------------------------------------------------------------
# Broadcasts and pubkeys in one device call (``bmpow_rx_objects``, include/bmpow_rx.h)
# ---------------------------------------------------------------------------------------------------------
KIND_BROADCAST, KIND_PUBKEY_V4, KIND_PUBKEY = 0, 1, 2
(OBJ_OK, OBJ_VARINT, OBJ_BC_VERSION, OBJ_SENDER_VERSION, OBJ_STREAM_MISMATCH, OBJ_WRONG_RIPE, OBJ_WRONG_TAG,
 OBJ_ENCODING_0, OBJ_BAD_SIGNATURE, OBJ_ADDRESS_VERSION_0, OBJ_ADDRESS_VERSION, OBJ_NEEDS_DECRYPTION, OBJ_TOO_SHORT,
 OBJ_KEY_SHORT, OBJ_NOT_SUBSCRIBED, OBJ_NOT_DECRYPTED, OBJ_NOT_NEEDED, OBJ_ADDRESS_MISMATCH,
 OBJ_V4_TOO_SHORT) = range(19)
# per kind: status -> the reference lines that return with it (``src/class_objectProcessor.py``; for
# ``KIND_PUBKEY_V4`` ``src/protocol.py`` but for 411 and 417, which are ``processpubkey``'s)
OBJ_STATUS_LINES = {
    KIND_BROADCAST: {OBJ_OK: (None,), OBJ_VARINT: ('varint',), OBJ_BC_VERSION: (760,), OBJ_SENDER_VERSION: (830, 838),
                     OBJ_STREAM_MISMATCH: (848,), OBJ_WRONG_RIPE: (882,), OBJ_WRONG_TAG: (893,), OBJ_ENCODING_0: (901,),
                     OBJ_BAD_SIGNATURE: (916,), OBJ_NOT_SUBSCRIBED: (801, 810), OBJ_NOT_DECRYPTED: (820,)},
    KIND_PUBKEY_V4: {OBJ_OK: (None,), OBJ_VARINT: ('varint',), OBJ_BAD_SIGNATURE: (484,), OBJ_WRONG_RIPE: (497,),
                     OBJ_NOT_DECRYPTED: (457,), OBJ_NOT_NEEDED: (417, 442), OBJ_ADDRESS_MISMATCH: (423, 428),
                     OBJ_V4_TOO_SHORT: (411,)},
    KIND_PUBKEY: {OBJ_OK: (None,), OBJ_VARINT: ('varint',), OBJ_ADDRESS_VERSION_0: (283,), OBJ_ADDRESS_VERSION: (287,),
                  OBJ_NEEDS_DECRYPTION: (410,), OBJ_TOO_SHORT: (293, 346), OBJ_KEY_SHORT: (304,),
                  OBJ_BAD_SIGNATURE: (374,)},
}

OBJ_REC = np.dtype([('object_version', np.uint64), ('object_stream', np.uint64), ('sender_version', np.uint64),
                    ('sender_stream', np.uint64), ('ntpb', np.uint64), ('extra', np.uint64), ('encoding', np.uint64),
                    ('payload_off', np.uint32), ('tag_off', np.uint32), ('end_of_pubkey', np.uint32),
                    ('msg_off', np.uint32), ('msg_len', np.uint32), ('sig_off', np.uint32), ('sig_len', np.uint32),
                    ('bottom', np.uint32), ('status', np.int32), ('ripe', np.uint8, 20), ('sig_hash', np.uint8, 32),
                    ('addr_len', np.uint8), ('addr', 'S63'), ('behaviour', np.uint8, 4), ('digest', np.uint8),
                    ('prefix_len', np.uint8), ('kind', np.uint8), ('keys_hashed', np.uint8)])
assert OBJ_REC.itemsize == ctypes.sizeof(_lib.BmpowRxObjRec) == 216


class OpenedObjects(object):
    """A batch's records (``bmpow_rx_obj_rec``) beside the objects and plaintexts they index.  ``status``,
    ``kind``, ``digest``, ``objectVersion``, ``objectStream``, ``senderVersion``, ``senderStream``, ``encoding``,
    ``nonceTrialsPerByte``, ``extraBytes`` and ``behaviour`` are numpy columns; the accessors slice row ``i``'s
    plaintext (the object itself for a clear pubkey).  Walked fields are filled as far as the reference gets
    before it returns; ``ripe``, ``fromAddress`` and ``sigHash`` belong to rows whose status is ``OBJ_OK``."""

    def __init__(self, recs, objects, plaintexts, match=None):
        self.recs, self.objects, self.plaintexts = recs, objects, plaintexts
        # :func:`open_sealed_objects` only: per row the index into the table that opened it (-1: none)
        self.match = match
        self.status, self.kind, self.digest = recs['status'], recs['kind'], recs['digest']
        self.objectVersion, self.objectStream = recs['object_version'], recs['object_stream']
        self.senderVersion, self.senderStream = recs['sender_version'], recs['sender_stream']
        self.encoding, self.behaviour = recs['encoding'], recs['behaviour']
        self.nonceTrialsPerByte, self.extraBytes = recs['ntpb'], recs['extra']

    def __len__(self):
        return len(self.recs)

    def _source(self, i):
        return self.objects[i] if self.recs[i]['kind'] == KIND_PUBKEY else self.plaintexts[i]

    def _cut(self, i, off, length):
        r = self.recs[i]
        return self._source(i)[int(r[off]):int(r[off]) + int(r[length])]

    def message(self, i):
        return self._cut(i, 'msg_off', 'msg_len')

    def signature(self, i):
        return self._cut(i, 'sig_off', 'sig_len')

    def signedData(self, i):
        r = self.recs[i]
        skip = 8 if r['kind'] == KIND_PUBKEY else 0
        return self.objects[i][8:8 + int(r['prefix_len'])] + self._source(i)[skip:skip + int(r['bottom'])]

    def pubkeyData(self, i):
        """A broadcast's ``decryptedData[:endOfPubkeyPosition]``: what ``:930-935`` stores."""
        return self.plaintexts[i][:int(self.recs[i]['end_of_pubkey'])]

    def storedData(self, i):
        """What a pubkey's row of the pubkeys table holds: ``data[20:readPosition]`` of a clear pubkey
        (``:310``, ``:364``), ``data[20:tagOffset] + decryptedData[:endOfKeys]`` of an encrypted one
        (``src/protocol.py:421``, ``:477``)."""
        r = self.recs[i]
        if r['kind'] == KIND_PUBKEY:
            return self.objects[i][20:int(r['end_of_pubkey'])]
        return self.objects[i][20:int(r['tag_off'])] + self.plaintexts[i][:int(r['end_of_pubkey'])]

    def fromAddress(self, i):
        r = self.recs[i]
        return 'BM-' + bytes(r['addr'])[:int(r['addr_len'])].decode('ascii')

    def ripe(self, i):
        return self.recs[i]['ripe'].tobytes()

    def sigHash(self, i):
        return self.recs[i]['sig_hash'].tobytes()

    def accepted(self):
        """The rows the reference would go on to store."""
        return [int(i) for i in np.flatnonzero(self.status == OBJ_OK)]


def _obj_inputs(kinds, objects, plaintexts, expects):
    kinds = [int(k) for k in kinds]
    objs = [o if type(o) is bytes else bytes(o) for o in objects]
    plains = [b'' if p is None else p if type(p) is bytes else bytes(p) for p in plaintexts]
    slots = [bytes(e or b'') for e in expects]
    if not (len(kinds) == len(objs) == len(plains) == len(slots)):
        raise ValueError('one kind, one plaintext and one expected value per object')
    if any(k not in (KIND_BROADCAST, KIND_PUBKEY_V4, KIND_PUBKEY) for k in kinds):
        raise ValueError('a kind is KIND_BROADCAST, KIND_PUBKEY_V4 or KIND_PUBKEY')
    if any(len(e) > 32 for e in slots):
        raise ValueError('an expected ripe is 20 bytes (at most the 32 of its slot)')
    return kinds, objs, plains, [e.ljust(32, b'\x00') for e in slots]


def open_objects(kinds, objects, plaintexts, expects):
    """The raw call (``bmpow_rx_objects``): rows of any kinds in one pass over the device, as an
    :class:`OpenedObjects`.  Per row the kind (``KIND_*``), the object, its decrypted payload (ignored, and may
    be None, for ``KIND_PUBKEY``) and the expected ripe: of the subscription key that opened a v4 broadcast, of
    the address an encrypted pubkey was asked for; unused (None) otherwise."""
    kinds, objs, plains, slots = _obj_inputs(kinds, objects, plaintexts, expects)
    n = len(objs)
    recs = np.zeros(n, dtype=OBJ_REC)
    if n == 0:
        return OpenedObjects(recs, objs, plains)
    lib = _lib.get()
    op = (ctypes.c_char_p * n)(*objs)
    pp = (ctypes.c_char_p * n)(*plains)
    ol = np.fromiter(map(len, objs), dtype=np.uint64, count=n)
    pl = np.fromiter(map(len, plains), dtype=np.uint64, count=n)
    _lib.check(lib, lib.bmpow_rx_objects(n, bytes(kinds), ctypes.cast(op, ctypes.c_void_p), ol.ctypes.data_as(signatures._P64),
                                         ctypes.cast(pp, ctypes.c_void_p), pl.ctypes.data_as(signatures._P64),
                                         b''.join(slots), recs.ctypes.data), 'bmpow_rx_objects')
    return OpenedObjects(recs, objs, plains)


def _walk_objects(kind, objs, plains=None):
    """``bmpow_rx_walk_object`` per object into one record array (host only); ``plains`` None: for an
    encrypted kind the headers alone."""
    lib = _lib.host()
    recs = np.zeros(len(objs), dtype=OBJ_REC)
    view = (_lib.BmpowRxObjRec * len(objs)).from_buffer(recs) if len(objs) else ()
    verifiable = []
    for i, o in enumerate(objs):
        p = None if plains is None else plains[i]
        verifiable.append(_lib.check(lib, lib.bmpow_rx_walk_object(kind, o, len(o), p, 0 if p is None else len(p), None,
                                                                    ctypes.byref(view[i])), 'bmpow_rx_walk_object') == 1)
    return recs, verifiable


def walk_object(kind, obj, plaintext=None):
    """The walk alone for one row, on the host by the code the kernel is built from
    (``bmpow_rx_walk_object``): ``(record, verifiable)`` -- a one-row :class:`OpenedObjects` and whether the
    signature and key would go to the curve kernels as they stand.  With ``plaintext`` None for an encrypted
    kind only the header is walked.  A row whose ``keys_hashed`` is set still awaits the ripe / tag
    comparison, which for a broadcast comes before the status the record shows."""
    kinds, objs, plains, _ = _obj_inputs([kind], [obj], [plaintext], [None])
    recs, verifiable = _walk_objects(kinds[0], objs, None if plaintext is None and kinds[0] != KIND_PUBKEY else plains)
    return OpenedObjects(recs, objs, plains), verifiable[0]


def open_broadcasts(objects, subscriptions):
    """``processbroadcast`` from ``:756`` to ``:926`` for a batch, with a status for every object
    (``OBJ_STATUS_LINES[KIND_BROADCAST]``): the headers on the host (``bmpow_rx_walk_object``), the tag lookup
    for v5 and the trial decryption for v4 as :func:`process_broadcasts` groups them, then one
    :func:`open_objects` over everything that decrypted.  ``subscriptions`` as for :func:`process_broadcasts`."""
    objs = [o if type(o) is bytes else bytes(o) for o in objects]
    n = len(objs)
    by_ripe, by_tag = collections.OrderedDict(), {}
    for status, version, _stream, _ripe, lookup, priv in addresses.address_keys(subscriptions):
        if status == 'success':
            (by_ripe if version <= 3 else by_tag).setdefault(lookup, priv)
    recs, _ = _walk_objects(KIND_BROADCAST, objs)
    plain, expect = [None] * n, [None] * n
    heads = [i for i in range(n) if recs['status'][i] == OBJ_OK]
    tags = {i: objs[i][int(recs['tag_off'][i]):int(recs['payload_off'][i])] for i in heads if recs['object_version'][i] == 5}
    for i, tag in tags.items():
        recs['status'][i] = OBJ_NOT_DECRYPTED if tag in by_tag else OBJ_NOT_SUBSCRIBED
    v5 = [i for i, tag in tags.items() if tag in by_tag]
    for i, p in zip(v5, _decrypt_grouped([objs[i][int(recs['payload_off'][i]):] for i in v5], [by_tag[tags[i]] for i in v5])):
        plain[i] = p
    v4 = [i for i in heads if recs['object_version'][i] == 4]
    for i in v4:
        recs['status'][i] = OBJ_NOT_SUBSCRIBED
    if v4 and by_ripe:
        ripes = list(by_ripe)
        opened = ecies.decrypt_batch([objs[i][int(recs['payload_off'][i]):] for i in v4], [by_ripe[r] for r in ripes])
        for i, r in zip(v4, opened):
            if r is not None:
                expect[i], plain[i] = ripes[r[0]], r[1]
    live = [i for i in range(n) if plain[i] is not None]
    if live:
        res = open_objects([KIND_BROADCAST] * len(live), [objs[i] for i in live], [plain[i] for i in live],
                           [expect[i] for i in live])
        recs[live] = res.recs
    return OpenedObjects(recs, objs, [p or b'' for p in plain])


def open_pubkeys(objects, needed):
    """``processpubkey`` (``:276-428``) for a batch, with a status for every object: clear v2 / v3 pubkeys and
    encrypted v4 ones in the same device call.  ``needed`` is ``state.neededPubkeys``: tag -> address string
    (or a tuple that starts with it) of the v4 addresses whose pubkey is awaited.  A v4 pubkey goes through
    ``:411`` (``OBJ_V4_TOO_SHORT``), ``:417`` (``OBJ_NOT_NEEDED``), the address's version and stream against
    the object's (``OBJ_ADDRESS_MISMATCH``), the decryption under the address's key (``OBJ_NOT_DECRYPTED``)
    and then the device, as ``decryptAndCheckPubkeyPayload`` does."""
    objs = [o if type(o) is bytes else bytes(o) for o in objects]
    n = len(objs)
    recs, _ = _walk_objects(KIND_PUBKEY, objs)
    v4 = [i for i in range(n) if recs['status'][i] == OBJ_NEEDS_DECRYPTION]
    if v4:
        recs[v4] = _walk_objects(KIND_PUBKEY_V4, [objs[i] for i in v4])[0]
    asked = {}
    for i in v4:
        tag = objs[i][int(recs['tag_off'][i]):int(recs['payload_off'][i])]
        if len(objs[i]) < 350:
            recs['status'][i] = OBJ_V4_TOO_SHORT
        elif tag not in needed:
            recs['status'][i] = OBJ_NOT_NEEDED
        else:
            entry = needed[tag]
            asked[i] = (tag, entry if isinstance(entry, str) else entry[0])
    plain, expect = [None] * n, [None] * n
    want = sorted(asked)
    keys = dict(zip(want, addresses.address_keys([asked[i][1] for i in want])))
    for i in list(want):
        status, version, stream, _ripe, lookup, _priv = keys[i]
        if status != 'success' or version != recs['object_version'][i] or stream != recs['object_stream'][i]:
            recs['status'][i] = OBJ_ADDRESS_MISMATCH
        elif lookup != asked[i][0]:  # the entry is another address's: protocol.py:442-454
            recs['status'][i] = OBJ_NOT_NEEDED
        else:
            continue
        want.remove(i)
    for i, p in zip(want, _decrypt_grouped([objs[i][int(recs['payload_off'][i]):] for i in want], [keys[i][5] for i in want])):
        if p is None:
            recs['status'][i] = OBJ_NOT_DECRYPTED
        else:
            plain[i], expect[i] = p, keys[i][3]
    clear = [i for i in range(n) if recs['kind'][i] == KIND_PUBKEY and recs['status'][i] == OBJ_OK]
    live = sorted(clear + [i for i in want if plain[i] is not None])
    if live:
        res = open_objects([int(recs['kind'][i]) for i in live], [objs[i] for i in live], [plain[i] for i in live],
                           [expect[i] for i in live])
        recs[live] = res.recs
    return OpenedObjects(recs, objs, [p or b'' for p in plain])


# ---------------------------------------------------------------------------------------------------------
# Broadcasts and pubkeys from wire bytes in one call (``bmpow_rx_sealed_objects``, include/bmpow_rxobjopen.h)
# ---------------------------------------------------------------------------------------------------------
NEEDED_DECODED, NEEDED_OWN_TAG = 1, 2
PLAN_CLEAR, PLAN_V4_SHORT = 4, 5


class SealedTables(object):
    """The three key tables of :func:`open_sealed_objects` as the library takes them: ``trial`` -- ``(ripes,
    privkeys)`` of the v2 / v3 subscriptions; ``tags`` -- ``(tags, privkeys)`` of the v4+ subscriptions;
    ``needed`` -- ``(tags, privkeys, ripes, versions, streams, flags)`` of ``neededPubkeys``."""

    def __init__(self, trial=((), ()), tags=((), ()), needed=((), (), (), (), (), ())):
        self.trial_ripes, self.trial_privs = [bytes(r) for r in trial[0]], [ecies._key32(k) for k in trial[1]]
        self.tags, self.tag_privs = [bytes(t) for t in tags[0]], [ecies._key32(k) for k in tags[1]]
        self.needed_tags, self.needed_privs = [bytes(t) for t in needed[0]], [ecies._key32(k) for k in needed[1]]
        self.needed_ripes = [bytes(r).ljust(20, b'\x00') for r in needed[2]]
        self.needed_versions, self.needed_streams = [int(v) for v in needed[3]], [int(s) for s in needed[4]]
        self.needed_flags = [int(f) for f in needed[5]]
        if len(self.trial_ripes) != len(self.trial_privs) or len(self.tags) != len(self.tag_privs) or not (
                len(self.needed_tags) == len(self.needed_privs) == len(self.needed_ripes) == len(self.needed_versions) ==
                len(self.needed_streams) == len(self.needed_flags)):
            raise ValueError('the columns of a table are equally long')
        if any(len(r) != 20 for r in self.trial_ripes + self.needed_ripes):
            raise ValueError('a ripe is 20 bytes')
        if any(len(t) != 32 for t in self.tags + self.needed_tags):
            raise ValueError('a tag is 32 bytes')

    def struct(self):
        """``(bmpow_rx_obj_tables, what it points into)``."""
        ver = np.array(self.needed_versions, dtype=np.uint64)
        stream = np.array(self.needed_streams, dtype=np.uint64)
        keep = (ver, stream)
        t = _lib.BmpowRxObjTables(
            len(self.trial_privs), b''.join(self.trial_privs), b''.join(self.trial_ripes),
            len(self.tags), b''.join(self.tags), b''.join(self.tag_privs),
            len(self.needed_tags), b''.join(self.needed_tags), b''.join(self.needed_privs), b''.join(self.needed_ripes),
            ver.ctypes.data, stream.ctypes.data, bytes(self.needed_flags))
        return t, keep


def sealed_tables(subscriptions=(), needed=None):
    """The :class:`SealedTables` of address strings: ``subscriptions`` as for :func:`open_broadcasts`, ``needed`` as
    for :func:`open_pubkeys`.  The addresses are resolved once, by one :func:`addresses.address_keys` over the
    distinct ones."""
    subs = list(subscriptions)
    asked = [(bytes(tag), entry if isinstance(entry, str) else entry[0]) for tag, entry in (needed or {}).items()]
    distinct = list(collections.OrderedDict.fromkeys(subs + [a for _, a in asked]))
    keys = dict(zip(distinct, addresses.address_keys(distinct)))
    by_ripe, by_tag = collections.OrderedDict(), collections.OrderedDict()
    for a in subs:
        status, version, _stream, _ripe, lookup, priv = keys[a]
        if status == 'success':
            (by_ripe if version <= 3 else by_tag).setdefault(lookup, priv)
    cols = ([], [], [], [], [], [])
    for tag, a in asked:
        status, version, stream, ripe, lookup, priv = keys[a]
        good = status == 'success'
        own = good and lookup == tag
        for col, v in zip(cols, (tag, priv if own else b'', ripe if good else b'', version if good else 0,
                                 stream if good else 0, (NEEDED_DECODED if good else 0) | (NEEDED_OWN_TAG if own else 0))):
            col.append(v)
    return SealedTables((list(by_ripe), list(by_ripe.values())), (list(by_tag), list(by_tag.values())), cols)


def open_sealed_tables(kinds, objects, tables):
    """The raw call (``bmpow_rx_sealed_objects``) over tables that are built already (:class:`SealedTables`)."""
    kinds = [int(k) for k in kinds]
    objs = [o if type(o) is bytes else bytes(o) for o in objects]
    if len(kinds) != len(objs):
        raise ValueError('one kind per object')
    n = len(objs)
    recs = np.zeros(n, dtype=OBJ_REC)
    match = np.full(n, -1, dtype=np.int32)
    offs, lens = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    if n == 0:
        return OpenedObjects(recs, objs, [], match)
    if any(not 0 <= k <= 255 for k in kinds):
        raise ValueError('a kind is KIND_BROADCAST or KIND_PUBKEY')
    lib = _lib.get()
    op = (ctypes.c_char_p * n)(*objs)
    ol = np.fromiter(map(len, objs), dtype=np.uint64, count=n)
    arena = np.empty(max(int(ol.sum()), 1), dtype=np.uint8)  # untouched pages cost nothing
    t, keep = tables.struct()
    _lib.check(lib, lib.bmpow_rx_sealed_objects(n, bytes(kinds), ctypes.cast(op, ctypes.c_void_p),
                                                ol.ctypes.data_as(signatures._P64), ctypes.byref(t), recs.ctypes.data,
                                                match.ctypes.data, arena.ctypes.data, arena.size, offs.ctypes.data,
                                                lens.ctypes.data), 'bmpow_rx_sealed_objects')
    del keep
    return OpenedObjects(recs, objs, _ArenaPlaintexts(arena, offs, lens), match)


def open_sealed_objects(kinds, objects, subscriptions=(), needed=None):
    """:func:`open_broadcasts` and :func:`open_pubkeys` for objects as they came off the wire, in one call on the
    device (``bmpow_rx_sealed_objects``, ``include/bmpow_rxobjopen.h``): per object its kind (``KIND_BROADCAST`` or
    ``KIND_PUBKEY``; the call routes a v4 pubkey to ``KIND_PUBKEY_V4`` itself), ``subscriptions`` as for
    :func:`open_broadcasts` and ``needed`` as for :func:`open_pubkeys`.  The head walks, the tag lookups, the trial
    decryption of v4 broadcasts, the one-key decryption of v5 broadcasts and v4 pubkeys (each row under its own
    key, in one launch), the AES pass and everything of :func:`open_objects` happen behind the one library call,
    with no ciphertext uploaded twice and no key or plaintext on the host in between.  Gives an
    :class:`OpenedObjects` whose records, statuses and plaintexts are those of the two compositions, bit for bit;
    ``match[i]`` is the index into the table that opened row ``i`` (-1: none): the v2 / v3 subscriptions in their
    order for a v4 broadcast, the v4+ subscriptions for a v5 broadcast, ``needed``'s entries for a v4 pubkey, each
    counted without addresses that do not decode or that repeat an earlier lookup key."""
    return open_sealed_tables(kinds, objects, sealed_tables(subscriptions, needed))


def open_sealed_broadcasts(objects, subscriptions):
    """:func:`open_broadcasts` in one library call (:func:`open_sealed_objects`)."""
    objs = list(objects)
    return open_sealed_objects([KIND_BROADCAST] * len(objs), objs, subscriptions)


def open_sealed_pubkeys(objects, needed):
    """:func:`open_pubkeys` in one library call (:func:`open_sealed_objects`)."""
    objs = list(objects)
    return open_sealed_objects([KIND_PUBKEY] * len(objs), objs, (), needed)


def sealed_object_plan(kind, obj):
    """What :func:`open_sealed_objects` decides about one object before any table is looked at or key tried, on
    the host (``bmpow_rx_sealed_object_plan``): ``(openable, reason, routed_kind, payload_off, tag_off, body_off,
    clen)`` with ``reason`` one of ``PLAN_OK``, ``PLAN_HEAD``, ``PLAN_PAYLOAD``, ``PLAN_CIPHER``, ``PLAN_CLEAR`` (a
    pubkey that is not version 4) and ``PLAN_V4_SHORT`` (a v4 pubkey below 350 bytes)."""
    lib = _lib.host()
    obj = obj if type(obj) is bytes else bytes(obj)
    po, to, bo, cl = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
    reason, routed = ctypes.c_int(0), ctypes.c_int(0)
    rc = _lib.check(lib, lib.bmpow_rx_sealed_object_plan(int(kind), obj, len(obj), ctypes.byref(routed), ctypes.byref(po),
                                                         ctypes.byref(to), ctypes.byref(bo), ctypes.byref(cl),
                                                         ctypes.byref(reason)), 'bmpow_rx_sealed_object_plan')
    return rc == 1, reason.value, routed.value, po.value, to.value, bo.value, cl.value


def sealed_obj_stats():
    """The counters of ``bmpow_rx_sealed_objects`` (``bmpow_rx_sealed_obj_stats``) as a dict."""
    lib = _lib.get()
    st = _lib.BmpowRxSealedObjStats()
    _lib.check(lib, lib.bmpow_rx_sealed_obj_get_stats(ctypes.byref(st)), 'bmpow_rx_sealed_obj_get_stats')
    return {f: getattr(st, f) for f, _ in st._fields_}


def sealed_obj_reset_stats():
    _lib.get().bmpow_rx_sealed_obj_reset_stats()


def obj_stats():
    """The counters of ``bmpow_rx_objects`` (``bmpow_rx_obj_stats``) as a dict; :func:`stats` stays msgs only."""
    lib = _lib.get()
    st = _lib.BmpowRxStats()
    _lib.check(lib, lib.bmpow_rx_obj_get_stats(ctypes.byref(st)), 'bmpow_rx_obj_get_stats')
    return {f: getattr(st, f) for f, _ in st._fields_}


def obj_reset_stats():
    _lib.get().bmpow_rx_obj_reset_stats()


def stats():
    """The library's msg-processing counters (``bmpow_rx_stats``) as a dict."""
    lib = _lib.get()
    st = _lib.BmpowRxStats()
    _lib.check(lib, lib.bmpow_rx_get_stats(ctypes.byref(st)), 'bmpow_rx_get_stats')
    return {f: getattr(st, f) for f, _ in st._fields_}


def reset_stats():
    _lib.get().bmpow_rx_reset_stats()
