"""Broadcasts and v4 pubkeys from bytes to a final verdict, with no per-object cryptography in Python.

``class_objectProcessor.processbroadcast`` (``src/class_objectProcessor.py:749-973``) and
``protocol.decryptAndCheckPubkeyPayload`` (``src/protocol.py:401-518``) decrypt an object with a key derived
from an address, check its signature, hash the sender's keys into the ripe and compare the ripe (or the tag
made from it) with what the object was encrypted for.  Here each of those steps is one batched call on the
device: :func:`addresses.address_keys`, :func:`ecies.decrypt_batch`, :func:`signatures.verify_batch`,
:func:`addresses.derive_batch`; what stays on the host is slicing and comparing bytes.  No CPU fallback.
"""
import collections
import hashlib

from . import addresses, ecies, signatures
from .ecies import _varint

Broadcast = collections.namedtuple('Broadcast', signatures.BroadcastParts._fields + ('fromAddress', 'ripe', 'sigHash'))


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
