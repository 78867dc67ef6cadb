"""The send side on the GPU (``bmpow_ec_pubkeys``, ``bmpow_ecdsa_sign_digest``, ``bmpow_sig_sign``,
``bmpow_ecies_encrypt``, ``pybitmessage_amd.sender``, ``worker.send_msgs_signed``) against the
reference-made fixture ``tests/golden/send_kats.json`` (tests/golden/make_send_golden.py), the integer
oracle ``oracle/ecdsa_oracle.py`` and the project's own receive path: with the random inputs supplied the
reference's blobs and the oracle's signatures come back bit for bit; with them drawn, everything made is
accepted by ``signatures.verify_batch`` / ``ecies.decrypt_batch`` / ``intake.check_objects``.

One case of the public-key family cannot be run as written: sixteen windows of 0xFFFF are the scalar
2^256 - 1, which is not below the group order, so the library refuses it (``ok = 0``, asserted here) and
the nearest scalar in range, 0xFFFE in the top window and 0xFFFF in the fifteen below, is checked
against ``mult_g`` beside it.  And a blob made for the negated recipient key -Q is opened by the key of Q
as well as by that of -Q: the shared secret is x(t Q) alone, which is x(t (-Q)) -- in pyelliptic as
here -- so ``decrypt_batch`` reports key 0 for it and the test says so."""
import hashlib
import random
import time

import pytest

from oracle import ecdsa_oracle as eo
from pybitmessage_amd import _lib, ecies, intake, sender, signatures, worker

pytestmark = pytest.mark.gpu

P, N = eo.P, eo.N
CODE = {'sha1': signatures.SHA1, 'sha256': signatures.SHA256}


def b32(v):
    return v.to_bytes(32, 'big')


def pub65(k):
    return b'\x04' + eo.xy_key(eo.mult_g(k))


def digest_int(alg, msg):
    return int.from_bytes(hashlib.new(alg, msg).digest(), 'big')


@pytest.fixture(scope='module')
def kats(golden):
    return golden('send_kats.json')


@pytest.fixture(scope='module')
def pool():
    """128 seeded scalars and their public keys by the oracle: shared, never changed."""
    rng = random.Random(77)
    ks = [rng.randrange(1, N) for _ in range(128)]
    return ks, [pub65(k) for k in ks]


@pytest.fixture(scope='module')
def recipients(kats):
    privs = [bytes.fromhex(k) for k in kats['recipient_keys']]
    return privs, [bytes.fromhex(k) for k in kats['recipient_pubs']]


# ------------------------------------------------------------------ public keys
def test_pointmult_kats_in_one_call(gpulib, kats):
    got = sender.priv_to_pub([bytes.fromhex(k['priv']) for k in kats['pointmult_kats']])
    assert got == [bytes.fromhex(k['pub']) for k in kats['pointmult_kats']]


@pytest.mark.parametrize('n', [1, 63, 64, 65])
def test_pubkey_call_sizes(gpulib, pool, n):
    ks, pubs = pool
    for start in (0, 128 - n):
        assert sender.priv_to_pub([b32(k) for k in ks[start:start + n]]) == pubs[start:start + n]


def test_pubkeys_of_structured_scalars(gpulib):
    rng = random.Random(78)
    ks = []
    for i in range(16):  # one nonzero 16-bit window, at every position
        ks += [1 << (16 * i), 0xFFFF << (16 * i), rng.randrange(1, 0xFFFF) << (16 * i)]
    near_top = (1 << 256) - (1 << 240) - 1  # 0xFFFE, then fifteen windows of 0xFFFF
    ks.append(near_top)
    for odd in (0, 1):  # alternating zero windows
        ks.append(sum(rng.randrange(1, 0x10000) << (16 * i) for i in range(16) if i % 2 == odd))
    ks.append(sum(0xFFFF << (16 * i) for i in range(16) if i % 2 == 0))
    assert all(1 <= k < N for k in ks)
    got = sender.priv_to_pub([b32(k) for k in ks] + [b32(2 ** 256 - 1)])
    assert got[:-1] == [pub65(k) for k in ks]
    assert got[-1] is None  # all sixteen windows 0xFFFF: not below n


def test_pubkeys_out_of_range(gpulib, pool):
    ks, pubs = pool
    got = sender.priv_to_pub([b32(ks[0]), b32(0), b32(N), b32(2 ** 256 - 1), b32(ks[1]), b32(N - 1)])
    assert got == [pubs[0], None, None, None, pubs[1], pub65(N - 1)]


# ------------------------------------------------------------------ signing
@pytest.mark.parametrize('alg', ['sha1', 'sha256'])
def test_sign_kats_with_their_nonces(gpulib, kats, alg):
    rows = [k for k in kats['sign_kats'] if k['digest'] == alg]
    assert len(rows) >= 14
    got = sender.sign_batch([bytes.fromhex(k['msg']) for k in rows], [bytes.fromhex(k['priv']) for k in rows], alg,
                            nonces=[bytes.fromhex(k['nonce']) for k in rows])
    assert got == [bytes.fromhex(k['sig']) for k in rows]
    rs = sender.sign_digest([bytes.fromhex(k['priv']) for k in rows], [bytes.fromhex(k['nonce']) for k in rows],
                            [b32(digest_int(alg, bytes.fromhex(k['msg']))) for k in rows])
    assert rs == [bytes.fromhex(k['r'] + k['s']) for k in rows]


@pytest.mark.parametrize('alg', ['sha1', 'sha256'])
def test_sign_message_lengths(gpulib, alg):
    rng = random.Random(79)
    msgs = [bytes(rng.randrange(256) for _ in range(ln)) for ln in (0, 55, 56, 63, 64, 65, 119, 120, 1000)]
    ds = [rng.randrange(1, N) for _ in msgs]
    ks = [rng.randrange(1, N) for _ in msgs]
    want = [eo.der_encode(*eo.sign(d, k, digest_int(alg, m))) for d, k, m in zip(ds, ks, msgs)]
    assert sender.sign_batch(msgs, [b32(d) for d in ds], alg, nonces=[b32(k) for k in ks]) == want


def test_sign_digest_edges(gpulib):
    """x(k G) >= n cannot be constructed; the digest's reduction can: e >= n, e = 0, e all ones."""
    rng = random.Random(80)
    es = [0, N, N + 1, 2 ** 256 - 1, N - 1, rng.getrandbits(256)]
    ds = [rng.randrange(1, N) for _ in es]
    ks = [rng.randrange(1, N) for _ in es]
    got = sender.sign_digest([b32(d) for d in ds], [b32(k) for k in ks], [b32(e) for e in es])
    assert got == [b32(r) + b32(s) for r, s in (eo.sign(d, k, e % N) for d, k, e in zip(ds, ks, es))]
    bad = sender.sign_digest([b32(0), b32(N), b32(ds[0]), b32(ds[0]), b32(ds[0])],
                             [b32(ks[0]), b32(ks[0]), b32(0), b32(N), b32(ks[0])], [b32(es[5])] * 5)
    assert bad[:4] == [None] * 4 and bad[4] == b32(eo.sign(ds[0], ks[0], es[5])[0]) + b32(eo.sign(ds[0], ks[0], es[5])[1])


def test_constructed_s_zero_row_among_its_wave(gpulib):
    rng = random.Random(81)
    msgs = [b'row %d' % i for i in range(64)]
    ds = [rng.randrange(1, N) for _ in msgs]
    ks = [rng.randrange(1, N) for _ in msgs]
    at = 37
    r = eo.mult_g(ks[at])[0] % N
    ds[at] = -digest_int('sha256', msgs[at]) * pow(r, -1, N) % N  # e + r d = 0: s = 0
    got = sender.sign_batch(msgs, [b32(d) for d in ds], 'sha256', nonces=[b32(k) for k in ks])
    assert got[at] is None
    for i in range(64):
        if i != at:
            assert got[i] == eo.der_encode(*eo.sign(ds[i], ks[i], digest_int('sha256', msgs[i]))), i


def test_sign_refuses_keys_and_nonces_out_of_range(gpulib):
    for d, k in ((0, 5), (N, 5), (5, 0), (5, N)):
        with pytest.raises(_lib.BmpowError) as err:
            sender.sign_batch([b'm'], [b32(d)], 'sha256', nonces=[b32(k)])
        assert err.value.code == _lib.E_ARG
    with pytest.raises(_lib.BmpowError):
        sender.sign_batch([b'm'], [b32(0)])


@pytest.mark.parametrize('alg', ['sha1', 'sha256'])
def test_drawn_nonces_differ_and_verify(gpulib, pool, alg):
    ks, pubs = pool
    msgs = [b'drawn nonce %d' % i * (i % 7 + 1) for i in range(65)]
    privs = [b32(k) for k in ks[:65]]
    one, two = sender.sign_batch(msgs, privs, alg), sender.sign_batch(msgs, privs, alg)
    assert all(a is not None and b is not None and a != b for a, b in zip(one, two))
    assert signatures.verify_batch_digest(msgs + msgs, one + two, pubs[:65] + pubs[:65]) == [CODE[alg]] * 130


def test_sign_one(gpulib, pool):
    ks, pubs = pool
    sig = sender.sign(b'one message', b32(ks[3]).hex())
    assert signatures.verify_batch_digest([b'one message'], [sig], [pubs[3]]) == [signatures.SHA256]


# ------------------------------------------------------------------ encryption
def test_encrypt_kats_with_their_ephemeral_keys(gpulib, kats, recipients):
    rows = kats['encrypt_kats']
    got = sender.encrypt_batch([bytes.fromhex(k['plaintext']) for k in rows], [recipients[1][k['recipient']] for k in rows],
                               ephemeral=[bytes.fromhex(k['ephemeral']) for k in rows],
                               ivs=[bytes.fromhex(k['iv']) for k in rows])
    assert got == [bytes.fromhex(k['blob']) for k in rows]
    assert sum(k['coord_lens'] != [32, 32] for k in rows) >= 2


@pytest.mark.parametrize('n', [1, 63, 64, 65])
def test_encrypt_call_sizes_round_trip(gpulib, recipients, n):
    privs, pubs = recipients
    rng = random.Random(82 + n)
    plains = [bytes(rng.randrange(256) for _ in range(rng.choice((0, 1, 15, 16, 17, 100, 333)))) for _ in range(n)]
    to = [rng.randrange(3) for _ in range(n)]
    blobs = sender.encrypt_batch(plains, [b'\x04' + pubs[t] for t in to])
    assert all(len(b) <= sender.blob_cap(len(p)) for b, p in zip(blobs, plains))
    assert ecies.decrypt_batch(blobs, privs) == list(zip(to, plains))


def test_refused_recipient_keys_in_one_wave(gpulib, recipients):
    privs, pubs = recipients
    x, y = eo.key_xy(pubs[0])
    keys = [pubs[i % 3] for i in range(64)]
    keys[5] = b32(x) + b32((y + 1) % P)  # off the curve
    keys[20] = b32(P) + b32(y)           # a coordinate that is not below p
    keys[41] = b32(x) + b32(P - y)       # the negated key: a point of the curve, the key n - d's
    keys[50] = b'\x00' * 63              # no key at all
    plains = [b'plain %d' % i for i in range(64)]
    blobs = sender.encrypt_batch(plains, keys)
    assert [i for i, b in enumerate(blobs) if b is None] == [5, 20, 50]
    # The negated key gets a blob.  ECDH keeps x alone and x(t (-Q)) = x(t Q), so the keys d and n - d
    # derive the same key_e || key_m: the blob is opened by key 0 as by n - d, here as in the reference.
    opened = ecies.decrypt_batch([b for b in blobs if b is not None], privs)
    want = [(0 if i == 41 else i % 3, plains[i]) for i in range(64) if i not in (5, 20, 50)]
    assert opened == want
    owner = b32(N - int.from_bytes(privs[0], 'big'))
    assert ecies.decrypt_batch([blobs[41]], [owner]) == [(0, plains[41])]


def test_encrypt_refuses_an_ephemeral_key_out_of_range(gpulib, recipients):
    for k in (0, N):
        with pytest.raises(_lib.BmpowError) as err:
            sender.encrypt_batch([b'x'], [recipients[1][0]], ephemeral=[b32(k)], ivs=[bytes(16)])
        assert err.value.code == _lib.E_ARG


def test_drawn_ephemeral_keys_differ_and_decrypt(gpulib, recipients):
    privs, pubs = recipients
    plains = [b'the same plaintext'] * 3 + [b'']
    to = [0, 1, 2, 1]
    one = sender.encrypt_batch(plains, [pubs[t] for t in to])
    two = sender.encrypt_batch(plains, [pubs[t] for t in to])
    assert all(a != b and a[:16] != b[:16] for a, b in zip(one, two))
    assert ecies.decrypt_batch(one, privs) == ecies.decrypt_batch(two, privs) == list(zip(to, plains))
    blob = sender.encrypt(b'hexed', (b'\x04' + pubs[2]).hex())
    assert ecies.decrypt_batch([blob], privs) == [(2, b'hexed')]
    with pytest.raises(ValueError):
        sender.encrypt(b'hexed', (b'\x04' + pubs[2][:32] + b32(1)).hex())


# ------------------------------------------------------------------ the set loop
def test_two_sets_in_one_call(gpulib, pool):
    """2^18 + 65 rows: a full set and a second one of 65.  Signing and encryption go through the same loop
    (send_run_locked, bmpow_host_send.hip), so one call covers its set arithmetic."""
    ks, pubs = pool
    n = (1 << 18) + 65
    privs = [b32(k) for k in ks]
    rows = [privs[i % 128] for i in range(n)]
    sender.reset_stats()
    t0 = time.perf_counter()
    got = sender.priv_to_pub(rows)
    wall = time.perf_counter() - t0
    st = sender.stats()
    print('priv_to_pub of %d rows: %.3f s wall, %.1f ms comb kernels, %.1f ms in the library'
          % (n, wall, st['comb_ms'], st['host_ms']))
    assert st['sets'] == 2 and st['rows'] == n and st['calls'] == 1 and st['launches'] == 2
    assert len(got) == n
    for j in range(128):
        assert all(g == pubs[j] for g in got[j::128]), j


def test_counters_of_every_kind_of_call(gpulib, pool, recipients):
    """Three rows per call: calls, sets, rows and launches as the set loop counts them for a signature over
    messages (hash, comb, sign), over digests (comb, sign), and an encryption (comb, digits, prep, shared)
    sealed by the host, by the device, and -- one row above the device's limit -- by both, which is two trips
    through the loop but one call.  The phase times add up to something, and hash_ms is exactly 0 where nothing
    is hashed: the gap between the two events around a hash that was not launched is no hashing time."""
    ks, pubs = pool
    privs = [b32(k) for k in ks[:3]]
    eph = [b32(k) for k in ks[3:6]]
    ivs = [bytes([i]) * 16 for i in range(3)]
    to = recipients[1][:3]
    plains = [b'counted %d' % i for i in range(3)]
    big = [plains[0], bytes((256 << 10) + 1), plains[2]]

    def counted(call, seal=None):
        prev = sender.set_seal(seal) if seal is not None else None
        sender.reset_stats()
        sender.reset_seal_stats()
        try:
            assert all(r is not None for r in call())
        finally:
            if prev is not None:
                sender.set_seal(prev)
        st = sender.stats()
        print({k: st[k] for k in ('calls', 'sets', 'rows', 'launches', 'hash_ms', 'comb_ms', 'scalar_ms', 'ladder_ms')})
        assert st['hash_ms'] + st['comb_ms'] + st['scalar_ms'] + st['ladder_ms'] > 0
        return st, sender.seal_stats()

    st, _ = counted(lambda: sender.sign_batch(plains, privs, 'sha256', nonces=eph))
    assert (st['calls'], st['sets'], st['rows'], st['launches']) == (1, 1, 3, 3) and st['hash_ms'] > 0
    st, _ = counted(lambda: sender.sign_digest(privs, eph, [hashlib.sha256(p).digest() for p in plains]))
    assert (st['calls'], st['sets'], st['rows'], st['launches']) == (1, 1, 3, 2) and st['hash_ms'] == 0
    st, seal = counted(lambda: sender.encrypt_batch(plains, to, ephemeral=eph, ivs=ivs), seal=0)
    assert (st['calls'], st['sets'], st['rows'], st['launches']) == (1, 1, 3, 4) and st['hash_ms'] == 0
    assert seal['launches'] == 0 and seal['rows_device'] == 0
    st, seal = counted(lambda: sender.encrypt_batch(plains, to, ephemeral=eph, ivs=ivs), seal=1)
    assert (st['calls'], st['sets'], st['rows'], st['launches']) == (1, 1, 3, 4) and st['hash_ms'] == 0
    assert seal['launches'] == 1 and seal['rows_device'] == 3
    st, seal = counted(lambda: sender.encrypt_batch(big, to, ephemeral=eph, ivs=ivs), seal=1)
    assert (st['calls'], st['sets'], st['rows'], st['launches']) == (1, 2, 3, 8) and st['hash_ms'] == 0
    assert seal['rows_device'] == 2 and seal['rows_host'] == 1


def test_abort_is_honoured(gpulib, pool, recipients):
    ks, pubs = pool
    gpulib.bmpow_abort()
    try:
        for call in (lambda: sender.priv_to_pub([b32(ks[0])]), lambda: sender.sign_batch([b'm'], [b32(ks[0])]),
                     lambda: sender.encrypt_batch([b'm'], [recipients[1][0]])):
            with pytest.raises(_lib.BmpowError) as e:
                call()
            assert e.value.code == _lib.E_ABORTED
    finally:
        gpulib.bmpow_clear_abort()
    assert sender.priv_to_pub([b32(ks[0])]) == [pubs[0]]


# ------------------------------------------------------------------ the whole send path
def test_send_msgs_signed_through_the_receive_path(gpulib, pool, recipients):
    ks, pubs = pool
    privs, rpubs = recipients
    now = 1760000000
    sign_priv, sign_pub, enc_pub = b32(ks[0]), pubs[0], pubs[1]
    ripes = [hashlib.sha1(p).digest() for p in rpubs[:2]]  # stand-ins: any 20 bytes identify a recipient here
    x, y = eo.key_xy(rpubs[2])
    seen = {}

    def build_plain(ctx, ack):
        seen[ctx['name']] = ack
        plain = worker.msg_plaintext(4, 1, worker.get_bitfield(), sign_pub, enc_pub, ctx['ripe'], 2,
                                     b'Subject:hello\nBody:' + ctx['name'].encode() * 20, ack, 10, 10)
        return plain, sign_priv, ctx['key'], 4, 1, 4 * 24 * 3600, 10, 10

    rng = random.Random(83)
    ackdata = [b'\x00\x00\x00\x02\x01\x01' + bytes(rng.randrange(256) for _ in range(32)) for _ in range(2)]
    jobs = [(ackdata[0], 4 * 24 * 3600, {'name': 'to_a', 'ripe': ripes[0], 'key': b'\x04' + rpubs[0]}),
            (None, 4 * 24 * 3600, {'name': 'to_b_no_ack', 'ripe': ripes[1], 'key': rpubs[1]}),
            (ackdata[1], 4 * 24 * 3600, {'name': 'bad_key', 'ripe': ripes[1], 'key': b32(x) + b32((y + 1) % P)})]
    # the recipients ask for the test-mode difficulty (10, 10); the sender works to the network minimum, which
    # is what the intake holds every object to whatever lower demand it is given
    out = worker.send_msgs_signed(jobs, build_plain, rng=random.Random(84), now=now)
    assert out[2] is None and out[0] is not None and out[1] is not None
    assert seen['to_b_no_ack'] == b'' and len(seen['to_a']) > 24 and len(seen['bad_key']) > 24
    objs = out[:2]
    # intake at the test-mode difficulty
    res = intake.check_objects(objs, streams=(1,), nonceTrialsPerByte=10, payloadLengthExtraBytes=10, now=now)
    assert list(res.status) == [intake.OK, intake.OK]
    assert list(res.objectType) == [worker.OBJECT_MSG] * 2
    # the recipients' keys open them, each its own
    opened = ecies.process_msgs(objs, {ripes[0]: privs[0], ripes[1]: privs[1]})
    assert [o[0] for o in opened] == ripes
    # the signatures verify under SHA-256 over the same embeddedTime the object carries
    parts = [signatures.msg_signed_parts(o, p[1]) for o, p in zip(objs, opened)]
    assert all(p is not None and p[2] == sign_pub[1:] for p in parts)
    assert signatures.verify_batch_digest([p[0] for p in parts], [p[1] for p in parts], [p[2] for p in parts]) \
        == [signatures.SHA256] * 2
    for o, p, name in zip(objs, opened, ('to_a', 'to_b_no_ack')):
        unsigned = worker.msg_plaintext(4, 1, worker.get_bitfield(), sign_pub, enc_pub, ripes[0 if name == 'to_a' else 1], 2,
                                        b'Subject:hello\nBody:' + name.encode() * 20, seen[name], 10, 10)
        assert p[1].startswith(unsigned)
    # the embedded ack is a finished object packet of its own
    ack = seen['to_a']
    assert ack[:4] == b'\xe9\xbe\xb4\xd9' and ack[4:10] == b'object'
    ack_res = intake.check_objects([ack[24:]], streams=(1,), now=now)
    assert list(ack_res.status) == [intake.OK]
    assert ack[24 + 8 + 8:] == ackdata[0]
