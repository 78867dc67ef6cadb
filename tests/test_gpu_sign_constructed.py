"""The signing kernels on signatures chosen by their r and s: ``sd_sign_kernel`` with k, 1 / k, d, e + r d, s and
the integer sum its addition sees forced to structured values, the device's DER writer (``tx_tail_kernel``) on
r and s of every byte length, the seal and the payload's SHA-512 behind it at every plaintext residue, and
``sd_digits_kernel`` on ephemeral keys with all-zero and all-one windows.  Every expectation is the oracle's
(``oracle/ecdsa_oracle.py``: ``sign_cases``, ``len_grid``), hashlib's or the host's ``sender.seal``;
``tests/test_sign_oracle.py`` shows from integers which defects these rows catch and which they do not.

The receive side (``rxf::der_parse`` in ``rx_walk_kernel`` and the ``rxs_open`` path) is run on real msgs that
``build_msgs`` made under the nonces of ``SHORT_R_NONCES`` with the sender's key fixed: r of 21, 30, 31 and 32
bytes, s wherever it falls, and per nonce one more row whose message was counted up until s has a leading zero
byte.  That gives device-written signatures of 59, 60 and 67 to 72 bytes (asserted below) which must come back
``OK`` from ``open_msgs`` and ``open_sealed_msgs``, and ``BAD_SIGNATURE`` with s ^ 1 or a needless 0x00.  What
cannot be made is a msg that verifies under a chosen s: its plaintext carries the sender's public key, so the
digest depends on d while d = (s k - e) / r depends on the digest.  The lengths 28, 29 and 40 the device writes
in ``build_objects`` are therefore never read back by the device; ``tests/test_sign_oracle.py`` runs the host
build of the same parser on them.  ``signatures.verify_batch_digest`` (test 2) parses on the host
(``sig_parse``), not with ``rxf::der_parse``."""
import collections
import hashlib
import random

import pytest

from oracle import ecdsa_oracle as eo
from pybitmessage_amd import ecies, outgoing, receive, sender, signatures, worker
from pybitmessage_amd.worker import _varint

pytestmark = pytest.mark.gpu

N = eo.N
CODE = {'sha1': signatures.SHA1, 'sha256': signatures.SHA256}
SEALED, CLEAR = outgoing.SEALED, outgoing.CLEAR
FAMILY_COUNTS = {'k': 735, 'kinv': 735, 'd': 735, 't': 1470, 's': 735, 'sum': 39, 'len': 1067}


def b32(v):
    return v.to_bytes(32, 'big')


def digest_int(alg, msg):
    return int.from_bytes(hashlib.new(alg, msg).digest(), 'big')


def check(cases, got):
    """Every row signed as the oracle signs it; a failure names how many rows of which family are not."""
    want = [b32(c.r) + b32(c.s) if c.s else None for c in cases]
    bad = [(c, g) for c, g, w in zip(cases, got, want) if g != w]
    families = sorted(collections.Counter(c.family for c, _ in bad).items())
    assert not bad and len(got) == len(cases), (len(bad), families, [(c.name, g and g.hex()) for c, g in bad[:5]])


def sign_all(cases):
    """One ``sign_digest`` call in which every row reaches the device."""
    sender.reset_stats()
    got = sender.sign_digest([b32(c.d) for c in cases], [b32(c.k) for c in cases], [b32(c.e) for c in cases])
    st = sender.stats()
    assert st['calls'] == 1 and st['rows'] == len(cases)
    return got


# ------------------------------------------------------------------ 1. the equation on every family
def test_sign_digest_on_every_family(gpulib):
    cases = list(eo.sign_cases())
    assert collections.Counter(c.family for c in cases) == FAMILY_COUNTS and len(cases) == 5516
    got = sign_all(cases)
    check(cases, got)
    assert [c.name for c, g in zip(cases, got) if g is None] == ['sum_1']


def test_sign_digest_shuffled_and_across_a_wave_boundary(gpulib):
    cases = list(eo.sign_cases())
    random.Random(51).shuffle(cases)
    check(cases, sign_all(cases))
    by = collections.defaultdict(list)
    for c in eo.sign_cases():
        by[c.family].append(c)
    part = by['sum'][:13] + by['len'][::97][:11] + by['k'][:10] + by['kinv'][:10] + by['t'][:11] + by['s'][:10]
    random.Random(52).shuffle(part)
    assert len(part) == 65 and sum(c.s == 0 for c in part) == 1
    assert collections.Counter(c.family for c in part) == {'sum': 13, 'len': 11, 'k': 10, 'kinv': 10, 't': 11, 's': 10}
    got = sign_all(part)
    check(part, got)
    assert got.count(None) == 1


# ------------------------------------------------------------------ 2. messages: the device's own digest, host DER
MSG_LENGTHS = (0, 55, 56, 64, 147)


@pytest.fixture(scope='module')
def grid():
    return eo.len_grid()


@pytest.mark.parametrize('alg', ['sha1', 'sha256'])
def test_sign_batch_on_every_length_of_r_and_s(gpulib, grid, alg):
    rng = random.Random(53)
    msgs, privs, want = [], [], []
    for j, (nonce, r, s) in enumerate(grid):
        ln = MSG_LENGTHS[j % 5]
        msg = (b'%d:' % j + bytes(rng.randrange(256) for _ in range(ln)))[:ln]
        r2, d = eo.key_from_s(nonce.k, s, digest_int(alg, msg))
        assert r2 == r and d
        msgs.append(msg)
        privs.append(d)
        want.append(eo.der_encode(r, s))
    assert len(grid) == 1067 and {len(m) for m in msgs} == set(MSG_LENGTHS)
    got = sender.sign_batch(msgs, [b32(d) for d in privs], alg, nonces=[b32(n.k) for n, _, _ in grid])
    bad = [(n.name, hex(s)) for (n, _, s), g, w in zip(grid, got, want) if g != w]
    assert not bad, (len(bad), bad[:5])
    assert {len(g) for g in got} == set(range(28, 73))
    pubs = [eo.xy_key(eo.mult_g(d)) for d in privs]
    assert signatures.verify_batch_digest(msgs, got, pubs) == [CODE[alg]] * len(grid)


# ------------------------------------------------------------------ 3. whole objects: the device writes the DER
HEADS = (outgoing.msg_head(1790000000, 1), outgoing.broadcast_head(1790000000, 4, 1, bytes(range(32))))
SHA512_EDGES = (111, 112, 127, 0)  # payload lengths mod 128: the last block's padding with and without room


def object_rows(grid, alg):
    """Per signature length at least 16 rows of the grid (its pairs repeated where there are fewer) under 16
    successive body lengths, the kind and the head turning; then per length one CLEAR row per SHA-512 edge."""
    rng = random.Random(54)
    by_len = collections.defaultdict(list)
    for nonce, r, s in grid:
        by_len[len(eo.der_encode(r, s))].append((nonce, r, s))
    recips = [rng.randrange(1, N) for _ in range(3)]
    ephs = [rng.randrange(1, N) for _ in range(4)]
    rows = []

    def add(kind, head, body_len, nonce, r, s, edge=None):
        body = bytes(rng.randrange(256) for _ in range(body_len))
        d = eo.key_from_s(nonce.k, s, digest_int(alg, head + body))[1]
        assert d
        j = len(rows)
        rows.append(dict(kind=kind, head=head, body=body, d=d, k=nonce.k, r=r, s=s, recip=recips[j % 3], eph=ephs[j % 4],
                         edge=edge, iv=bytes(rng.randrange(256) for _ in range(16))))

    for ln, pairs in sorted(by_len.items()):
        for i in range(max(len(pairs), 16)):
            turn = (i + i // 16) % 4
            add((SEALED, CLEAR)[turn % 2], HEADS[turn // 2], 20 + i % 16, *pairs[i % len(pairs)])
        for j, edge in enumerate(SHA512_EDGES):
            head = HEADS[j % 2]
            add(CLEAR, head, (edge - len(head) - 1 - ln) % 128 + 128, *pairs[j % len(pairs)], edge=edge)
    return rows


@pytest.mark.parametrize('alg', ['sha1', 'sha256'])
def test_build_objects_on_every_length_of_r_and_s(gpulib, grid, alg):
    rows = object_rows(grid, alg)
    assert len(rows) == 1392
    built = outgoing.build_objects(*[[r[c] for r in rows] for c in ('kind', 'head', 'body')], [b32(r['d']) for r in rows],
                                   [eo.xy_key(eo.mult_g(r['recip'])) for r in rows], alg, [b32(r['k']) for r in rows],
                                   [b32(r['eph']) for r in rows], [r['iv'] for r in rows])
    assert built.accepted() == list(range(len(rows)))
    shared = {}
    residues, edges, kinds = collections.defaultdict(set), collections.defaultdict(set), collections.Counter()
    for i, r in enumerate(rows):
        sig = eo.der_encode(r['r'], r['s'])
        assert built.signature(i) == sig, (i, hex(r['r']), hex(r['s']))
        assert built.plain_len[i] == len(r['body']) + 1 + len(sig) and built.digest[i] == sender.DIGESTS[alg]
        plain = r['body'] + _varint(len(sig)) + sig
        if r['kind'] == CLEAR:
            payload = r['head'] + plain
            if r['edge'] is not None:
                edges[len(sig)].add(len(payload) % 128)
        else:
            pair = (r['eph'], r['recip'])
            if pair not in shared:
                x = eo.mult(r['eph'], eo.mult_g(r['recip']))[0]
                shared[pair] = (eo.xy_key(eo.mult_g(r['eph'])), hashlib.sha512(b32(x)).digest())
            payload = r['head'] + sender.seal(plain, r['iv'], *shared[pair])
        assert built.payload(i) == payload, i
        assert built.initial_hash(i) == hashlib.sha512(payload).digest(), i
        residues[len(sig)].add(int(built.plain_len[i]) % 16)
        kinds[r['kind'], len(r['head'])] += 1
    assert sorted(residues) == list(range(28, 73)) and all(v == set(range(16)) for v in residues.values())
    # a sealed payload is head + 118 + 16 m under full-width coordinates, 4 mod 16: only a clear one reaches the edges
    assert sorted(edges) == list(range(28, 73)) and all(v == set(SHA512_EDGES) for v in edges.values())
    assert kinds == {(SEALED, 14): 293, (SEALED, 46): 321, (CLEAR, 14): 395, (CLEAR, 46): 383}
    assert len(shared) == 12


# ------------------------------------------------------------------ 5. ephemeral keys from V
def test_ephemeral_keys_from_the_scalar_set(gpulib):
    rng = random.Random(55)
    V = eo.scalar_set()
    eph = V + [N - v for v in V[:64]]
    n = len(eph)
    assert n == 735 + 64
    recips = [rng.randrange(1, N) for _ in range(3)]
    pubs = [eo.mult_g(d) for d in recips]
    plains = [bytes(rng.randrange(256) for _ in range(j % 41)) for j in range(n)]
    ivs = [bytes(rng.randrange(256) for _ in range(16)) for _ in range(n)]
    prev = sender.set_seal(0)
    try:
        blobs = sender.encrypt_batch(plains, [eo.xy_key(pubs[j % 3]) for j in range(n)], ephemeral=[b32(t) for t in eph], ivs=ivs)
    finally:
        sender.set_seal(prev)
    keys = {}
    bad = []
    for j, t in enumerate(eph):
        pair = (min(t, N - t), j % 3)  # x(t Q) = x((n - t) Q)
        if pair not in keys:
            keys[pair] = hashlib.sha512(b32(eo.mult(t, pubs[j % 3])[0])).digest()
        if blobs[j] != sender.seal(plains[j], ivs[j], eo.xy_key(eo.mult_g(t)), keys[pair]):
            bad.append((j, hex(t)))
    assert not bad, (len(bad), bad[:5])
    # v and n - v: another R (the y differs), the same key material
    for j in range(64):
        i = 735 + j
        assert eo.mult_g(eph[i]) == eo.neg(eo.mult_g(eph[j])) and blobs[i] != blobs[j]
    assert sum(t % 2 == 0 for t in eph) == 343  # the n - t flip of make_odd
    assert ecies.decrypt_batch(blobs, [b32(d) for d in recips]) == [(j % 3, plains[j]) for j in range(n)]


# ------------------------------------------------------------------ 4. the receive side on msgs the device built
SIG_LENGTHS = [59, 60, 67, 68, 69, 70, 71, 72]  # what the 39 msgs reach; 28, 29 and 40 cannot be made (above)
STIFF_UNDER_SHA1 = ('half', 'one', 'two', 'minus_one', 'minus_two')


@pytest.fixture(scope='module')
def built_msgs(gpulib):
    """Real msgs under every nonce of SHORT_R_NONCES and both digests, the sender's key fixed: per nonce one
    row as it comes and one whose message is counted up until s is below 2^248.  Under SHA-1 the digest has 160
    bits, and for k = 1, 2, n - 1, n - 2 and (n + 1) / 2 (1 / k = 2) the top byte of s = (e + r d) / k does not
    move with it: those five searched rows do not exist.  The recipients' ripes are stand-ins (any 20 bytes name
    a recipient), so that every body, and with it every s, is known without the device."""
    from tests.test_gpu_tx import Identity
    rng = random.Random(56)
    me = [Identity(rng, 3), Identity(rng, 4)]
    to = [Identity(rng, 4), Identity(rng, 3)]
    ephs = [rng.randrange(1, N) for _ in range(2)]
    for t in to:
        t.ripe = hashlib.sha1(t.pub_s).digest()
    rows = []
    for alg in ('sha1', 'sha256'):
        part = []
        for j, nonce in enumerate(eo.SHORT_R_NONCES):
            r, kinv = eo.mult_g(nonce.k)[0] % N, pow(nonce.k, -1, N)
            for short in (False, True):
                if short and alg == 'sha1' and nonce.name in STIFF_UNDER_SHA1:
                    continue
                a, b = me[j % 2], to[(j // 2) % 2]
                head = outgoing.msg_head(1790000000, b.stream)
                text = bytes(rng.randrange(256) for _ in range(rng.randrange(60)))
                for tries in range(1 << 16):
                    fields = outgoing.MsgFields(1790000000, b.stream, a.version, a.stream, worker.get_bitfield(), a.pub_s,
                                                a.pub_e, b.ripe, 2, b'%d ' % tries + text, b'', 1000, 1000, a.priv_s, b.pub_e)
                    body = worker.msg_plaintext(a.version, a.stream, fields.bitfield, a.pub_s, a.pub_e, b.ripe, 2,
                                                fields.message, b'', 1000, 1000)
                    s = (digest_int(alg, head + body) + r * a.ks) * kinv % N
                    if s and (not short or s < 2 ** 248):
                        break
                part.append(dict(alg=alg, nonce=nonce, fields=fields, head=head, body=body, r=r, s=s, me=a, to=b,
                                 eph=ephs[len(part) % 2], iv=bytes(rng.randrange(256) for _ in range(16))))
        built = outgoing.build_msgs([p['fields'] for p in part], alg, [b32(p['nonce'].k) for p in part],
                                    [b32(p['eph']) for p in part], [p['iv'] for p in part])
        assert built.accepted() == list(range(len(part)))
        for i, p in enumerate(part):
            p.update(payload=built.payload(i), sig=built.signature(i))
        rows += part
    return rows, to


def reseal(p, plain, cache={}):
    """The msg object of ``plain`` under row p's head, ephemeral key and IV: the key from the oracle's shared x,
    the blob by the host's ``sender.seal``."""
    pair = (p['eph'], p['to'].ke)
    if pair not in cache:
        x = eo.mult(p['eph'], eo.mult_g(p['to'].ke))[0]
        cache[pair] = (eo.xy_key(eo.mult_g(p['eph'])), hashlib.sha512(b32(x)).digest())
    return bytes(8) + p['head'] + sender.seal(plain, p['iv'], *cache[pair])


def needless_pad(r, s, which):
    """The DER of (r, s) with one 0x00 more than the sign needs in front of r (which = 0) or s (1)."""
    ints = [v.to_bytes(v.bit_length() // 8 + 1, 'big') for v in (r, s)]
    ints[which] = b'\x00' + ints[which]
    body = b''.join(b'\x02' + bytes([len(v)]) + v for v in ints)
    return b'\x30' + bytes([len(body)]) + body


def test_built_msgs_open_on_the_receive_side(built_msgs):
    rows, to = built_msgs
    assert len(rows) == 39
    for p in rows:
        assert p['sig'] == eo.der_encode(p['r'], p['s']), p['nonce'].name  # the device's writer on a real msg
        assert p['payload'] == reseal(p, p['body'] + _varint(len(p['sig'])) + p['sig'])[8:], p['nonce'].name
    assert sum(p['s'] < 2 ** 248 for p in rows) == 17 and sum(p['r'] < 2 ** 248 for p in rows) == 19
    objs = [bytes(8) + p['payload'] for p in rows]
    keys = [t.priv_e for t in to]
    got = ecies.decrypt_batch([p['payload'][len(p['head']):] for p in rows], keys)
    assert [g[0] for g in got] == [to.index(p['to']) for p in rows]
    plains = [g[1] for g in got]
    assert plains == [p['body'] + _varint(len(p['sig'])) + p['sig'] for p in rows]
    opened = receive.open_msgs(objs, plains, [p['to'].ripe for p in rows])
    sealed = receive.open_sealed_msgs(objs, ([t.ripe for t in to], keys))
    for res in (opened, sealed):
        assert res.status.tolist() == [receive.OK] * 39
        assert [res.signature(i) for i in range(39)] == [p['sig'] for p in rows]
        assert res.digest.tolist() == [CODE[p['alg']] for p in rows]
        assert [res.fromAddress(i) for i in range(39)] == [p['me'].address for p in rows]
    assert list(sealed.plaintexts) == plains and sealed.match.tolist() == [to.index(p['to']) for p in rows]
    print('signature lengths', sorted({len(p['sig']) for p in rows}))
    assert sorted({len(p['sig']) for p in rows}) == SIG_LENGTHS


def test_tampered_signatures_are_refused_as_the_oracle_predicts(built_msgs):
    """Every built msg again with its signature replaced by (a) ``der_encode(r, s ^ 1)``, canonical but wrong,
    and (b) the same r and s under a needless 0x00 (r and s in turn), the length varint adjusted; the intact
    rows ride in the same calls."""
    rows, to = built_msgs
    objs, plains, ripes, want = [], [], [], []
    for j, p in enumerate(rows):
        signed, key = p['head'] + p['body'], p['me'].pub_s[1:]
        for sig in (p['sig'], eo.der_encode(p['r'], p['s'] ^ 1), needless_pad(p['r'], p['s'], j % 2)):
            code = eo.verify(signed, sig, key)
            plain = p['body'] + _varint(len(sig)) + sig
            objs.append(reseal(p, plain))
            plains.append(plain)
            ripes.append(p['to'].ripe)
            want.append((receive.OK if code else receive.BAD_SIGNATURE, code, sig))
        assert eo.der_decode(needless_pad(p['r'], p['s'], j % 2)) is None
        assert eo.der_decode(eo.der_encode(p['r'], p['s'] ^ 1)) == (p['r'], p['s'] ^ 1)
    assert [w[0] for w in want] == [receive.OK, receive.BAD_SIGNATURE, receive.BAD_SIGNATURE] * 39
    assert [w[1] for w in want[::3]] == [CODE[p['alg']] for p in rows]
    opened = receive.open_msgs(objs, plains, ripes)
    sealed = receive.open_sealed_msgs(objs, ([t.ripe for t in to], [t.priv_e for t in to]))
    for res in (opened, sealed):
        bad = [(i, int(st), w[0]) for i, (st, w) in enumerate(zip(res.status, want)) if st != w[0]]
        assert not bad, bad[:5]
        assert [res.signature(i) for i in range(len(want))] == [w[2] for w in want]
        assert [int(d) for d in res.digest[::3]] == [w[1] for w in want[::3]]
    assert list(sealed.plaintexts) == plains
    assert sorted({len(w[2]) for w in want[2::3]}) == [n + 1 for n in SIG_LENGTHS]
