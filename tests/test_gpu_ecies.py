"""ECIES trial decryption on the GPU (``bmpow_ecdh``, ``bmpow_ecies_match``, ``pybitmessage_amd.ecies``)
against the reference-made fixture ``tests/golden/ecies_kats.json`` (pyelliptic over OpenSSL,
tests/golden/make_ecies_golden.py) and against payloads built here with hashlib / hmac from the
fixture's (key, point, shared x) triples."""
import ctypes
import hashlib
import hmac
import random
import struct

import pytest

from pybitmessage_amd import _lib, ecies

pytestmark = pytest.mark.gpu

P = 2 ** 256 - 2 ** 32 - 977
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141


@pytest.fixture(scope='module')
def kats(golden):
    return golden('ecies_kats.json')


@pytest.fixture(scope='module')
def pairs(kats):
    """Every (key, point, shared x) of ecdh_kats, as bytes."""
    e = kats['ecdh_kats']
    out = []
    for p, row in zip(e['points'], e['shared_x']):
        pt = (bytes.fromhex(p['x']), bytes.fromhex(p['y']))
        out += [(bytes.fromhex(k), pt, bytes.fromhex(sx)) for k, sx in zip(e['keys'], row)]
    return out


def b32(v):
    return v.to_bytes(32, 'big')


def payload_for(shared_x, point, body, iv=b'\x24' * 16):
    """iv | curve | len X | X | len Y | Y | body | HMAC-SHA256(key_m, all before), key_m from shared_x."""
    x, y = point
    head = iv + struct.pack('!HH', 714, len(x)) + x + struct.pack('!H', len(y)) + y + body
    return head + hmac.new(hashlib.sha512(shared_x).digest()[32:], head, hashlib.sha256).digest()


def body_of(rng, n):
    return bytes(rng.getrandbits(8) for _ in range(n))


# ------------------------------------------------------------------ ECDH
def test_ecdh_kats_in_one_call(gpulib, pairs):
    got = ecies.ecdh([k for k, _, _ in pairs], [pt for _, pt, _ in pairs])
    assert got == [sx for _, _, sx in pairs]


@pytest.mark.parametrize('n', [1, 63, 64, 65])
def test_ecdh_call_sizes(gpulib, pairs, n):
    for start in (0, len(pairs) - n):
        sl = pairs[start:start + n]
        assert ecies.ecdh([k for k, _, _ in sl], [pt for _, pt, _ in sl]) == [sx for _, _, sx in sl]


def test_ecdh_is_strict(gpulib, pairs):
    k, (x, y), sx = pairs[30]
    yi = int.from_bytes(y, 'big')
    cases = [
        (k, (x, y), sx),
        (b32(0), (x, y), None),                  # key 0
        (b32(N), (x, y), None),                  # key = n
        (b32(N + 1), (x, y), None),
        (b32(2 ** 256 - 1), (x, y), None),
        (k, (b32(P), y), None),                  # coordinate = p
        (k, (x, b32(P + 1)), None),
        (k, (b32(2 ** 256 - 1), y), None),
        (k, (x, b32((yi + 1) % P)), None),       # off the curve
        (k, (b32(0), b32(0)), None),
        (k, (x, b32(P - yi)), sx),               # the opposite point: same x
        (k.lstrip(b'\x00')[1:], (x, y), 'short'),  # a shorter key is left-padded: another, valid scalar
    ]
    got = ecies.ecdh([c[0] for c in cases], [c[1] for c in cases])
    for c, g in zip(cases, got):
        if c[2] == 'short':
            assert g is not None and g != sx
        else:
            assert g == c[2]
    # the ok flags and zeroed outputs of the raw call
    n = len(cases)
    out, ok = ctypes.create_string_buffer(32 * n), ctypes.create_string_buffer(n)
    u8 = ctypes.POINTER(ctypes.c_uint8)
    priv = b''.join(c[0].rjust(32, b'\x00') for c in cases)
    pub = b''.join(c[1][0] + c[1][1] for c in cases)
    assert gpulib.bmpow_ecdh(n, priv, pub, ctypes.cast(out, u8), ctypes.cast(ok, u8)) == 0
    assert list(ok.raw) == [1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1]
    assert out.raw[32:64] == b'\x00' * 32


def test_ecdh_on_many_points(gpulib):
    """``var_table`` and the ladder on 256 points m G (m structured and random), 4 structured keys each,
    against the integer oracle (``oracle/ecdsa_oracle.py``): x(k m G), one fixed-base multiplication per
    pair; every eighth point also negated (the same x) and with y + 1 (off the curve: refused)."""
    from oracle import ecdsa_oracle as eo
    rng = random.Random(23)
    V = eo.scalar_set()
    ms = V[:7] + V[7::6][:121] + [rng.randrange(1, N) for _ in range(128)]
    assert len(ms) == 256 and {1, N - 1} <= set(ms)
    keys, points, want = [], [], []
    for j, m in enumerate(ms):
        x, y = eo.mult_g(m)
        ks = rng.sample(V, 4)
        shared = [b32(eo.mult_g(k * m % N)[0]) for k in ks]
        for pt, sx in (((x, y), shared), ((x, P - y), shared), ((x, (y + 1) % P), [None] * 4)):
            if pt[1] != y and j % 8:
                continue
            assert eo.on_curve(pt) == (sx[0] is not None)
            keys += [b32(k) for k in ks]
            points += [(b32(pt[0]), b32(pt[1]))] * 4
            want += sx
    assert len(want) == 4 * (256 + 32 + 32) and want.count(None) == 128
    got = ecies.ecdh(keys, points)
    assert got == want, [i for i, (g, w) in enumerate(zip(got, want)) if g != w][:10]


# ------------------------------------------------------------------ match
def test_match_msg_kats_against_the_three_keys(gpulib, kats):
    keys = [bytes.fromhex(k) for k in kats['recipient_keys']]
    blobs = [bytes.fromhex(m['blob']) for m in kats['msg_kats']]
    want = [m['recipient'] for m in kats['msg_kats']]
    assert any('coord_lens' in m for m in kats['msg_kats'])  # a short coordinate is among them
    assert ecies.match_keys(blobs, keys) == want
    # an unrelated key alone: nothing matches
    assert ecies.match_keys(blobs, [b32(0x1234567 * 2 ** 200 + 99)]) == [None] * len(blobs)
    # [k1, k0, k0]: the lowest index of k0 is 1, k1 is 0, k2 is absent
    got = ecies.match_keys(blobs, [keys[1], keys[0], keys[0]])
    assert got == [{0: 1, 1: 0, 2: None}[r] for r in want]
    # keys as pyelliptic holds them, leading zeros stripped
    assert ecies.match_keys(blobs, [k.lstrip(b'\x00') for k in keys]) == want


def test_match_verdict_kats(gpulib, kats):
    key = bytes.fromhex(kats['verdict_key'])
    verdicts = kats['verdict_kats']
    got = ecies.match_keys([bytes.fromhex(v['blob']) for v in verdicts], [b32(7), key])
    for v, g in zip(verdicts, got):
        assert g == (1 if v['match'] else None), v['name']
        if v['outcome'] == 'decrypted':
            assert v['match'], v['name']
    names = {v['name'] for v in verdicts if v['match']}
    assert {'curve_zero', 'x_33_leading_zero', 'y_34_leading_zeros', 'x_plus_p', 'neg_y'} <= names
    assert not {'off_curve', 'bad_mac', 'tail_0', 'tail_31', 'tail_32_bad_mac', 'short_19', 'empty'} & names


def test_match_argument_edges(gpulib, kats):
    blob = bytes.fromhex(kats['msg_kats'][0]['blob'])
    key = bytes.fromhex(kats['recipient_keys'][0])
    assert ecies.match_keys([], [key]) == []
    assert ecies.match_keys([blob, blob], []) == [None, None]
    for bad in (b32(0), b32(N), b32(2 ** 256 - 1)):
        with pytest.raises(_lib.BmpowError) as e:
            ecies.match_keys([blob], [key, bad])
        assert e.value.code == _lib.E_ARG
    assert ecies.match_keys([b'', blob, b'x' * 19], [b32(N - 1), key]) == [None, 1, None]


# ------------------------------------------------------------------ HMAC lengths
MAC_LENS = [L for L in range(86, 301) if L % 64 in (54, 55, 56, 57, 63, 0, 1)] + [20023]


def test_hmac_lengths_and_single_bit_flips(gpulib, pairs):
    """MACed lengths around the SHA-256 padding boundary (L + 9 crossing a multiple of 64), which the
    reference's own blobs (86 + 16 j) never reach, and one of ~20 KB; each payload matches, and stops
    matching after one flipped bit in the MAC, the IV or the last body byte."""
    rng = random.Random(5)
    k, pt, sx = pairs[25]
    assert len(pt[0]) == 32 and len(pt[1]) == 32
    assert {L % 64 for L in MAC_LENS} == {54, 55, 56, 57, 63, 0, 1} and len(MAC_LENS) == 22
    good, bad = [], []
    for L in MAC_LENS:
        p = payload_for(sx, pt, body_of(rng, L - 86))
        assert len(p) == L + 32
        good.append(p)
        for at in (len(p) - 1, 0, L - 1):  # last MAC byte, first IV byte, last MACed byte
            bad.append(p[:at] + bytes([p[at] ^ 0x10]) + p[at + 1:])
    got = ecies.match_keys(good + bad, [b32(3), k])
    assert got[:len(good)] == [1] * len(good)
    assert got[len(good):] == [None] * len(bad)


def test_mixed_wave(gpulib, pairs):
    """64 payloads of 118 bytes to a few KB in shuffled order against 2 keys: half for key 1, a quarter
    for key 0, a quarter for nobody; over all three fixture points."""
    rng = random.Random(11)
    per_key = len(pairs) // 3
    ia, ib = 40, 41  # two of the fixture's random keys
    keys = [pairs[ia][0], pairs[ib][0]]
    payloads, want = [], []
    for j in range(64):
        pi = j % 3
        body = body_of(rng, rng.choice([0, 1, 16, 23, 100, 1000, 2500, 4000]) if j else 0)
        who = [1, 0, 1, None][j % 4]
        sx = pairs[pi * per_key + (ib if who == 1 else ia)][2] if who is not None else b32(j + 1)
        pt = pairs[pi * per_key][1]
        payloads.append(payload_for(sx, pt, body))
        want.append(who)
    assert len(payloads[0]) == 118
    order = list(range(64))
    rng.shuffle(order)
    got = ecies.match_keys([payloads[i] for i in order], keys)
    assert got == [want[i] for i in order]


def test_key_groups_and_object_sets(gpulib, kats, pairs):
    """More pairs than one launch takes (2,048 objects x 1,100 keys: the keys go in groups of 1,024, and
    the matching keys lie in the second group, so key_e is gathered from there), and more objects than
    one set of 2^18 (300,000 x 1 key)."""
    rng = random.Random(17)
    k, pt, sx = pairs[33]
    mine = payload_for(sx, pt, body_of(rng, 48))
    other = payload_for(b32(5), pt, body_of(rng, 48))
    longer = payload_for(sx, pt, body_of(rng, 700))
    real = next(m for m in kats['msg_kats'] if m['recipient'] == 0 and len(m['plaintext']) == 200)
    objs = [mine if i % 5 == 0 else longer if i % 7 == 0 else other for i in range(2048)]
    objs[3] = objs[2047] = bytes.fromhex(real['blob'])
    keys = [b32(rng.randrange(1, N)) for _ in range(1100)]
    keys[1055] = bytes.fromhex(kats['recipient_keys'][0])
    keys[1056] = keys[1099] = k
    want = [1055 if i in (3, 2047) else None if o is other else 1056 for i, o in enumerate(objs)]
    gpulib.bmpow_ecies_reset_stats()
    assert ecies.match_keys(objs, keys) == want
    st = _lib.BmpowEciesStats()
    assert gpulib.bmpow_ecies_get_stats(ctypes.byref(st)) == 0
    assert (st.calls, st.objects, st.pairs) == (1, 2048, 2048 * 1100) and st.launches == 2
    assert st.ecdh_ms > 0 and st.mac_ms > 0 and st.prep_ms > 0
    res = ecies.decrypt_batch(objs, keys)
    assert res[3] == res[2047] == (1055, bytes.fromhex(real['plaintext']))
    assert all(r is None for i, r in enumerate(res) if objs[i] is other)
    many = [mine, other, longer, other, b'junk'] * 60000
    assert ecies.match_keys(many, [k]) == [0, None, 0, None, None] * 60000


# ------------------------------------------------------------------ the Python module
def test_decrypt_batch_and_process_msgs(gpulib, kats):
    keys = [bytes.fromhex(k) for k in kats['recipient_keys']]
    msgs = kats['msg_kats']
    blobs = [bytes.fromhex(m['blob']) for m in msgs]
    res = ecies.decrypt_batch(blobs, keys)
    assert res == [(m['recipient'], bytes.fromhex(m['plaintext'])) for m in msgs]
    # valid MAC, but the reference raised in the cipher: no plaintext, while the key still matches
    vkey = bytes.fromhex(kats['verdict_key'])
    bad = [v for v in kats['verdict_kats'] if v['match'] and v['outcome'] != 'decrypted']
    assert {'bad_padding_valid_mac', 'ct_17_valid_mac', 'tail_32_valid_mac'} <= {v['name'] for v in bad}
    bblobs = [bytes.fromhex(v['blob']) for v in bad]
    assert ecies.decrypt_batch(bblobs, [vkey]) == [None] * len(bad)
    assert ecies.match_keys(bblobs, [vkey]) == [0] * len(bad)
    good = [v for v in kats['verdict_kats'] if v['outcome'] == 'decrypted']
    assert ecies.decrypt_batch([bytes.fromhex(v['blob']) for v in good], [vkey]) == \
        [(0, bytes.fromhex(v['plaintext'])) for v in good]
    # process_msgs: the header walk, then the same
    ripes = [b'ripe-of-address-%d....' % i for i in range(3)]
    by_ripe = dict(zip(ripes, keys))
    head = b'\x00' * 8 + b'\x22' * 8 + b'\x00\x00\x00\x02'
    objects = [head + b'\x01\x01' + b for b in blobs]
    objects.append(head + b'\x02\x01' + blobs[0])             # version 2
    objects.append(head + b'\x01\xfd\x01\x00' + blobs[1])     # 3-byte stream number
    objects.append(head + b'\x01\x01' + bblobs[0])            # matches nobody here
    want = [(ripes[m['recipient']], bytes.fromhex(m['plaintext'])) for m in msgs]
    want += [None, want[1], None]
    assert ecies.process_msgs(objects, by_ripe) == want


def test_abort_is_honoured(gpulib, kats):
    blob = bytes.fromhex(kats['msg_kats'][0]['blob'])
    key = bytes.fromhex(kats['recipient_keys'][0])
    gpulib.bmpow_abort()
    try:
        with pytest.raises(_lib.BmpowError) as e:
            ecies.match_keys([blob], [key])
        assert e.value.code == _lib.E_ABORTED
    finally:
        gpulib.bmpow_clear_abort()
    assert ecies.match_keys([blob], [key]) == [0]
