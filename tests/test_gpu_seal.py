"""The device seal on the GPU (``sl_seal_kernel``, ``sl_cbc_kernel``; ``bmpow_ecies_seal_batch``,
``bmpow_aes256_cbc``, ``bmpow_ecies_encrypt`` in device mode, ``ecies.decrypt_batch``) against libcrypto
through the library's host calls (``sender.seal``, ``ecies.decrypt``), the reference-made fixtures
``send_kats.json`` / ``ecies_kats.json`` and the published AES-256 vectors (tests/test_seal.py pins those
against libcrypto without a GPU).  Host mode and device mode must give the same bytes under the same
ephemeral keys and IVs; ``seal_stats()['rows_device']`` says that the kernel ran."""
import hashlib
import random

import pytest

from oracle import ecdsa_oracle as eo
from pybitmessage_amd import _lib, ecies, intake, sender, signatures, worker
from tests.test_seal import (C3_CIPHER, C3_KEY, C3_PLAIN, F25_CIPHER, F25_IV, F25_KEY, F25_PLAIN, host_cbc_decrypt,
                             host_cbc_encrypt)

pytestmark = pytest.mark.gpu

P, N = eo.P, eo.N
DEVICE_PLAIN = 256 << 10  # longer rows are sealed by the host's code in either mode


def b32(v):
    return v.to_bytes(32, 'big')


@pytest.fixture(scope='module')
def kats(golden):
    return golden('send_kats.json')


@pytest.fixture(scope='module')
def recipients(kats):
    privs = [bytes.fromhex(k) for k in kats['recipient_keys']]
    return privs, [bytes.fromhex(k) for k in kats['recipient_pubs']]


@pytest.fixture
def device_seal(gpulib):
    prev = sender.set_seal(1)
    sender.reset_seal_stats()
    yield
    sender.set_seal(prev)


def in_host_mode(call):
    prev = sender.set_seal(0)
    try:
        return call()
    finally:
        sender.set_seal(prev)


# ------------------------------------------------------------------ 1. the raw calls on the published vectors
def test_published_vectors_both_ways(gpulib):
    enc = ecies.aes_cbc_batch([C3_KEY, F25_KEY], [bytes(16), F25_IV], [C3_PLAIN, F25_PLAIN])
    assert enc[0][:16] == C3_CIPHER and len(enc[0]) == 32
    assert enc[1] == F25_CIPHER
    dec = ecies.aes_cbc_batch([C3_KEY, F25_KEY], [bytes(16), F25_IV], enc, decrypt=True)
    assert dec == [C3_PLAIN, F25_PLAIN]
    assert ecies.aes_cbc_batch([F25_KEY], [F25_IV], [F25_CIPHER], decrypt=True) == [F25_PLAIN]


# ------------------------------------------------------------------ 2. raw AES against libcrypto
RAW_LENS = list(range(81)) + [255, 256, 257, 4095, 4096, 65537]


@pytest.fixture(scope='module')
def raw_cases():
    """(key, iv, plaintext, libcrypto's ciphertext) per length, shuffled: shared, never changed."""
    rng = random.Random(91)
    cases = []
    for ln in RAW_LENS:
        key, iv, plain = rng.randbytes(32), rng.randbytes(16), rng.randbytes(ln)
        cases.append((key, iv, plain, host_cbc_encrypt(key, iv, plain)))
    rng.shuffle(cases)
    return cases


@pytest.mark.parametrize('n', [1, 63, 64, 65, 130])
def test_raw_cbc_call_sizes_of_mixed_lengths(gpulib, raw_cases, n):
    rows = [raw_cases[(i + 5 * n) % len(raw_cases)] for i in range(n)]
    if n == 130:
        assert {len(r[2]) for r in rows} == set(RAW_LENS)  # every length, in one call
    keys, ivs = [r[0] for r in rows], [r[1] for r in rows]
    enc = ecies.aes_cbc_batch(keys, ivs, [r[2] for r in rows])
    assert enc == [r[3] for r in rows]
    assert ecies.aes_cbc_batch(keys, ivs, enc, decrypt=True) == [r[2] for r in rows]
    for r in rows[:8]:
        assert host_cbc_decrypt(r[0], r[1], r[3]) == r[2]


def test_raw_cbc_bad_inputs_beside_good_rows(gpulib, raw_cases):
    rng = random.Random(92)
    key, iv = rng.randbytes(32), rng.randbytes(16)

    def ending(tail):  # a ciphertext whose plaintext is 32 bytes ending in `tail`, with no padding block behind
        plain = rng.randbytes(32 - len(tail)) + tail
        return host_cbc_encrypt(key, iv, plain)[:32]

    bad = {5: b'', 17: rng.randbytes(17), 29: ending(b'\x00'), 40: ending(b'\x11'), 41: ending(b'\x03\x02\x03'),
           63: ending(b'\x05' * 4), 64: ending(bytes([16] * 15))}
    good_tail = {70: ending(b'\x01'), 71: ending(b'\x04' * 4)}
    rows = []
    for i in range(80):
        if i in bad:
            rows.append((key, iv, bad[i]))
        elif i in good_tail:
            rows.append((key, iv, good_tail[i]))
        else:
            c = raw_cases[i % len(raw_cases)]
            rows.append((c[0], c[1], c[3]))
    got = ecies.aes_cbc_batch([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], decrypt=True)
    want = [host_cbc_decrypt(*r) for r in rows]
    assert got == want
    assert [i for i, g in enumerate(got) if g is None] == sorted(bad)
    assert len(got[70]) == 31 and len(got[71]) == 28


# ------------------------------------------------------------------ 3. every head length and SHA-256 boundary
def test_seal_batch_every_head_and_boundary(gpulib):
    rng = random.Random(93)
    rows, residues, heads = [], set(), set()
    for head in range(22, 87):
        strip = 86 - head
        xs = min(32, strip)  # strip == 32 and above: an all-zero X
        ys = strip - xs
        for ln in range(65):
            body = bytes(rng.randrange(1, 256) for _ in range(64))
            R = bytes(xs) + body[xs:32] + bytes(ys) + body[32 + ys:]
            rows.append((rng.randbytes(ln), rng.randbytes(16), R, rng.randbytes(64)))
            residues.add((head + 16 * (ln // 16 + 1)) % 64)
            heads.add(head % 4)
    assert len(rows) == 4225 and {55, 56, 63, 0} <= residues and heads == {0, 1, 2, 3}
    sender.reset_seal_stats()
    got = sender.seal_batch(*zip(*rows))
    st = sender.seal_stats()
    assert st['rows_device'] == 4225 and st['rows_host'] == 0 and st['sets'] == 1 and st['launches'] == 1
    for i, r in enumerate(rows):
        assert got[i] == sender.seal(*r), (i, len(r[0]))
    assert {len(g) - 32 - 16 * (len(r[0]) // 16 + 1) for g, r in zip(got, rows)} == set(range(22, 87))


# ------------------------------------------------------------------ 4. encrypt_batch in device mode
def test_encrypt_kats_bit_for_bit(device_seal, kats, recipients):
    rows = kats['encrypt_kats']
    assert len(rows) == 23
    got = sender.encrypt_batch([bytes.fromhex(k['plaintext']) for k in rows], [recipients[1][k['recipient']] for k in rows],
                               ephemeral=[bytes.fromhex(k['ephemeral']) for k in rows],
                               ivs=[bytes.fromhex(k['iv']) for k in rows])
    assert got == [bytes.fromhex(k['blob']) for k in rows]
    assert sum(k['coord_lens'] != [32, 32] for k in rows) >= 2
    assert sender.seal_stats()['rows_device'] == 23


@pytest.mark.parametrize('n', [1, 63, 64, 65])
def test_device_mode_equals_host_mode(device_seal, recipients, n):
    privs, pubs = recipients
    rng = random.Random(94 + n)
    plains = [rng.randbytes(rng.choice((0, 1, 15, 16, 17, 100, 333, 2000))) for _ in range(n)]
    to = [pubs[rng.randrange(3)] for _ in range(n)]
    eph = [b32(rng.randrange(1, N)) for _ in range(n)]
    ivs = [rng.randbytes(16) for _ in range(n)]
    dev = sender.encrypt_batch(plains, to, ephemeral=eph, ivs=ivs)
    st = sender.seal_stats()
    assert st['rows_device'] == n and st['rows_host'] == 0 and st['calls'] == 1
    host = in_host_mode(lambda: sender.encrypt_batch(plains, to, ephemeral=eph, ivs=ivs))
    assert sender.seal_stats()['rows_device'] == n  # host mode launched no seal
    assert dev == host and all(b is not None for b in dev)


def test_refused_recipient_keys_in_one_wave_device_mode(device_seal, recipients):
    privs, pubs = recipients
    x, y = eo.key_xy(pubs[0])
    keys = [pubs[i % 3] for i in range(64)]
    keys[5] = b32(x) + b32((y + 1) % P)  # off the curve
    keys[20] = b32(P) + b32(y)           # a coordinate that is not below p
    keys[41] = b32(x) + b32(P - y)       # the negated key
    keys[50] = b'\x00' * 63              # no key at all
    plains = [b'plain %d' % i for i in range(64)]
    blobs = sender.encrypt_batch(plains, keys)
    assert [i for i, b in enumerate(blobs) if b is None] == [5, 20, 50]
    assert sender.seal_stats()['rows_device'] == 62  # the off-curve row reaches the kernel, which writes no blob
    opened = ecies.decrypt_batch([b for b in blobs if b is not None], privs)
    assert opened == [(0 if i == 41 else i % 3, plains[i]) for i in range(64) if i not in (5, 20, 50)]


# ------------------------------------------------------------------ 5. the host's sealer inside a device call
def test_a_row_above_the_object_limit_is_sealed_by_the_host(device_seal, recipients):
    privs, pubs = recipients
    rng = random.Random(95)
    plains = [rng.randbytes(rng.randrange(0, 300)) for _ in range(65)]
    plains[33] = rng.randbytes(DEVICE_PLAIN + 1)
    to = [pubs[i % 3] for i in range(65)]
    eph = [b32(rng.randrange(1, N)) for _ in range(65)]
    ivs = [rng.randbytes(16) for _ in range(65)]
    dev = sender.encrypt_batch(plains, to, ephemeral=eph, ivs=ivs)
    st = sender.seal_stats()
    assert st['rows_host'] == 1 and st['rows_device'] == 64
    assert dev == in_host_mode(lambda: sender.encrypt_batch(plains, to, ephemeral=eph, ivs=ivs))
    # at the limit itself the row stays on the device
    sender.reset_seal_stats()
    edge = sender.encrypt_batch([plains[33][:DEVICE_PLAIN]], [to[33]], ephemeral=[eph[33]], ivs=[ivs[33]])
    assert sender.seal_stats()['rows_device'] == 1 and sender.seal_stats()['rows_host'] == 0
    assert edge == in_host_mode(lambda: sender.encrypt_batch([plains[33][:DEVICE_PLAIN]], [to[33]], ephemeral=[eph[33]],
                                                             ivs=[ivs[33]]))


# ------------------------------------------------------------------ 6. two sets
def test_two_sets_in_one_device_call(device_seal, recipients):
    """2^18 + 65 rows of 16-byte plaintexts cycling over 128 seeded (plaintext, ephemeral key, IV, recipient)
    rows: host mode seals the 128, and every one of the device call's blobs equals its row's."""
    privs, pubs = recipients
    rng = random.Random(96)
    base = [(rng.randbytes(16), pubs[i % 3], b32(rng.randrange(1, N)), rng.randbytes(16)) for i in range(128)]
    host = in_host_mode(lambda: sender.encrypt_batch(*zip(*base)))
    n = (1 << 18) + 65
    cols = [[b[c] for b in base] * (n // 128 + 1) for c in range(4)]
    got = sender.encrypt_batch(cols[0][:n], cols[1][:n], ephemeral=cols[2][:n], ivs=cols[3][:n])
    st = sender.seal_stats()
    assert st['sets'] == 2 and st['rows_device'] == n and st['calls'] == 1 and st['launches'] == 2
    assert len(got) == n
    for j in range(128):
        assert host[j] is not None and all(g == host[j] for g in got[j::128]), j


# ------------------------------------------------------------------ 7. the receive side
def test_verdict_kats_repeated_in_one_decrypt_batch(gpulib, golden):
    ek = golden('ecies_kats.json')
    verdicts = ek['verdict_kats']
    assert len(verdicts) == 29
    key = bytes.fromhex(ek['verdict_key'])
    rows = [verdicts[i % 29] for i in range(130)]
    sender.reset_seal_stats()
    got = ecies.decrypt_batch([bytes.fromhex(v['blob']) for v in rows], [b32(7), key])
    for v, g in zip(rows, got):
        assert g == ((1, bytes.fromhex(v['plaintext'])) if v['outcome'] == 'decrypted' else None), v['name']
    by_name = {v['name']: v for v in verdicts}
    assert by_name['bad_padding_valid_mac']['match'] and by_name['bad_padding_valid_mac']['outcome'] != 'decrypted'
    assert sender.seal_stats()['launches'] == 1  # one CBC call for all the matches


def test_round_trips_of_mixed_lengths(device_seal, recipients):
    privs, pubs = recipients
    rng = random.Random(97)
    plains = [rng.randbytes(rng.choice((0, 1, 15, 16, 17, 31, 32, 100, 333, 1000, 5000))) for _ in range(130)]
    to = [rng.randrange(3) for _ in range(130)]
    blobs = sender.encrypt_batch(plains, [pubs[t] for t in to])
    assert ecies.decrypt_batch(blobs, privs) == list(zip(to, plains))


# ------------------------------------------------------------------ 8. abort
def test_abort_is_honoured(device_seal, recipients):
    privs, pubs = recipients
    calls = (lambda: sender.encrypt_batch([b'm'], [pubs[0]]),
             lambda: sender.seal_batch([b'm'], [bytes(16)], [bytes([1]) * 64], [bytes(64)]),
             lambda: ecies.aes_cbc_batch([bytes(32)], [bytes(16)], [b'm']))
    gpulib = _lib.get()
    gpulib.bmpow_abort()
    try:
        for call in calls:
            with pytest.raises(_lib.BmpowError) as e:
                call()
            assert e.value.code == _lib.E_ABORTED
    finally:
        gpulib.bmpow_clear_abort()
    blob = calls[0]()[0]
    assert ecies.decrypt_batch([blob], privs) == [(0, b'm')]
    assert calls[1]() == [sender.seal(b'm', bytes(16), bytes([1]) * 64, bytes(64))]
    assert calls[2]() == [host_cbc_encrypt(bytes(32), bytes(16), b'm')]


# ------------------------------------------------------------------ 9. the whole send path
def test_send_msgs_signed_through_the_receive_path_device_mode(device_seal, recipients):
    """tests/test_gpu_send.py's test of the same name, with the blobs sealed on the device."""
    rng0 = random.Random(77)
    ks = [rng0.randrange(1, N) for _ in range(2)]
    pubs = [b'\x04' + eo.xy_key(eo.mult_g(k)) for k in ks]
    privs, rpubs = recipients
    now = 1760000000
    sign_priv, sign_pub, enc_pub = b32(ks[0]), pubs[0], pubs[1]
    ripes = [hashlib.sha1(p).digest() for p in rpubs[:2]]
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
    out = worker.send_msgs_signed(jobs, build_plain, rng=random.Random(84), now=now)
    assert sender.seal_stats()['rows_device'] >= 2 and sender.seal_stats()['rows_host'] == 0
    assert out[2] is None and out[0] is not None and out[1] is not None
    objs = out[:2]
    res = intake.check_objects(objs, streams=(1,), nonceTrialsPerByte=10, payloadLengthExtraBytes=10, now=now)
    assert list(res.status) == [intake.OK, intake.OK]
    opened = ecies.process_msgs(objs, {ripes[0]: privs[0], ripes[1]: privs[1]})
    assert [o[0] for o in opened] == ripes
    parts = [signatures.msg_signed_parts(o, p[1]) for o, p in zip(objs, opened)]
    assert all(p is not None and p[2] == sign_pub[1:] for p in parts)
    assert signatures.verify_batch_digest([p[0] for p in parts], [p[1] for p in parts], [p[2] for p in parts]) \
        == [signatures.SHA256] * 2
    for p, name in zip(opened, ('to_a', 'to_b_no_ack')):
        unsigned = worker.msg_plaintext(4, 1, worker.get_bitfield(), sign_pub, enc_pub, ripes[0 if name == 'to_a' else 1], 2,
                                        b'Subject:hello\nBody:' + name.encode() * 20, seen[name], 10, 10)
        assert p[1].startswith(unsigned)
