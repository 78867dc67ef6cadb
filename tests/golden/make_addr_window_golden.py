#!/usr/bin/env python3
"""Generate tests/golden/addr_window_kats.json -- EVERY try with a one-zero-byte ripe in whole
windows of the address search, from the REFERENCE's own primitives (build container only; needs
/root/reference, read-only):

    BITMESSAGE_HOME=$(mktemp -d) PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_addr_window_golden.py

Same means as make_addr_golden.py: ``highlevelcrypto.pointMult`` (OpenSSL EC_POINT_mul),
``fallback.RIPEMD160Hash``, ``addresses.encodeVarint`` and the re-run under an ``OPENSSL_CONF``
that activates OpenSSL 3's legacy provider (RIPEMD-160).

The search kernel's own ripes are otherwise observed only at a handful of first hits; a window
lists every k in ``[start, start + count)`` whose ripe starts with a zero byte, so a test that
enumerates the window through the public calls sees every false negative and false positive of
every lane slot (tests/test_gpu_addr_windows.py).

* mode 0 (deterministic, ``class_addressGenerator.py:238-271``): try k has
  ``SHA512(pp || varint(2k))[:32]`` and ``SHA512(pp || varint(2k + 1))[:32]``;
* mode 1 (random, as ``bmpow_address_search_random`` defines it): fixed signing key, encryption key
  ``SHA512(seed || varint(k))[:32]``.

The windows sit on the varint boundaries of the nonce, on the one-block / two-block switch of the
SHA-512 tail, and at the top of the deterministic range (2k + 1 = 2^64 - 1, the last nonce
``encodeVarint`` takes).  The conditions the tests rely on are asserted here before the file is
written.
"""
import hashlib
import json
import multiprocessing
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REF_SRC = '/root/reference/src'
CNF = '''openssl_conf = openssl_init
[openssl_init]
providers = provider_sect
[provider_sect]
default = default_sect
legacy = legacy_sect
[default_sect]
activate = 1
[legacy_sect]
activate = 1
'''

SAMPLE_SEED = b'TIGER, tiger, burning bright. In the forests of the night'  # src/tests/samples.py:32
RANDOM_SEED = hashlib.sha512(b'bmpow random-mode test').digest()
RANDOM_PRIV_SIGNING = hashlib.sha256(b'bmpow random-mode signing key').digest()

# (seed, start, count, first k on the far side of the varint boundary inside the window or None)
DET_WINDOWS = [
    (SAMPLE_SEED, 0, 2048, 127),                  # 2k crosses 253 at k = 126/127
    (b'x' * 118, 32768 - 1024, 2048, 32768),      # two tail blocks; 2k crosses 2^16
    (b'q' * 200, 2 ** 31 - 1024, 2048, 2 ** 31),  # midstate + tail 72 (byte-aligned); 2k crosses 2^32
    (b'', 2 ** 40 + 3, 2048, None),               # odd start, 9-byte varints, tail 0
    (b'y' * 127, 2 ** 63 - 2048, 2048, None),     # ends on the last try that exists
    (b'p' * 111, 12345, 2048, None),              # one-block / two-block switch, odd start
    (b'z' * 300, 65536 - 1000, 2048, None),       # two midstate blocks, 5-byte varints
    (b'w' * 103, 2 ** 32 - 1, 2048, None),        # tail + varint = 112 exactly, at 9 bytes
]
RANDOM_WINDOWS = [
    (RANDOM_SEED, 0, 4096, None),
    (RANDOM_SEED[:55], 65536 - 2048, 4096, 65536),
    (b'r' * 119, 2 ** 32 - 2048, 4096, 2 ** 32),
    (b'', 2 ** 40 + 1, 4096, None),
    (hashlib.sha512(b'bmpow random-mode test 3').digest(), 0, 512, 253),
]

_prims = {}


def _setup():
    if not _prims:
        sys.path.insert(0, REF_SRC)
        import highlevelcrypto
        from addresses import encodeVarint
        from fallback import RIPEMD160Hash
        _prims.update(pm=highlevelcrypto.pointMult, varint=encodeVarint, ripemd=RIPEMD160Hash)
        _prims['pub_s'] = highlevelcrypto.pointMult(RANDOM_PRIV_SIGNING)
    return _prims


def scan(job):
    """Every hit of tries [lo, hi) of one window: (k, ripe, priv_signing, priv_encryption)."""
    mode, _, seed, lo, hi = job
    p = _setup()
    pm, varint, ripemd = p['pm'], p['varint'], p['ripemd']
    hits = []
    for k in range(lo, hi):
        if mode == 0:
            ps = hashlib.sha512(seed + varint(2 * k)).digest()[:32]
            pe = hashlib.sha512(seed + varint(2 * k + 1)).digest()[:32]
            pub_s = pm(ps)
        else:
            ps = RANDOM_PRIV_SIGNING
            pe = hashlib.sha512(seed + varint(k)).digest()[:32]
            pub_s = p['pub_s']
        ripe = ripemd(hashlib.sha512(pub_s + pm(pe)).digest()).digest()
        if ripe[:1] == b'\x00':
            hits.append({'k': k, 'ripe': ripe.hex(), 'priv_signing': ps.hex(), 'priv_encryption': pe.hex()})
    return hits


def main():
    try:
        hashlib.new('ripemd160')
    except ValueError:
        with tempfile.NamedTemporaryFile('w', suffix='.cnf', delete=False) as f:
            f.write(CNF)
        env = dict(os.environ, OPENSSL_CONF=f.name)
        sys.exit(subprocess.call([sys.executable] + sys.argv, env=env))
    _setup()
    specs = [(0, i) + w for i, w in enumerate(DET_WINDOWS)] + [(1, i) + w for i, w in enumerate(RANDOM_WINDOWS)]
    chunk = 256
    jobs = [(mode, index, seed, lo, min(lo + chunk, start + count))
            for mode, index, seed, start, count, _ in specs for lo in range(start, start + count, chunk)]
    with multiprocessing.Pool(min(12, os.cpu_count() or 1)) as pool:
        parts = pool.map(scan, jobs)
    windows = []
    for mode, index, seed, start, count, boundary in specs:
        hits = [h for job, part in zip(jobs, parts) if job[:2] == (mode, index) for h in part]
        offs = [h['k'] - start for h in hits]
        print('mode %d window %d: %2d hits at offsets %s' % (mode, index, len(hits), offs))
        assert offs == sorted(set(offs)) and all(0 <= o < count for o in offs)
        assert len(hits) >= 3, 'a window needs at least 3 hits'
        if boundary is not None:
            assert any(h['k'] < boundary for h in hits) and any(h['k'] >= boundary for h in hits), \
                'no hit on one side of the varint boundary k = %d' % boundary
        w = {'mode': mode, 'index': index, 'seed': seed.hex(), 'start': start, 'count': count, 'hits': hits}
        if mode == 1:
            w['priv_signing'] = RANDOM_PRIV_SIGNING.hex()
        windows.append(w)
    for mode, mod in ((0, 2), (1, 4)):
        counts = [sum((h['k'] - w['start']) % mod == r for w in windows if w['mode'] == mode for h in w['hits'])
                  for r in range(mod)]
        print('mode %d: %d hits, offsets mod %d: %s' % (mode, sum(counts), mod, counts))
        assert all(counts), 'a lane slot of mode %d has no hit' % mode
    with open(os.path.join(HERE, 'addr_window_kats.json'), 'w') as f:
        json.dump({'source': 'reference highlevelcrypto.pointMult (OpenSSL), fallback.RIPEMD160Hash, '
                             'addresses.encodeVarint: every k of each window whose ripe starts with 00',
                   'windows': windows}, f, indent=1)
    print('wrote addr_window_kats.json')


if __name__ == '__main__':
    main()
