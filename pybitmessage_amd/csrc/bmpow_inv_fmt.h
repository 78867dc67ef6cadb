// bmpow_inv_fmt.h -- the byte- and word-level half of the device-resident inventory sets (include/bmpow_inv.h):
// the slot state word, the seeded mix that picks a key's start slot and its tag, the load of a 32-byte key from
// any byte offset of an uploaded buffer, the steps of claim / finalize / lookup / remove / rebuild on one slot,
// and the walk of an `inv` / `dinv` / `getdata` payload -- written once for the device (bmpow_inv.hip), for the
// host unit (bmpow_host_inv.hip) and for the stand-alone test program (tests/native/inv_sim.cpp builds this
// header with g++ and drives the same slot functions from one thread).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define IV_HD __host__ __device__ __forceinline__
#else
#define IV_HD inline
#endif

// What a slot holds beside its state word and its 32-byte key.
struct iv_val {
  uint64_t expires;
  uint32_t stream;
  uint32_t aux;
};

#define IV_NONE 0xffffffffu     // no slot / no row
#define IV_PRESENT 0xfffffffeu  // claim[]: the key was resident before the call

namespace ivf {

// ---- the state word ----
//   0                    empty
//   1                    tombstone (a removed entry; probes pass over it, inserts never reuse it)
//   01 .. | row          pending: claimed in this launch by input row `row`, key and value not yet written
//   1  .. | tag          full: key and value were written by an earlier launch; tag = 63 bits of the key's mix
constexpr uint64_t kEmpty = 0, kTomb = 1;
constexpr uint64_t kPendingBit = 1ull << 62, kFullBit = 1ull << 63;
IV_HD bool is_full(uint64_t w) { return (w & kFullBit) != 0; }
IV_HD bool is_pending(uint64_t w) { return (w >> 62) == 1; }
IV_HD uint64_t pending_word(uint32_t row) { return kPendingBit | row; }
IV_HD uint32_t pending_row(uint64_t w) { return (uint32_t)w; }
IV_HD uint64_t full_word(uint64_t tag) { return kFullBit | tag; }

// ---- the mix ----
IV_HD uint64_t fmix(uint64_t x) {  // the 64-bit finaliser of MurmurHash3 (public domain)
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdULL;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ULL;
  x ^= x >> 33;
  return x;
}

// The start slot of key k (four little-endian words) in a table of 2^log2 slots: every word of the key and the
// set's seed go through the finaliser in a chain, and the top bits of the end pick the slot.  A peer chooses
// the 32 bytes of an `inv` item freely; without the seed it cannot aim them at one slot.  1 <= log2 <= 31.
IV_HD uint32_t start_slot(uint64_t seed, uint32_t log2, const uint64_t (&k)[4]) {
  uint64_t h = fmix(seed ^ 0x9e3779b97f4a7c15ULL);
  for (int i = 0; i < 4; ++i) h = fmix(h ^ k[i]);
  return (uint32_t)(h >> (64 - log2));
}

// The tag a full slot carries: 63 bits mixed from the seed and the key's first two words only, so that two keys
// that differ in their last 16 bytes alone have equal tags (the tests build such pairs) -- an equal tag is a
// hint; the resident key decides.
IV_HD uint64_t tag_of(uint64_t seed, const uint64_t (&k)[4]) {
  return fmix(fmix(k[0] ^ seed) + k[1]) & ~kFullBit;
}

IV_HD bool key_eq(const uint64_t (&a)[4], const uint64_t (&b)[4]) {
  return ((a[0] ^ b[0]) | (a[1] ^ b[1]) | (a[2] ^ b[2]) | (a[3] ^ b[3])) == 0;
}

// ---- the key load ----
// Word q of a buffer of nbytes bytes whose base is 8-byte aligned, as a little-endian number: one aligned
// 8-byte load where the whole word lies inside the buffer, else the bytes that do, one by one (the buffer's last
// word only).  Never touches a byte at or past nbytes.
IV_HD uint64_t load_word(const uint64_t* buf, uint64_t nbytes, uint64_t q) {
  if (8 * q + 8 <= nbytes) return buf[q];
  uint64_t w = 0;
  const uint8_t* b = reinterpret_cast<const uint8_t*>(buf);
  for (uint64_t i = 8 * q, j = 0; i < nbytes && j < 8; ++i, ++j) w |= (uint64_t)b[i] << (8 * j);
  return w;
}

// The 32 bytes at byte offset off (off + 32 <= nbytes) as four little-endian words.  An item of an `inv` payload
// sits behind a 1-, 3-, 5- or 9-byte varint and is never 8-byte aligned: the words come from the aligned-down
// address, five of them funnelled by off mod 8 (four where off is aligned).
IV_HD void load_key(const uint64_t* buf, uint64_t nbytes, uint64_t off, uint64_t (&k)[4]) {
  const uint64_t q = off >> 3;
  const uint32_t sh = 8 * (uint32_t)(off & 7);
  uint64_t w[5];
  for (int i = 0; i < 4; ++i) w[i] = load_word(buf, nbytes, q + (uint64_t)i);
  w[4] = sh ? load_word(buf, nbytes, q + 4) : 0;
  for (int i = 0; i < 4; ++i) k[i] = sh ? (w[i] >> sh) | (w[i + 1] << (64 - sh)) : w[i];
}

// ---- the table and the input rows ----
struct Table {
  uint64_t* state;  // [slots]
  uint64_t* keys;   // [4 slots]
  iv_val* vals;     // [slots]
  uint64_t seed;
  uint32_t log2;
};
IV_HD uint32_t slots_of(const Table& t) { return 1u << t.log2; }

// n rows: row i's key is the 32 bytes at offs[i] of buf (offs null: at 32 i); every row lies inside nbytes.
struct Rows {
  const uint64_t* buf;
  uint64_t nbytes;
  const uint32_t* offs;
  uint32_t n;
};
IV_HD bool row_key(const Rows& r, uint32_t i, uint64_t (&k)[4]) {
  const uint64_t off = r.offs ? r.offs[i] : 32ull * i;
  if (off + 32 > r.nbytes) return false;  // never: the host planned every row inside the upload
  load_key(r.buf, r.nbytes, off, k);
  return true;
}

// The state word's accesses, one definition per side: on the device relaxed agent-scope atomics (plain HIP
// atomics: vector instructions), on the host (one thread: the model of the native test) plain accesses.
#if defined(__HIP_DEVICE_COMPILE__)
IV_HD uint64_t st_load(uint64_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
IV_HD void st_store(uint64_t* p, uint64_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
IV_HD uint64_t st_swap(uint64_t* p, uint64_t v) {
  return __hip_atomic_exchange(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// true: *p was expect and is now v; else expect = what *p holds
IV_HD bool st_cas(uint64_t* p, uint64_t& expect, uint64_t v) {
  return __hip_atomic_compare_exchange_strong(p, &expect, v, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
IV_HD void min_u32(uint32_t* p, uint32_t v) { __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
#else
IV_HD uint64_t st_load(uint64_t* p) { return *p; }
IV_HD void st_store(uint64_t* p, uint64_t v) { *p = v; }
IV_HD uint64_t st_swap(uint64_t* p, uint64_t v) {
  const uint64_t old = *p;
  *p = v;
  return old;
}
IV_HD bool st_cas(uint64_t* p, uint64_t& expect, uint64_t v) {
  if (*p == expect) {
    *p = v;
    return true;
  }
  expect = *p;
  return false;
}
IV_HD void min_u32(uint32_t* p, uint32_t v) {
  if (v < *p) *p = v;
}
#endif

IV_HD bool resident_eq(const Table& t, uint32_t s, const uint64_t (&k)[4]) {
  const uint64_t* r = t.keys + 4ull * s;
  const uint64_t rk[4] = {r[0], r[1], r[2], r[3]};
  return key_eq(rk, k);
}

// Lookup: the slot that holds k, IV_NONE where an empty slot ends the probe.  *probes counts the slots looked
// at; *bad is set where the loop ran over every slot (no empty one: the host's load bound was broken) or met a
// pending word (none outlives the insert that wrote it).  Reads resident keys only: an earlier launch wrote them.
IV_HD uint32_t lookup(const Table& t, const uint64_t (&k)[4], uint32_t* probes, bool* bad) {
  const uint32_t n = slots_of(t), mask = n - 1;
  const uint64_t tag = tag_of(t.seed, k);
  uint32_t s = start_slot(t.seed, t.log2, k);
  for (uint32_t i = 0; i < n; ++i, s = (s + 1) & mask) {
    const uint64_t w = st_load(t.state + s);
    ++*probes;
    if (w == kEmpty) return IV_NONE;
    if (is_pending(w)) break;
    if (is_full(w) && w == full_word(tag) && resident_eq(t, s, k)) return s;
  }
  *bad = true;
  return IV_NONE;
}

// Claim, row i of rows (key k): what the probe from k's start slot ends on, as claim[i]:
//   IV_PRESENT -- a full slot whose resident key (an earlier launch's) equals k; *slot = that slot;
//   j          -- the row whose pending word stands in the slot: i itself where the row took an empty slot
//                 (compare-and-swap empty -> pending + i; on failure the same slot again, with the word that came
//                 back), another row where that row's *input* key equals k.  Either way first[j] takes the
//                 minimum with i, and *slot = the slot;
//   IV_NONE    -- the loop ran over every slot (*bad).
// No key or value byte that this launch writes is read: the launch writes none.
IV_HD uint32_t claim(const Table& t, const Rows& rows, uint32_t i, const uint64_t (&k)[4], uint32_t* first,
                     uint32_t* slot, uint32_t* probes, bool* bad) {
  const uint32_t n = slots_of(t), mask = n - 1;
  const uint64_t tag = tag_of(t.seed, k);
  uint32_t s = start_slot(t.seed, t.log2, k);
  for (uint32_t step = 0; step < n; ++step, s = (s + 1) & mask) {
    uint64_t w = st_load(t.state + s);
    ++*probes;
    if (w == kEmpty) {
      if (st_cas(t.state + s, w, pending_word(i))) {
        min_u32(first + i, i);
        *slot = s;
        return i;
      }
      // w is what the slot holds now: pending (another row of this launch took it) -- judged below
    }
    if (is_pending(w)) {
      const uint32_t j = pending_row(w);
      uint64_t kj[4];
      if (j < rows.n && row_key(rows, j, kj) && key_eq(kj, k)) {
        min_u32(first + j, i);
        *slot = s;
        return j;
      }
    } else if (is_full(w) && w == full_word(tag) && resident_eq(t, s, k)) {
      *slot = s;
      return IV_PRESENT;
    }
  }
  *bad = true;
  *slot = IV_NONE;
  return IV_NONE;
}

// Finalize, the launch after: the row that holds the slot's pending word writes the key, the value of row
// first[i] (the lowest row that carries the key) and, last, the full word.  Nothing reads them in this launch.
IV_HD void finalize_slot(const Table& t, uint32_t s, const uint64_t (&k)[4], const iv_val& v) {
  uint64_t* r = t.keys + 4ull * s;
  for (int q = 0; q < 4; ++q) r[q] = k[q];
  t.vals[s] = v;
  st_store(t.state + s, full_word(tag_of(t.seed, k)));
}

// Remove, the launch after a lookup: the tombstone into the found slot.  True for the one caller that found the
// slot full (the entry leaves the count once, however many equal rows name it).
IV_HD bool bury(const Table& t, uint32_t s) { return is_full(st_swap(t.state + s, kTomb)); }

// Rebuild: a full entry of the old table into a fresh one.  Keys are distinct, so the empty -> full claim is all:
// the claimer writes key and value behind it, and no launch reads them before the next.  False where the loop
// ran over every slot.
IV_HD bool reinsert(const Table& t, const uint64_t (&k)[4], const iv_val& v, uint32_t* probes) {
  const uint32_t n = slots_of(t), mask = n - 1;
  const uint64_t full = full_word(tag_of(t.seed, k));
  uint32_t s = start_slot(t.seed, t.log2, k);
  for (uint32_t step = 0; step < n; ++step, s = (s + 1) & mask) {
    uint64_t w = st_load(t.state + s);
    ++*probes;
    if (w != kEmpty || !st_cas(t.state + s, w, full)) continue;
    uint64_t* r = t.keys + 4ull * s;
    for (int q = 0; q < 4; ++q) r[q] = k[q];
    t.vals[s] = v;
    return true;
  }
  return false;
}

// ---- the payload walk (host) ----
// decode_payload_content("l32s") of src/network/bmproto.py:190-315 over payload[0, len), as the reference's parser
// behaves (tests/golden/inv_kats.json was made by running it): the count is a varint by addresses.decodeVarint's
// rules (empty data decodes as 0; a truncated or non-minimal one raises), and the parser then cuts
// max(count, 1) items of payload[at : at + 32] -- a count of 0 still yields one item, a payload that ends early
// yields one short item and then empty ones, and bytes behind the last item are not looked at.
#define IV_WALK_OK 0
#define IV_WALK_MALFORMED 1
struct Walk {
  uint64_t count;    // len(items) as the reference sees it
  uint64_t at;       // the payload offset of item 0
  uint64_t full;     // leading items of 32 bytes
  uint32_t tail;     // bytes of the short item behind them (0: none)
  int status;
};
inline bool walk_varint(const uint8_t* p, uint64_t len, uint64_t* value, uint64_t* used) {
  *value = 0, *used = 0;
  if (len == 0) return true;
  const uint8_t f = p[0];
  if (f < 253) {
    *value = f, *used = 1;
    return true;
  }
  const uint64_t need = f == 253 ? 3 : f == 254 ? 5 : 9;
  if (len < need) return false;
  uint64_t v = 0;
  for (uint64_t i = 1; i < need; ++i) v = (v << 8) | p[i];
  if (v < (f == 253 ? 253ull : f == 254 ? 65536ull : 4294967296ull)) return false;
  *value = v, *used = need;
  return true;
}
inline Walk walk(const uint8_t* payload, uint64_t len) {
  Walk w{};
  uint64_t count = 0, used = 0;
  if (!walk_varint(payload, len, &count, &used)) {
    w.status = IV_WALK_MALFORMED;
    return w;
  }
  w.count = count ? count : 1;
  w.at = used;
  const uint64_t avail = len - used;
  w.full = avail / 32 < w.count ? avail / 32 : w.count;
  w.tail = w.full < w.count ? (uint32_t)(avail % 32) : 0;
  return w;
}

}  // namespace ivf
