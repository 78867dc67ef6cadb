// bmpow_proc_fmt.h -- the byte-level half of the object processor's dispatch (include/bmpow_proc.h): the varint
// rules of addresses.decodeVarint, the walks of a getpubkey and of an onionpeer with their verdict chains
// (src/class_objectProcessor.py:156-268), the IP classes of protocol.checkIPAddress (src/protocol.py:150-227),
// the mix that picks a watched key's slot and tag, the compare of two byte runs at any offsets, and the probes of
// the watch index and of the address table -- written once for the device (bmpow_proc.hip), for the host unit
// (bmpow_host_proc.hip) and for the stand-alone test program (tests/native/proc_sim.cpp builds this header with
// g++).  Every byte is read through ivf::load_word: aligned 8-byte loads that never touch a byte at or past the
// buffer's end.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "bmpow_inv_fmt.h"

#define PC_HD IV_HD

#define PC_NONE 0xffffffffu  // no entry / no row / no address

// record values, restated by include/bmpow_proc.h (static_asserts in bmpow_host_proc.hip tie the two)
enum {
  PC_ROUTE_GETPUBKEY = 0, PC_ROUTE_PUBKEY = 1, PC_ROUTE_MSG = 2, PC_ROUTE_BROADCAST = 3, PC_ROUTE_ONIONPEER = 4,
  PC_ROUTE_UNKNOWN_TYPE = 5
};
enum { PC_ACK_NOT_CHECKED = 0, PC_ACK_NOT_WATCHED = 1, PC_ACK_FOUND = 2, PC_ACK_FOUND_EARLIER = 3 };
enum {
  PC_NONE_STATUS = 0, PC_TOO_LONG = 1, PC_MALFORMED = 2, PC_VERSION_ZERO = 3, PC_VERSION_ONE = 4,
  PC_VERSION_TOO_HIGH = 5, PC_SHORT_HASH = 6, PC_SHORT_TAG = 7, PC_NOT_MINE = 8, PC_VERSION_MISMATCH = 9,
  PC_STREAM_MISMATCH = 10, PC_CHAN = 11, PC_SENT_RECENTLY = 12, PC_SEND_V2 = 13, PC_SEND_V3 = 14, PC_SEND_V4 = 15,
  PC_NO_HOST = 16, PC_RAISES = 17, PC_PEER = 18
};
enum { PC_HOST_NONE = 0, PC_HOST_V4 = 1, PC_HOST_ONION = 2, PC_HOST_V6 = 3 };

#define PC_TYPE_ONIONPEER 0x746f72u  // protocol.OBJECT_ONIONPEER
#define PC_GETPUBKEY_MAX 200u        // len(data) > 200: "abnormally long"
#define PC_ONION_HEAD 64u            // 20 + three varints of 9 bytes at most + the host's first 16 bytes, rounded up
#define PC_PUBKEY_INTERVAL 2419200   // 28 days

// One record, laid out as bmpow_proc_rec.
struct pc_rec {
  uint64_t version, stream, port;
  uint32_t route, ack, ack_aux, ack_first;
  uint32_t status, key_off, key_len, address;
  uint32_t host_off, host_len, host_class, reserved;
};

// One of my addresses, laid out as bmpow_proc_address.
struct pc_addr {
  uint8_t ripe[20];
  uint8_t tag[32];
  uint32_t version;
  uint64_t stream;
  int64_t last_pubkey_send_time;
  uint32_t chan;
  uint32_t reserved;
};

namespace pcf {

using ivf::fmix;
using ivf::load_word;

// ---- bytes ----
// A run of bytes inside a pool: `avail` bytes from byte offset off of buf (nbytes in all, base 8-byte aligned),
// standing for the first bytes of an object of `len` bytes (avail <= len: the host uploads only what a verdict
// can depend on).
struct Bytes {
  const uint64_t* buf;
  uint64_t nbytes;
  uint64_t off;
  uint32_t avail;
  uint32_t len;
};
PC_HD uint8_t byte_at(const Bytes& b, uint32_t i) {  // i < avail
  const uint64_t at = b.off + i;
  return (uint8_t)(load_word(b.buf, b.nbytes, at >> 3) >> (8 * (uint32_t)(at & 7)));
}
// The 8 bytes at byte offset off as a little-endian number, zero for bytes at or past nbytes: two aligned loads
// funnelled by off mod 8 (one where off is aligned).
PC_HD uint64_t load_u64_at(const uint64_t* buf, uint64_t nbytes, uint64_t off) {
  const uint64_t q = off >> 3;
  const uint32_t sh = 8 * (uint32_t)(off & 7);
  const uint64_t lo = load_word(buf, nbytes, q);
  if (sh == 0) return lo;
  return (lo >> sh) | (load_word(buf, nbytes, q + 1) << (64 - sh));
}
PC_HD uint64_t low_bytes(uint64_t w, uint32_t n) { return n >= 8 ? w : w & ((1ull << (8 * n)) - 1ull); }  // n >= 1
// len bytes at offset oa of a against len bytes at offset ob of b; both runs lie inside their buffers.
PC_HD bool bytes_eq(const uint64_t* a, uint64_t na, uint64_t oa, const uint64_t* b, uint64_t nb, uint64_t ob, uint32_t len) {
  if (oa + len > na || ob + len > nb) return false;  // never: the host planned both runs inside their pools
  for (uint32_t i = 0; i < len; i += 8) {
    const uint32_t rem = len - i;
    if (low_bytes(load_u64_at(a, na, oa + i) ^ load_u64_at(b, nb, ob + i), rem) != 0) return false;
  }
  return true;
}

// ---- the varint ----
// addresses.decodeVarint(data[at : at + 10]) (src/addresses.py:82-134) over the object's first `len` bytes: an
// empty slice decodes as (0, 0); false for varintDecodeError (truncated, or not the shortest encoding).  A walk
// reads below avail only: the host uploaded every byte a varint can reach.
PC_HD bool varint(const Bytes& b, uint32_t at, uint64_t* value, uint32_t* used) {
  *value = 0, *used = 0;
  const uint32_t end = b.len < b.avail ? b.len : b.avail;
  if (at >= end) return true;
  const uint32_t have = end - at < 10 ? end - at : 10;
  const uint8_t f = byte_at(b, at);
  if (f < 253) {
    *value = f, *used = 1;
    return true;
  }
  const uint32_t need = f == 253 ? 3 : f == 254 ? 5 : 9;
  if (have < need) return false;
  uint64_t v = 0;
  for (uint32_t i = 1; i < need; ++i) v = (v << 8) | byte_at(b, at + i);
  if (v < (f == 253 ? 253ull : f == 254 ? 65536ull : 4294967296ull)) return false;
  *value = v, *used = need;
  return true;
}

// ---- the address table ----
// The rows of shared.myAddressesByHash / myAddressesByTag with two open-addressing indexes over them, built on the
// host (fill_index): 2^log2 slots each, at least twice the rows, a slot the row number or PC_NONE.
struct AddrTable {
  const pc_addr* rows;
  const uint32_t* by_ripe;  // [1 << log2]
  const uint32_t* by_tag;   // [1 << log2]
  uint32_t n;
  uint32_t log2;
};
PC_HD uint64_t key_word(const Bytes& b, uint32_t at) {  // the 8 bytes at `at` (inside avail), little-endian
  uint64_t w = 0;
  for (uint32_t i = 0; i < 8; ++i) w |= (uint64_t)byte_at(b, at + i) << (8 * i);
  return w;
}
PC_HD uint64_t key_word(const uint8_t* p) {
  uint64_t w = 0;
  for (uint32_t i = 0; i < 8; ++i) w |= (uint64_t)p[i] << (8 * i);
  return w;
}
PC_HD uint32_t addr_slot(uint64_t first8, uint32_t log2) { return log2 ? (uint32_t)(fmix(first8 ^ 0x9e3779b97f4a7c15ULL) >> (64 - log2)) : 0; }
// The row whose ripe (tag false: 20 bytes) or tag (32 bytes) equals the bytes at `at` of b, or PC_NONE.
PC_HD uint32_t addr_find(const AddrTable& t, const Bytes& b, uint32_t at, bool tag) {
  if (t.n == 0 || !t.rows) return PC_NONE;
  const uint32_t slots = 1u << t.log2, mask = slots - 1, width = tag ? 32 : 20;
  const uint32_t* index = tag ? t.by_tag : t.by_ripe;
  uint32_t s = addr_slot(key_word(b, at), t.log2);
  for (uint32_t step = 0; step < slots; ++step, s = (s + 1) & mask) {
    const uint32_t r = index[s];
    if (r == PC_NONE) return PC_NONE;
    if (r >= t.n) return PC_NONE;  // never: the host wrote row numbers
    const uint8_t* k = tag ? t.rows[r].tag : t.rows[r].ripe;
    bool eq = true;
    for (uint32_t i = 0; i < width; ++i) eq = eq && k[i] == byte_at(b, at + i);
    if (eq) return r;
  }
  return PC_NONE;
}
// Host: both indexes of n rows into 2^log2 slots each (2^log2 >= 2 n).  False for two rows with one ripe or tag.
inline bool fill_index(const pc_addr* rows, uint32_t n, uint32_t log2, uint32_t* by_ripe, uint32_t* by_tag) {
  const uint32_t slots = 1u << log2, mask = slots - 1;
  for (uint32_t s = 0; s < slots; ++s) by_ripe[s] = by_tag[s] = PC_NONE;
  for (int which = 0; which < 2; ++which) {
    uint32_t* index = which ? by_tag : by_ripe;
    const uint32_t width = which ? 32 : 20;
    for (uint32_t r = 0; r < n; ++r) {
      const uint8_t* k = which ? rows[r].tag : rows[r].ripe;
      uint32_t s = addr_slot(key_word(k), log2);
      for (; index[s] != PC_NONE; s = (s + 1) & mask) {
        const uint8_t* o = which ? rows[index[s]].tag : rows[index[s]].ripe;
        bool eq = true;
        for (uint32_t i = 0; i < width; ++i) eq = eq && o[i] == k[i];
        if (eq) return false;
      }
      index[s] = r;
    }
  }
  return true;
}
PC_HD uint32_t addr_log2_for(uint32_t n) {
  uint32_t l = 1;
  while ((1ull << l) < 2ull * n) ++l;
  return l;
}

// ---- processgetpubkey (src/class_objectProcessor.py:176-268) ----
// The first refusal in the reference's order, or the worker command.  b holds the object's first bytes (all of
// them: an object above 200 bytes is TOO_LONG before any byte is read).  `now` stands for time.time().
PC_HD void walk_getpubkey(const Bytes& b, const AddrTable& t, int64_t now, pc_rec* r) {
  r->address = PC_NONE;
  if (b.len > PC_GETPUBKEY_MAX) {  // :179-182
    r->status = PC_TOO_LONG;
    return;
  }
  uint64_t version = 0, stream = 0;
  uint32_t l1 = 0, l2 = 0;
  if (!varint(b, 20, &version, &l1) || !varint(b, 20 + l1, &stream, &l2)) {  // :184-189
    r->status = PC_MALFORMED;
    return;
  }
  r->version = version, r->stream = stream;
  if (version == 0 || version == 1 || version > 4) {  // :191-202
    r->status = version == 0 ? PC_VERSION_ZERO : version == 1 ? PC_VERSION_ONE : PC_VERSION_TOO_HIGH;
    return;
  }
  const uint32_t at = 20 + l1 + l2, want = version <= 3 ? 20 : 32;  // at <= len: version >= 2 was read from inside
  const uint32_t end = b.len < b.avail ? b.len : b.avail;
  const uint32_t got = at >= end ? 0 : (end - at < want ? end - at : want);
  r->key_off = at, r->key_len = got;
  if (got != want) {  // :207-210, :219-222
    r->status = version <= 3 ? PC_SHORT_HASH : PC_SHORT_TAG;
    return;
  }
  const uint32_t a = addr_find(t, b, at, version >= 4);  // :215-216, :226-227
  if (a == PC_NONE) {
    r->status = PC_NOT_MINE;  // :229-231
    return;
  }
  r->address = a;
  const pc_addr& row = t.rows[a];
  if (row.version != version) r->status = PC_VERSION_MISMATCH;                               // :233-238
  else if (row.stream != stream) r->status = PC_STREAM_MISMATCH;                            // :239-244
  else if (row.chan) r->status = PC_CHAN;                                                   // :245-249
  else if (row.last_pubkey_send_time > now - PC_PUBKEY_INTERVAL) r->status = PC_SENT_RECENTLY;  // :250-258
  else r->status = version == 2 ? PC_SEND_V2 : version == 3 ? PC_SEND_V3 : PC_SEND_V4;      // :263-268
}

// ---- protocol.checkIPAddress(host) with private=False (src/protocol.py:150-227) ----
// Over the host's first min(n, 16) bytes h[] and its length n.  PC_PEER with *cls, PC_NO_HOST (False), or
// PC_RAISES: socket.inet_ntop(AF_INET, host[12:]) on other than 4 bytes raises ValueError, which nothing between
// there and the run loop's `except Exception` catches.
PC_HD uint32_t ip_class(const uint8_t (&h)[16], uint32_t n, uint32_t* cls) {
  *cls = PC_HOST_NONE;
  bool mapped = n >= 12;
  for (uint32_t i = 0; i < 12 && mapped; ++i) mapped = h[i] == (i < 10 ? 0x00 : 0xff);
  if (mapped) {  // :155-157, checkIPv4Address :176-202
    if (n != 16) return PC_RAISES;
    if (h[12] == 0x7f || h[12] == 0x0a) return PC_NO_HOST;
    if (h[12] == 0xc0 && h[13] == 0xa8) return PC_NO_HOST;
    if (h[12] == 0xac && h[13] >= 0x10 && h[13] < 0x20) return PC_NO_HOST;
    *cls = PC_HOST_V4;
    return PC_PEER;
  }
  if (n >= 6 && h[0] == 0xfd && h[1] == 0x87 && h[2] == 0xd8 && h[3] == 0x7e && h[4] == 0xeb && h[5] == 0x43) {
    *cls = PC_HOST_ONION;  // :158-163: whatever follows the prefix, of any length
    return PC_PEER;
  }
  if (n != 16) return PC_NO_HOST;  // :165-168 inet_ntop(AF_INET6) raises ValueError, caught
  bool loopback = h[15] == 1;      // checkIPv6Address :205-227
  for (uint32_t i = 0; i < 15 && loopback; ++i) loopback = h[i] == 0;
  if (loopback) return PC_NO_HOST;
  if (h[0] == 0xfe && (h[1] & 0xc0) == 0x80) return PC_NO_HOST;
  if ((h[0] & 0xfe) == 0xfc) return PC_NO_HOST;
  *cls = PC_HOST_V6;
  return PC_PEER;
}

// ---- processonion (src/class_objectProcessor.py:156-174) ----
// b holds the object's first min(len, PC_ONION_HEAD) bytes: three varints from offset 20 (the first one's value
// is not used) and the host, data[at:], of which the class reads 16 bytes and the length.
PC_HD void walk_onion(const Bytes& b, pc_rec* r) {
  uint64_t v = 0, stream = 0, port = 0;
  uint32_t l0 = 0, l1 = 0, l2 = 0;
  if (!varint(b, 20, &v, &l0) || !varint(b, 20 + l0, &stream, &l1) || !varint(b, 20 + l0 + l1, &port, &l2)) {
    r->status = PC_MALFORMED;
    return;
  }
  r->stream = stream, r->port = port;
  const uint32_t at = 20 + l0 + l1 + l2;
  const uint32_t n = at >= b.len ? 0 : b.len - at;  // len(data[at:])
  uint8_t h[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (uint32_t i = 0; i < 16 && i < n && at + i < b.avail; ++i) h[i] = byte_at(b, at + i);
  uint32_t cls = PC_HOST_NONE;
  r->status = ip_class(h, n, &cls);
  r->host_class = cls;
  if (r->status == PC_PEER) r->host_off = at, r->host_len = n;
}

// ---- the watch set's index ----
// Slot and tag of a watched key come from one mix of the seed, the key's length and its first 16 bytes (zeros
// behind a shorter key), so that keys equal in those have equal tags and one start slot: a tag match is a hint,
// the resident key's length and bytes decide.  The keys are our own ack data, never a peer's choice; what a peer
// chooses, the tails it sends, costs a probe no longer than our own keys' longest cluster.
PC_HD uint64_t watch_mix(uint64_t seed, uint32_t len, uint64_t w0, uint64_t w1) {
  return fmix(fmix(fmix(seed ^ 0x9e3779b97f4a7c15ULL) ^ len) + w0) ^ fmix(w1 + 0xc2b2ae3d27d4eb4fULL);
}
PC_HD uint32_t watch_slot(uint64_t mix, uint32_t log2) { return (uint32_t)(fmix(mix) >> (64 - log2)); }  // 1 <= log2
PC_HD uint64_t watch_tag(uint64_t mix) { return mix | (1ull << 63); }                                    // never 0: 0 is empty

struct pc_entry {  // one watched key: where its bytes lie in the key pool, and the caller's aux
  uint32_t off, len, aux;
};
struct WatchTable {
  const uint64_t* tags;     // [1 << log2]: 0 empty, else the tag
  const uint32_t* slot_entry;  // [1 << log2]
  const pc_entry* entries;  // [n]
  const uint64_t* pool;     // the keys back to back
  uint64_t pool_bytes;
  uint64_t seed;
  uint32_t n;
  uint32_t log2;
};
// The entry whose key equals the len bytes at offset off of buf (a run inside nbytes; len >= 16), or PC_NONE.
PC_HD uint32_t watch_find(const WatchTable& t, const uint64_t* buf, uint64_t nbytes, uint64_t off, uint32_t len) {
  if (t.n == 0 || len < 16 || off + len > nbytes) return PC_NONE;
  const uint32_t slots = 1u << t.log2, mask = slots - 1;
  const uint64_t mix = watch_mix(t.seed, len, load_u64_at(buf, nbytes, off), load_u64_at(buf, nbytes, off + 8));
  const uint64_t tag = watch_tag(mix);
  uint32_t s = watch_slot(mix, t.log2);
  for (uint32_t step = 0; step < slots; ++step, s = (s + 1) & mask) {
    const uint64_t w = t.tags[s];
    if (w == 0) return PC_NONE;
    if (w != tag) continue;
    const uint32_t e = t.slot_entry[s];
    if (e >= t.n) continue;  // never
    const pc_entry& ent = t.entries[e];
    if (ent.len == len && bytes_eq(buf, nbytes, off, t.pool, t.pool_bytes, ent.off, len)) return e;
  }
  return PC_NONE;
}
// Host: entry e under its mix into the first free slot from its start slot (the index is at most half full).
inline void watch_place(uint64_t* tags, uint32_t* slot_entry, uint32_t log2, uint64_t mix, uint32_t e) {
  const uint32_t mask = (1u << log2) - 1;
  uint32_t s = watch_slot(mix, log2);
  while (tags[s] != 0) s = (s + 1) & mask;
  tags[s] = watch_tag(mix), slot_entry[s] = e;
}
// Host: the mix of a key given as plain bytes.
inline uint64_t watch_mix_of(uint64_t seed, const uint8_t* key, uint32_t len) {
  uint8_t head[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (uint32_t i = 0; i < 16 && i < len; ++i) head[i] = key[i];
  return watch_mix(seed, len, key_word(head), key_word(head + 8));
}
PC_HD uint32_t watch_log2_for(uint64_t n) {  // at least 8 slots, at least twice the entries
  uint32_t l = 3;
  while ((1ull << l) < 2 * n) ++l;
  return l;
}

}  // namespace pcf
