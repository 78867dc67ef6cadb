// bmpow_packets_fmt.h -- the byte-oriented half of the packet framing (include/bmpow_packets.h): the walk over
// a connection buffer's headers by the reference's rules (src/network/bmproto.py:85-156), the rows the device
// packs, and the packing of a row's bytes into padded SHA-512 blocks from a source at any byte offset --
// written once for the device (bmpow_packets.hip), for the host unit (bmpow_host_packets.hip) and for the
// stand-alone test program (tests/native/packets_sim.cpp builds this header with g++).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/bmpow_packets.h"

#if defined(__HIPCC__)
#define PK_HD __host__ __device__ __forceinline__
#else
#define PK_HD inline
#endif
#if defined(__clang__)
#define PK_UNROLL _Pragma("unroll")
#else
#define PK_UNROLL
#endif

// One packed row: payload bytes [src, src + len) of the arena (every connection buffer back to back).
//   PK_OBJECT : the pool gets object[8:] = arena[src + 8, src + len) padded, at block blk, and the row's
//               bv_obj the nonce arena[src, src + 8); len >= 20
//   PK_SUM    : the pool gets the whole payload padded; len >= 1
struct pk_row {
  uint32_t src;
  uint32_t len;
  uint32_t blk;
  uint32_t kind;
};
#define PK_OBJECT 0u
#define PK_SUM 1u
#define PK_PACK_LANES 16u  // lanes per row of pk_pack_kernel: four rows per wave

namespace pkf {

PK_HD uint32_t padded_blocks(uint64_t m) { return (uint32_t)((m + 17 + 127) / 128); }
// bytes of a row that are hashed from the pool, and the pool blocks they take
PK_HD uint32_t row_data_len(uint32_t kind, uint32_t len) { return kind == PK_OBJECT ? (len >= 8 ? len - 8 : 0) : len; }
PK_HD uint32_t row_blocks(uint32_t kind, uint32_t len) {
  return kind == PK_OBJECT && len < 8 ? 0u : padded_blocks(row_data_len(kind, len));
}

PK_HD uint32_t load_be32(const uint8_t* p) {
  return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
}

// Chunk c (16 bytes) of  data || 0x80 || zeros || bit length  in nblk 128-byte blocks as four words in memory
// order, where data is the m bytes at byte offset s of the arena.  The arena is read as aligned 16-byte
// chunks only (arena16[q], q < arena_chunks; a chunk past the end reads as zeros): the two that hold the
// destination chunk's bytes, funnelled by s mod 16.  c < 8 nblk, nblk == padded_blocks(m).
PK_HD void pack_chunk(uint32_t c, uint32_t nblk, const uint32_t* arena16, uint64_t arena_chunks, uint64_t s, uint32_t m,
                      uint32_t (&w)[4]) {
  const uint64_t at = 16ull * c;
  PK_UNROLL
  for (int q = 0; q < 4; ++q) w[q] = 0;
  if (at < m) {
    const uint64_t q0 = (s + at) >> 4;
    const uint32_t sh = (uint32_t)(s & 15u), ws = sh >> 2, bs = 8 * (sh & 3u);
    uint32_t in[8];
    PK_UNROLL
    for (int h = 0; h < 2; ++h) {
      const bool ok = q0 + (uint64_t)h < arena_chunks;
      const uint32_t* p = arena16 + 4 * (ok ? q0 + (uint64_t)h : 0);
      PK_UNROLL
      for (int q = 0; q < 4; ++q) in[4 * h + q] = ok ? p[q] : 0u;
    }
    uint32_t t[5];
    PK_UNROLL
    for (int j = 0; j < 5; ++j) t[j] = ws == 0 ? in[j] : ws == 1 ? in[j + 1] : ws == 2 ? in[j + 2] : in[j + 3];
    PK_UNROLL
    for (int j = 0; j < 4; ++j) w[j] = (uint32_t)((((uint64_t)t[j + 1] << 32) | t[j]) >> bs);
    if (at + 16 <= m) return;  // wholly inside the data
  }
  // the chunk holds the data's end, padding or the length: byte by byte
  const uint64_t total = 128ull * nblk, bits = (uint64_t)m * 8;
  PK_UNROLL
  for (int j = 0; j < 16; ++j) {
    const uint64_t i = at + (uint64_t)j;
    const uint32_t keep = i < m ? 0xffu : 0u;
    uint32_t b = (w[j >> 2] >> (8 * (j & 3))) & keep;
    if (i == m) b = 0x80;
    else if (i > m && i + 8 >= total) b = (uint32_t)(bits >> (8 * (total - 1 - i))) & 0xffu;
    w[j >> 2] = (w[j >> 2] & ~(0xffu << (8 * (j & 3)))) | (b << (8 * (j & 3)));
  }
}

// ---- the walk over a buffer's headers (host) ----

// The handler "bm_command_" + command.lower() names, of the 12 command bytes with their trailing NULs
// stripped; exact: spelled in lower case as the handler is (the comparisons of :113-114 and of
// ackDataHasAValidHeader are case-sensitive, the getattr of :121-122 is not).
inline uint8_t command_of(const uint8_t* cmd12, uint8_t* exact) {
  static const char* const kNames[] = {"error", "getdata", "inv",  "dinv", "object", "addr",
                                       "portcheck", "ping", "pong", "verack", "version"};
  size_t n = 12;
  while (n > 0 && cmd12[n - 1] == 0) --n;
  *exact = 0;
  for (size_t k = 0; k < sizeof(kNames) / sizeof(kNames[0]); ++k) {
    const char* nm = kNames[k];
    size_t l = 0;
    while (nm[l]) ++l;
    if (l != n) continue;
    bool same = true, lower = true;
    for (size_t i = 0; i < n; ++i) {
      const uint8_t ch = cmd12[i], lo = ch >= 'A' && ch <= 'Z' ? (uint8_t)(ch + 32) : ch;
      same = same && lo == (uint8_t)nm[i];
      lower = lower && ch == (uint8_t)nm[i];
    }
    if (same) {
      *exact = lower ? 1 : 0;
      return (uint8_t)(k + 1);
    }
  }
  return BMPOW_PKT_UNIMPLEMENTED;
}

// The header at p (24 bytes) into r: every field but conn, offset and intake; the status that needs no hash.
inline void header_into(const uint8_t* p, bool established, bmpow_packet_rec* r) {
  r->length = load_be32(p + 16);
  r->command = command_of(p + 4, &r->exact);
  r->reserved = 0;
  r->checksum = load_be32(p + 20);
  r->computed = 0;
  r->reserved2 = 0;
  uint32_t st = BMPOW_PKT_OK;
  if (r->length > BMPOW_PKT_MAX_MESSAGE) st |= BMPOW_PKT_TOO_LONG;  // :99-100
  const bool early = r->exact && (r->command == BMPOW_PKT_ERROR || r->command == BMPOW_PKT_VERSION ||
                                  r->command == BMPOW_PKT_VERACK);
  if (!established && !early) st |= BMPOW_PKT_NOT_ESTABLISHED;  // :113-118
  r->status = st;
}

// What a judged packet does to the walk of its connection (:119-156): 0 go on, else the close reason.
inline uint32_t after_packet(const bmpow_packet_rec& r, bool datagram) {
  if (r.status != BMPOW_PKT_OK) return datagram ? BMPOW_PKT_OPEN : BMPOW_PKT_INVALID_COMMAND;  // :144-151
  if (r.command == BMPOW_PKT_VERSION || r.command == BMPOW_PKT_VERACK) return BMPOW_PKT_HANDSHAKE;
  return BMPOW_PKT_OPEN;
}

// Walk buf[0, len) (len < 2^32).  emit(rec) is called per framed packet, its intake left untouched.  all: every
// packet that has all its bytes is emitted and nothing but a bad magic on a stream socket ends the walk (what
// the batch hashes, to judge afterwards); else the walk ends as after_packet says, the checksums taken for
// good.  Returns the packets framed; *consumed and *close as bmpow_packet_conn's.
template <class Emit>
inline uint64_t walk(const uint8_t* buf, uint64_t len, uint32_t flags, bool all, uint64_t* consumed, uint32_t* close,
                     Emit&& emit) {
  const bool established = (flags & BMPOW_PKT_CONN_ESTABLISHED) != 0, datagram = (flags & BMPOW_PKT_CONN_DATAGRAM) != 0;
  uint64_t at = 0, n = 0;
  *close = BMPOW_PKT_OPEN;
  while (len - at >= BMPOW_PKT_HEADER) {
    const uint8_t* p = buf + at;
    if (load_be32(p) != BMPOW_PKT_MAGIC) {  // :90-98
      if (!datagram) {
        *close = BMPOW_PKT_BAD_MAGIC;
        break;
      }
      ++at;
      continue;
    }
    bmpow_packet_rec r{};
    r.offset = (uint32_t)at;
    header_into(p, established, &r);
    if (len - at - BMPOW_PKT_HEADER < r.length) break;  // expectBytes = payloadLength, for a TOO_LONG one too
    emit(r);
    ++n;
    const uint32_t end = all ? (uint32_t)BMPOW_PKT_OPEN : after_packet(r, datagram);
    if (end == BMPOW_PKT_INVALID_COMMAND) {
      *close = end;
      break;
    }
    at += (uint64_t)BMPOW_PKT_HEADER + r.length;
    if (end == BMPOW_PKT_HANDSHAKE) {
      *close = end;
      break;
    }
  }
  *consumed = at;
  return n;
}

}  // namespace pkf
