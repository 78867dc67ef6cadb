/*
 * bmpow_ident.h -- C ABI of libbmpow_hip.so's batched sender identification.
 *
 * Once a signature has verified, the reference hashes the sender's two public keys into the ripe,
 *     ripe = RIPEMD160(SHA512(04 || signX || signY || 04 || encX || encY))
 * (src/class_objectProcessor.py:311-314, :376-379, :586-589, :877-879; src/protocol.py:493-495), and
 * then either turns it into the BM-... address it stores and displays (addresses.encodeAddress,
 * src/addresses.py:146-180) or compares it, or the tag made from it, with what the object claims
 * (:882, :889-893; protocol.py:497).  The send side derives the same keys and tags for subscriptions and
 * needed pubkeys (src/shared.py:169-184, src/class_singleWorker.py:84-90).  Here a batch goes through
 * all of it in one launch, one lane per row.
 *
 * Per row, with data = varint(version) || varint(stream) || ripe, d1 = SHA512(data), d2 = SHA512(d1):
 *     key_v3  = d1[:32]   the subscription / pubkey-request key of a v2 / v3 address
 *     tag_key = d2[:32]   the same of a v4 address
 *     tag     = d2[32:]   the tag of a v4 address
 *     addr    = encodeAddress(version, stream, ripe) without its "BM-"
 * version and stream may be any 64-bit value; encodeAddress's zero-byte rule applies to versions 2, 3
 * (at most two leading zero bytes dropped) and 4 (all of them) only.
 *
 * Nothing here is secret: key_v3 and tag_key are functions of a public address, so no buffer is zeroed.
 *
 * Same conventions as bmpow.h (return codes, bmpow_last_error, thread safety); the calls run on the
 * first selected device in sets of at most 2^18 rows, bmpow_abort() is honoured between sets, and
 * n == 0 succeeds with nothing launched.
 */
#ifndef BMPOW_IDENT_H
#define BMPOW_IDENT_H

#include "bmpow.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bmpow_ident_rec {
  uint8_t ripe[20];
  uint8_t key_v3[32];
  uint8_t tag_key[32];
  uint8_t tag[32];
  uint8_t addr_len; /* characters in addr: 1 .. 58 */
  char addr[63];    /* the address after "BM-", zero padded, not terminated */
} bmpow_ident_rec;  /* 180 bytes, no padding */

/* keys128: per row pub_signing (X || Y, 64 bytes) then pub_encryption (X || Y, 64 bytes), as
 * bmpow_sig_verify takes keys.  The coordinates are hashed as given; nothing is checked against the curve. */
BMPOW_API int bmpow_ident_derive(size_t n, const uint8_t *keys128, const uint64_t *versions, const uint64_t *streams,
                                 bmpow_ident_rec *out);

/* The same from the 20-byte ripe on (out[i].ripe is the given one): encodeAddress for a batch, and the
 * keys and tags of subscriptions and needed pubkeys. */
BMPOW_API int bmpow_ident_from_ripe(size_t n, const uint8_t *ripes20, const uint64_t *versions,
                                    const uint64_t *streams, bmpow_ident_rec *out);

/* Counters of the two calls since the last reset. */
typedef struct bmpow_ident_stats {
  uint64_t calls;    /* calls that launched */
  uint64_t rows;     /* rows they were given */
  uint64_t sets;     /* sets of at most 2^18 rows */
  uint64_t launches; /* kernel launches: one per set */
  double kernel_ms;  /* GPU time between events recorded around the launches */
  double host_ms;    /* wall time of the calls: upload, launches, download */
} bmpow_ident_stats;

BMPOW_API int bmpow_ident_get_stats(bmpow_ident_stats *out);
BMPOW_API void bmpow_ident_reset_stats(void);

#ifdef __cplusplus
}
#endif

#endif /* BMPOW_IDENT_H */
