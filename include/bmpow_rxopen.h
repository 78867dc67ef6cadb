/*
 * bmpow_rxopen.h -- C ABI of libbmpow_hip.so's one-call opening of received msgs: from the objects' wire bytes
 * and the user's private keys to processmsg's verdict per object.
 *
 * The reference's processmsg (src/class_objectProcessor.py:435-747) reads the msg version and the stream
 * (:441-452), tries every key the user holds against the payload (:459-477; one pyelliptic ECC.decrypt per
 * try: ECDH, SHA-512, HMAC-SHA256, and AES-256-CBC where the MAC verifies), returns at :478 where none opens
 * it, and goes on with the plaintext as bmpow_rx.h describes.  Here a batch does all of that in one call: the
 * trial decryption of bmpow_ecies_match, then for the rows whose MAC verified an AES pass that reads the
 * ciphertext where the MAC kernel hashed it and the key where the match left it, then the nine launches of
 * bmpow_rx_msgs over the plaintexts where that pass left them.  No ciphertext is uploaded twice, key_e never
 * reaches the host, and a plaintext crosses the bus once, downwards, for matched rows only.
 *
 * Same conventions as bmpow.h (return codes, bmpow_last_error, thread safety); the call runs on the first
 * selected device in sets of at most 2^18 objects and 256 MB of padded MAC blocks, bmpow_abort() is honoured
 * between sets and between key groups, and every key is tried against every payload whatever the outcome.
 */
#ifndef BMPOW_RXOPEN_H
#define BMPOW_RXOPEN_H

#include "bmpow_rx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* processmsg from :441 to :591 for n msg objects and n_keys private encryption keys (32 big-endian bytes each,
 * privkeys32) with the ripes of their addresses (20 bytes each, ripes20).  Per object i:
 *
 *   recs[i].status        match[i]       plaintext
 *   BMPOW_RX_MSG_VERSION  -1             none   the head refuses (:444, or a head varint does not decode); the
 *                                               record is bmpow_rx_walk_msg's for an empty plaintext
 *   BMPOW_RX_NOT_MINE     -1             none   malformed payload, point off the curve, or no key's MAC verifies
 *                                               (:478); only claimed_stream and prefix_len are filled
 *   BMPOW_RX_NOT_MINE     the key index  none   the MAC verifies under that key but the ciphertext is empty or no
 *                                               multiple of 16 bytes, or its padding is refused: the reference's
 *                                               decrypt raises and the loop goes on
 *   anything else         the key index  yes    what bmpow_rx_msgs gives for (object, plaintext, ripes20[20 match]),
 *                                               bit for bit
 *
 * match[i] is the lowest index of a key whose MAC verifies.  The plaintexts are written side by side into
 * arena, in input order: plain_off[i] / plain_len[i] name object i's (both 0 where there is none).  arena_cap
 * below the sum of obj_lens is BMPOW_E_ARG before anything is launched (a plaintext is shorter than its
 * object).  A key that is 0 or not below the group order and a payload above 2^31 bytes are BMPOW_E_ARG.
 * n == 0 succeeds with nothing launched; with n_keys == 0 every well-headed object is BMPOW_RX_NOT_MINE, with
 * nothing launched either. */
BMPOW_API int bmpow_rx_sealed_msgs(size_t n, const uint8_t *const *objs, const uint64_t *obj_lens, size_t n_keys,
                                   const uint8_t *privkeys32, const uint8_t *ripes20, bmpow_rx_msg_rec *recs,
                                   int32_t *match, uint8_t *arena, uint64_t arena_cap, uint64_t *plain_off,
                                   uint64_t *plain_len);

/* Host only: what the call does with one object before any key is tried.  Returns 1 for an object that is tried
 * against the keys and could be opened; 0 with *reason set otherwise.  payload_off (where data[readPosition:]
 * starts) is filled unless the head refuses, body_off (within the payload) and clen (the ciphertext's length)
 * unless the payload is malformed. */
#define BMPOW_RXS_PLAN_OK 0
#define BMPOW_RXS_PLAN_HEAD 1    /* the head refuses: BMPOW_RX_MSG_VERSION, never tried */
#define BMPOW_RXS_PLAN_PAYLOAD 2 /* malformed payload (bmpow_ecies_parse refuses it): never tried */
#define BMPOW_RXS_PLAN_CIPHER 3  /* tried, but the ciphertext is empty or no multiple of 16: never opened */
BMPOW_API int bmpow_rx_sealed_plan(const uint8_t *obj, size_t len, size_t *payload_off, size_t *body_off, size_t *clen,
                                   int *reason);

/* Counters of bmpow_rx_sealed_msgs since the last reset; bmpow_ecies_stats and bmpow_rx_stats do not move.
 * The times are GPU time between events recorded around the launches of each phase. */
typedef struct bmpow_rx_sealed_stats {
  uint64_t calls;      /* calls that launched */
  uint64_t rows;       /* objects they were given */
  uint64_t matched;    /* rows whose ciphertext went through the opening kernel */
  uint64_t sets;       /* ECIES sets of at most 2^18 objects and 256 MB of pool */
  uint64_t launches;   /* kernel launches: 1 + 3 per key group per set, and 10 more for a set with a matched row */
  uint64_t rx_launches; /* of those, the opening kernel and the nine of the msg processing */
  uint64_t bytes_up;   /* host to device: digits, points, ec_objs, padded MAC pool, matched rows' descriptors */
  uint64_t bytes_down; /* device to host: match[], and for matched rows records, opened[] and plaintext slots */
  double match_ms;     /* key tables, ladder + SHA-512, HMAC-SHA256 and the gather */
  double open_ms;      /* AES-256-CBC of the matched rows */
  double walk_ms;      /* the six phases of bmpow_rx_stats, over the matched rows */
  double hash_ms;
  double scalar_ms;
  double curve_ms;
  double ident_ms;
  double finish_ms;
  double host_ms;      /* wall time of the calls */
} bmpow_rx_sealed_stats;

BMPOW_API int bmpow_rx_sealed_get_stats(bmpow_rx_sealed_stats *out);
BMPOW_API void bmpow_rx_sealed_reset_stats(void);

#ifdef __cplusplus
}
#endif

#endif /* BMPOW_RXOPEN_H */
