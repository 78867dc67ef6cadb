/*
 * bmpow_rxobjopen.h -- C ABI of libbmpow_hip.so's one-call opening of received broadcasts and pubkeys: from the
 * objects' wire bytes and the keys their addresses give to the verdict of processbroadcast
 * (src/class_objectProcessor.py:749-973), processpubkey (:270-433) and decryptAndCheckPubkeyPayload
 * (src/protocol.py:401-518) per object.
 *
 * The reference tries a v4 broadcast against the key of every v2 / v3 subscription (:779-801), a v5 broadcast
 * against the one key filed under its tag (:808-820), and an encrypted v4 pubkey against the key of the address
 * that state.neededPubkeys files under its tag (src/protocol.py:411-457).  Here a batch does all of that in one
 * call: the heads are walked on the host, the tags looked up in a hash table built once per call, and per set of
 * the ECIES pool (uploaded once) the trial keys run over the v4 broadcasts as bmpow_ecies_match runs them while
 * one launch derives the key of every tagged row from that row's own table entry; the rows whose MAC verified
 * are decrypted where the MAC kernel hashed them, and the nine launches of bmpow_rx_objects read the plaintexts
 * where that pass left them.  Clear v2 / v3 pubkeys take no key and go through the same nine launches as
 * uploaded rows.  No ciphertext is uploaded twice, key_e never reaches the host, and a plaintext crosses the bus
 * once, downwards, for matched rows only.
 *
 * Same conventions as bmpow.h (return codes, bmpow_last_error, thread safety); the call runs on the first
 * selected device in sets of at most 2^18 objects and 256 MB of padded MAC blocks, and bmpow_abort() is honoured
 * between sets and between key groups.
 */
#ifndef BMPOW_RXOBJOPEN_H
#define BMPOW_RXOBJOPEN_H

#include "bmpow_rxopen.h"

#ifdef __cplusplus
extern "C" {
#endif

/* needed_flags[] bits: what the wrapper found when it resolved the entry's address */
#define BMPOW_RXOS_NEEDED_DECODED 1 /* the address decoded (status 'success') */
#define BMPOW_RXOS_NEEDED_OWN_TAG 2 /* the tag the entry is filed under is the address's own */

/* The three key tables of a call.  Private keys are 32 big-endian bytes, ripes 20 bytes, tags 32 bytes, entry
 * after entry.  A table may be empty (its pointers are then not looked at).
 *
 * A tag that appears twice in tag32[] or in needed_tag32[]: the FIRST entry wins, as dict.setdefault keeps the
 * first subscription of reloadBroadcastSendersForWhichImWatching; the later entry is never tried and match[]
 * never names it.  It is no error.
 *
 * Every trial key, every tag key, and the key of every needed entry whose flags have both bits set must be in
 * 1 .. n - 1 (n the group order): BMPOW_E_ARG otherwise.  The key, ripe, version and stream of a needed entry
 * whose address did not decode are not looked at. */
typedef struct bmpow_rx_obj_tables {
  size_t n_trial;               /* trial keys: the v2 / v3 subscriptions, each tried against every v4 broadcast */
  const uint8_t *trial_priv32;
  const uint8_t *trial_ripe20;
  size_t n_tags;                /* subscription tags: the v4+ subscriptions, one key per tag */
  const uint8_t *tag32;
  const uint8_t *tag_priv32;
  size_t n_needed;              /* needed pubkeys: the tag each is filed under and what its address resolved to */
  const uint8_t *needed_tag32;
  const uint8_t *needed_priv32;
  const uint8_t *needed_ripe20;
  const uint64_t *needed_version;
  const uint64_t *needed_stream;
  const uint8_t *needed_flags;  /* BMPOW_RXOS_NEEDED_* */
} bmpow_rx_obj_tables;

/* n objects as they came off the wire, each with its kind: BMPOW_RXO_KIND_BROADCAST or BMPOW_RXO_KIND_PUBKEY
 * (any other value, BMPOW_RXO_KIND_PUBKEY_V4 included, is BMPOW_E_ARG: the call itself routes a pubkey that
 * processpubkey hands to decryptAndCheckPubkeyPayload, :410, to BMPOW_RXO_KIND_PUBKEY_V4).  Per object i the
 * record recs[i], match[i] and the plaintext are what the composition of bmpow_rx_walk_object, the table
 * lookups, bmpow_ecies_match + bmpow_aes256_cbc and bmpow_rx_objects gives, bit for bit:
 *
 *   a broadcast whose head refuses      the record of the header walk (BMPOW_RXO_VARINT, BMPOW_RXO_BC_VERSION)
 *   a v4 broadcast                      BMPOW_RXO_NOT_SUBSCRIBED over the header's record unless a trial key's
 *                                       MAC verifies and its plaintext opens (:801); match[i] is the lowest index
 *                                       of a trial key whose MAC verifies; the row's expected ripe is that key's
 *   a v5 broadcast                      BMPOW_RXO_NOT_SUBSCRIBED where its tag (32 whole bytes) is in no entry of
 *                                       tag32[] (:810); else BMPOW_RXO_NOT_DECRYPTED unless the entry's key opens
 *                                       it (:820); match[i] is the entry's index where the MAC verifies
 *   a clear pubkey (version not 4)      what bmpow_rx_objects gives for it; no key, match[i] is -1
 *   a v4 pubkey                         in the order of src/protocol.py:411-457: BMPOW_RXO_V4_TOO_SHORT below
 *                                       350 bytes; BMPOW_RXO_NOT_NEEDED where its tag is in no entry of
 *                                       needed_tag32[]; BMPOW_RXO_ADDRESS_MISMATCH where the entry's address
 *                                       did not decode or its version or stream is not the object's;
 *                                       BMPOW_RXO_NOT_NEEDED where the entry's tag is not the address's own;
 *                                       BMPOW_RXO_NOT_DECRYPTED unless the entry's key opens it; match[i] is the
 *                                       entry's index where the MAC verifies; the expected ripe is the entry's
 *
 * A MAC that verifies over a ciphertext that is empty, no multiple of 16 bytes, or badly padded leaves the
 * status of a row no key opened, match[i] set, and no plaintext (the reference's decrypt raises).  Every row that
 * opened goes through the nine launches of bmpow_rx_objects with its plaintext and expected ripe.
 *
 * The plaintexts are written side by side into arena, in input order: plain_off[i] / plain_len[i] name object
 * i's (both 0 where there is none; a clear pubkey has none: its source is the object).  arena_cap below the sum
 * of obj_lens is BMPOW_E_ARG before anything is launched, as are a key out of range and an object above 2^31
 * bytes.  n == 0 succeeds with nothing launched; with all three tables empty nothing that needs a key is
 * launched (clear pubkeys still take their nine). */
BMPOW_API int bmpow_rx_sealed_objects(size_t n, const uint8_t *kinds, const uint8_t *const *objs,
                                      const uint64_t *obj_lens, const bmpow_rx_obj_tables *tables,
                                      bmpow_rx_obj_rec *recs, int32_t *match, uint8_t *arena, uint64_t arena_cap,
                                      uint64_t *plain_off, uint64_t *plain_len);

/* Host only: what the call decides about one object of the given kind before any table is looked at or key
 * tried.  Returns 1 for an object that would be tried against a key and could be opened; 0 with *reason set
 * otherwise (BMPOW_RXS_PLAN_* of bmpow_rxopen.h and the two below).  *routed is the kind after routing;
 * payload_off and tag_off (the header's; tag_off == payload_off for a v4 broadcast) are filled unless the head
 * refuses, body_off (within the payload) and clen unless the payload is malformed too. */
#define BMPOW_RXOS_PLAN_CLEAR 4    /* a pubkey that is not version 4: no key is involved */
#define BMPOW_RXOS_PLAN_V4_SHORT 5 /* a v4 pubkey below 350 bytes: BMPOW_RXO_V4_TOO_SHORT, never tried */
BMPOW_API int bmpow_rx_sealed_object_plan(int kind, const uint8_t *obj, size_t len, int *routed, size_t *payload_off,
                                          size_t *tag_off, size_t *body_off, size_t *clen, int *reason);

/* Counters of bmpow_rx_sealed_objects since the last reset; bmpow_ecies_stats, bmpow_rx_stats,
 * bmpow_rx_obj_stats and bmpow_rx_sealed_stats do not move.  The times are GPU time between events recorded
 * around the launches of each phase. */
typedef struct bmpow_rx_sealed_obj_stats {
  uint64_t calls;        /* calls that launched */
  uint64_t rows;         /* objects they were given */
  uint64_t matched;      /* rows whose ciphertext went through the opening kernel */
  uint64_t clear;        /* clear pubkeys uploaded as rows */
  uint64_t sets;         /* ECIES sets of at most 2^18 objects and 256 MB of pool */
  uint64_t launches;     /* kernel launches: per set 1, 3 per trial-key group and 3 for its tagged rows, 10 more
                            for a set with a matched row; 9 per set of clear pubkeys */
  uint64_t rx_launches;  /* of those, the opening kernel and the nine of the object processing */
  uint64_t tagged_tries; /* (row, key) pairs of rows tried against the one key their tag names */
  uint64_t trial_tries;  /* (row, key) pairs of v4 broadcasts against the trial keys */
  uint64_t bytes_up;     /* host to device: digits, key indices, points, ec_objs, padded MAC pool, matched rows'
                            descriptors, clear pubkeys and their descriptors */
  uint64_t bytes_down;   /* device to host: match[], and records, opened[] and plaintext slots of matched rows,
                            records of clear pubkeys */
  double match_ms;       /* key tables, ladders + SHA-512, HMAC-SHA256 and the gathers */
  double open_ms;        /* AES-256-CBC of the matched rows */
  double walk_ms;        /* the six phases of bmpow_rx_obj_stats, over matched rows and clear pubkeys */
  double hash_ms;
  double scalar_ms;
  double curve_ms;
  double ident_ms;
  double finish_ms;
  double host_ms;        /* wall time of the calls */
} bmpow_rx_sealed_obj_stats;

BMPOW_API int bmpow_rx_sealed_obj_get_stats(bmpow_rx_sealed_obj_stats *out);
BMPOW_API void bmpow_rx_sealed_obj_reset_stats(void);

#ifdef __cplusplus
}
#endif

#endif /* BMPOW_RXOBJOPEN_H */
