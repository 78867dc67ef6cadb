/*
 * bmpow_tx.h -- C ABI of libbmpow_hip.so's one-call assembly of outgoing signed objects (send side).
 *
 * The reference signs, encrypts and hashes every msg, broadcast and pubkey it sends one at a time
 * (src/class_singleWorker.py: sendMsg :1224-1276, sendBroadcast :641-681, sendOutOrStoreMyV4Pubkey
 * :420-465, sendOutOrStoreMyV3Pubkey :342-378).  Every one of them has one shape:
 *
 *     head  = pack('>Q', embeddedTime) || objectType(4) || varint(version) || varint(stream) [|| tag(32)]
 *     body  = what the signature covers behind the head
 *     sig   = DER( ECDSA( digest(head || body), signing key ) )
 *     tail  = varint(len(sig)) || sig                     (1 + len(sig) bytes; len(sig) <= 72)
 *     SEALED (msg, broadcast, v4 pubkey):  payload = head || ECIES(body || tail, recipient key)
 *     CLEAR  (v3 pubkey):                  payload = head || body || tail
 *     initialHash = SHA512(payload)                       (_doPOWDefaults; :1275)
 *
 * Here a batch goes from head and body bytes to the finished payload (without its nonce) and the
 * initialHash of its proof of work in one call.  The message bytes go up once; the padding of the signed
 * data, both digests, the signing equation, the DER encoding, the ECIES key agreement, AES-256-CBC,
 * HMAC-SHA256 and the SHA-512 of the payload all run on the device, and the signature never visits the
 * host between signing and encryption.  This call always seals on the device (BMPOW_SEAL is not read).
 *
 * Same conventions as bmpow_rx.h / bmpow_send.h (return codes, bmpow_last_error, thread safety); the
 * call runs on the first selected device in sets of at most 2^18 rows and 256 MB of pool, bmpow_abort()
 * is honoured between sets and before the ladder, and n == 0 succeeds with nothing launched.
 */
#ifndef BMPOW_TX_H
#define BMPOW_TX_H

#include "bmpow.h"
#include "bmpow_send.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BMPOW_TX_SEALED 0 /* payload = head || ECIES(body || tail) */
#define BMPOW_TX_CLEAR 1  /* payload = head || body || tail */

#define BMPOW_TX_OK 0
#define BMPOW_TX_BAD_RECIPIENT 1 /* a recipient coordinate >= p or off the curve: "encrypt didn't work", :1236 */
#define BMPOW_TX_NO_SIGNATURE 2  /* r or s came out zero (after the passes when the nonces are drawn) */
#define BMPOW_TX_TOO_LARGE 3     /* 8 + obj_len > 2^18: :1296, :681 */

#define BMPOW_TX_HEAD_MIN 12
#define BMPOW_TX_HEAD_MAX 62
#define BMPOW_TX_MAX_OBJECT (1u << 18) /* nonce included */

/* The bound on a payload of either kind: the tail is at most 73 bytes. */
#define BMPOW_TX_OBJ_CAP(head_len, body_len) ((size_t)(head_len) + BMPOW_ECIES_BLOB_CAP((size_t)(body_len) + 73))

/* One object.  sig and sig_len are filled unless status is BMPOW_TX_NO_SIGNATURE (and for a row that never
 * reached the device: a body above 2^18 bytes, a recipient coordinate >= p).  initial_hash and the payload
 * in outs[i] belong to BMPOW_TX_OK only; obj_len is 0 for BMPOW_TX_BAD_RECIPIENT and BMPOW_TX_NO_SIGNATURE,
 * and the exact length that was refused for BMPOW_TX_TOO_LARGE (0 where the body alone decided). */
typedef struct bmpow_tx_rec {
  int32_t status;    /* BMPOW_TX_* */
  uint32_t obj_len;  /* payload bytes, without the nonce */
  uint32_t plain_len; /* body_len + 1 + sig_len */
  uint8_t sig_len;
  uint8_t kind;   /* BMPOW_TX_SEALED / BMPOW_TX_CLEAR */
  uint8_t digest; /* BMPOW_SIG_SHA1 / BMPOW_SIG_SHA256 */
  uint8_t reserved;
  uint8_t sig[72];          /* the DER signature, zero padded */
  uint8_t initial_hash[64]; /* SHA512(payload) */
} bmpow_tx_rec; /* 152 bytes, no padding */

/* n rows of either kind.  heads[i] / head_lens[i]: 12 .. 62 bytes (anything else is BMPOW_E_ARG);
 * bodies[i] / body_lens[i]; privkeys: 32 big-endian bytes per row (0 or >= n, the group order, is
 * BMPOW_E_ARG); pubkeys: X || Y of the recipient, 64 bytes per row, ignored for BMPOW_TX_CLEAR (NULL when
 * no row is sealed); digest: BMPOW_SIG_SHA1 or BMPOW_SIG_SHA256.  nonces and ephem (32 bytes per row) and
 * ivs (16 bytes per row) may each be NULL: drawn from RAND_bytes, the scalars from [1, n - 1] by rejection;
 * a supplied scalar that is 0 or >= n is BMPOW_E_ARG.  With drawn nonces a row whose r or s is zero goes
 * through the whole chain again with a fresh nonce, at most three passes.  outs[i] / out_caps[i]: where the
 * payload goes; a cap below BMPOW_TX_OBJ_CAP(head_lens[i], body_lens[i]) is BMPOW_E_ARG, but for a body
 * above 2^18 bytes, which is BMPOW_TX_TOO_LARGE without going to the device (its outs[i] is never written). */
BMPOW_API int bmpow_tx_objects(size_t n, const uint8_t *kinds, const uint8_t *const *heads, const uint8_t *head_lens,
                               const uint8_t *const *bodies, const uint64_t *body_lens, const uint8_t *privkeys,
                               const uint8_t *pubkeys, int digest, const uint8_t *nonces, const uint8_t *ephem,
                               const uint8_t *ivs, uint8_t *const *outs, const uint64_t *out_caps, bmpow_tx_rec *out);

/* Where a row's pieces lie in its slot of the device pool, by the code the device uses. */
typedef struct bmpow_tx_layout {
  uint64_t slot_bytes;  /* the slot: a multiple of 16, bmseal::seal_slot_bytes(body_len + 73) */
  uint32_t body_at;     /* the body's first byte: SL_PLAIN_AT */
  uint32_t tail_at;     /* varint(len(sig)): body_at + body_len */
  uint32_t plain_cap;   /* body_len + 73: the most the tail kernel makes of the plaintext */
  uint32_t signed_len;  /* head_len + body_len */
  uint32_t hash_blocks; /* 64-byte blocks of the padded signed data */
  uint32_t reserved;
} bmpow_tx_layout;

/* Host only.  BMPOW_E_ARG for a head outside 12 .. 62 bytes or a body above 2^18. */
BMPOW_API int bmpow_tx_layout_row(uint32_t head_len, uint64_t body_len, bmpow_tx_layout *out);

/* Counters of bmpow_tx_objects since the last reset.  The times are GPU time between events recorded
 * around the launches of each phase. */
typedef struct bmpow_tx_stats {
  uint64_t calls;    /* calls that launched */
  uint64_t rows;     /* rows sent to the device (a redrawn signature counts again) */
  uint64_t sets;     /* sets of at most 2^18 rows and 256 MB of pool */
  uint64_t launches; /* kernel launches: six per set, eleven with sealed rows in it */
  double pack_ms;    /* head || body into padded SHA blocks */
  double hash_ms;    /* SHA-1 + SHA-256 of the signed data */
  double sign_ms;    /* k G by the comb, r, k^-1 and s mod n, DER and the tail */
  double ladder_ms;  /* the ephemeral key's comb and digits, recipient tables, r Q and its SHA-512 */
  double seal_ms;    /* AES-256-CBC and HMAC-SHA256 */
  double finish_ms;  /* SHA-512 of the payload and the record */
  double host_ms;    /* wall time of the calls: staging, upload, launches, download, scatter */
} bmpow_tx_stats;

BMPOW_API int bmpow_tx_get_stats(bmpow_tx_stats *out);
BMPOW_API void bmpow_tx_reset_stats(void);

#ifdef __cplusplus
}
#endif

#endif /* BMPOW_TX_H */
