/*
 * bmpow_rx.h -- C ABI of libbmpow_hip.so's batched processing of decrypted msgs (receive side).
 *
 * Once a msg object has decrypted, the reference's processmsg (src/class_objectProcessor.py:435-747)
 * walks the plaintext's fields (:488-561), composes
 *     signedData = data[8:20] || varint(1) || varint(stream of the object) || plaintext[:bottomOfAckData]
 * checks the signature over it (:566), and hashes the sender's keys into the ripe and the address
 * (:586-591) and the signature into sigHash (:583).  Here a batch goes from the plaintext bytes to one
 * record per msg in one call: the field walk, the DER parse of the signature, the composition and SHA
 * padding of signedData, both digests, the ECDSA equation, the ripe and the address all run on the device.
 *
 * All positions follow the reference's Python semantics: a slice past the end is empty, decodeVarint of
 * nothing is (0, 0), a length varint may be any value up to 2^64 - 1 (positions saturate, never wrap),
 * and a varint that is truncated or not minimal is the reference's exception (BMPOW_RX_VARINT).
 *
 * Same conventions as bmpow.h (return codes, bmpow_last_error, thread safety); the call runs on the first
 * selected device in sets of at most 2^18 rows and 256 MB of padded signed data, bmpow_abort() is
 * honoured between sets, and n == 0 succeeds with nothing launched.
 */
#ifndef BMPOW_RX_H
#define BMPOW_RX_H

#include "bmpow.h"

#ifdef __cplusplus
extern "C" {
#endif

/* status: the first line of processmsg that returns */
#define BMPOW_RX_OK 0                  /* reaches :582 */
#define BMPOW_RX_MSG_VERSION 1         /* :444, also a header varint that does not decode */
#define BMPOW_RX_NOT_MINE 2            /* :478 -- no key decrypts; never set by this library */
#define BMPOW_RX_SENDER_VERSION_0 3    /* :492 */
#define BMPOW_RX_SENDER_VERSION_HIGH 4 /* :496 */
#define BMPOW_RX_TOO_SHORT 5           /* :500 */
#define BMPOW_RX_SENDER_STREAM_0 6     /* :506 */
#define BMPOW_RX_WRONG_TO_RIPE 7       /* :531 */
#define BMPOW_RX_VARINT 8              /* decodeVarint raises, at whichever position of the plaintext */
#define BMPOW_RX_BAD_SIGNATURE 9       /* :566 */

/* One msg.  The walked fields are filled as far as the walk got and zero behind it.  Offsets and lengths
 * are those of the slices as Python cuts them: clipped to the plaintext, so off + len <= its length.
 * ripe, sig_hash and addr are filled for BMPOW_RX_OK only. */
typedef struct bmpow_rx_msg_rec {
  uint64_t sender_version;
  uint64_t sender_stream;
  uint64_t ntpb;           /* requiredAverageProofOfWorkNonceTrialsPerByte (sender version >= 3, else 0) */
  uint64_t extra;          /* requiredPayloadLengthExtraBytes (the same) */
  uint64_t encoding;       /* messageEncodingType */
  uint64_t claimed_stream; /* streamNumberAsClaimedByMsg (:450) */
  uint32_t end_of_pubkey;  /* endOfThePublicKeyPosition (:530) */
  uint32_t msg_off, msg_len;
  uint32_t ack_off, ack_len;
  uint32_t sig_off, sig_len;
  uint32_t bottom;         /* plaintext bytes the signature covers: positionOfBottomOfAckData, clipped */
  int32_t status;          /* BMPOW_RX_* */
  uint8_t ripe[20];        /* the sender's ripe (:589) */
  uint8_t sig_hash[32];    /* SHA512(SHA512(signature))[32:] (:583) */
  uint8_t addr_len;        /* characters in addr: 1 .. 58 */
  char addr[63];           /* fromAddress after "BM-", zero padded, not terminated */
  uint8_t behaviour[4];    /* the bitfield behind the sender's stream number */
  uint8_t digest;          /* BMPOW_SIG_SHA1 / BMPOW_SIG_SHA256 for BMPOW_RX_OK, else 0 */
  uint8_t prefix_len;      /* bytes of signedData in front of the plaintext: 14, 16, 18 or 22 */
  uint8_t reserved[2];
} bmpow_rx_msg_rec; /* 208 bytes, no padding */

/* processmsg from :441 to :591 for n decrypted msgs.  objs[i] / obj_lens[i]: the whole object (only its
 * first 38 bytes are read: data[8:20] and the two varints of :441-452); plains[i] / plain_lens[i]: what
 * the key of ripe to_ripes20[20 i ..] decrypted it to.  A plaintext above 2^31 bytes is BMPOW_E_ARG. */
BMPOW_API int bmpow_rx_msgs(size_t n, const uint8_t *const *objs, const uint64_t *obj_lens,
                            const uint8_t *const *plains, const uint64_t *plain_lens, const uint8_t *to_ripes20,
                            bmpow_rx_msg_rec *out);

/* Host only: the same walk for one msg, by the code the kernel is built from.  Fills everything but what
 * the device computes: a walk that gets through leaves status BMPOW_RX_OK, digest 0 and ripe, sig_hash
 * and addr zero.  Returns 1 when the signature is canonical DER with 1 <= r, s < n and both coordinates
 * of the signing key are below p (the row the device verifies as it stands), 0 when the walk or those
 * checks refuse it. */
BMPOW_API int bmpow_rx_walk_msg(const uint8_t *obj, size_t obj_len, const uint8_t *plain, size_t plain_len,
                                const uint8_t *to_ripe20, bmpow_rx_msg_rec *rec);

/* Counters of bmpow_rx_msgs since the last reset.  The times are GPU time between events recorded
 * around the launches of each phase. */
typedef struct bmpow_rx_stats {
  uint64_t calls;    /* calls that launched */
  uint64_t rows;     /* msgs they were given */
  uint64_t sets;     /* sets of at most 2^18 rows and 256 MB of pool */
  uint64_t launches; /* kernel launches: nine per set */
  double walk_ms;    /* field walk and packing of signedData */
  double hash_ms;    /* SHA-1 + SHA-256 of signedData */
  double scalar_ms;  /* s^-1, u1, u2 mod n and u2's digits */
  double curve_ms;   /* key tables, ladder, combs and the final test */
  double ident_ms;   /* ripe and address */
  double finish_ms;  /* sigHash and the final record */
  double host_ms;    /* wall time of the calls: staging, upload, launches, download */
} bmpow_rx_stats;

BMPOW_API int bmpow_rx_get_stats(bmpow_rx_stats *out);
BMPOW_API void bmpow_rx_reset_stats(void);

#ifdef __cplusplus
}
#endif

#endif /* BMPOW_RX_H */
