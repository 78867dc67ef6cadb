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
#define BMPOW_RX_NOT_MINE 2            /* :478 -- no key decrypts; set by bmpow_rx_sealed_msgs (bmpow_rxopen.h) only */
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

/* ---------------------------------------------------------------------------------------------------
 * Broadcasts and pubkeys: processbroadcast (src/class_objectProcessor.py:756-926), processpubkey
 * (:276-408) and decryptAndCheckPubkeyPayload (src/protocol.py:412-518) from bytes to one record, in the
 * same single call and on the same kernels as the msgs above.  A row is one of three kinds:
 *
 *   kind        "plaintext"        signedData                                     expect (32-byte slot)
 *   BROADCAST   decrypted payload  obj[8:payload_off] || plain[:bottomOfMessage]  v4: the ripe of the
 *                                                                                 subscription key that
 *                                                                                 decrypted it; v5: unused
 *   PUBKEY_V4   decrypted payload  obj[8:payload_off] || plain[:endOfKeys]        the ripe of the address
 *   PUBKEY      the object itself  v3: obj[8:endOfSignedData]; v2: none           unused
 *
 * status is the first line that returns, in the reference's order.  For a broadcast the ripe (:882) or tag
 * (:893) comparison sits between the walk's checks: everything up to the two difficulty varints decides
 * first, then the comparison, then the encoding and the lengths, then the signature.  For an encrypted
 * pubkey the signature (:484) comes before the ripe (:497).
 * --------------------------------------------------------------------------------------------------- */
#define BMPOW_RXO_KIND_BROADCAST 0
#define BMPOW_RXO_KIND_PUBKEY_V4 1
#define BMPOW_RXO_KIND_PUBKEY 2

#define BMPOW_RXO_OK 0
#define BMPOW_RXO_VARINT 1            /* decodeVarint raises, in the object's header or in the plaintext */
#define BMPOW_RXO_BC_VERSION 2        /* :760 */
#define BMPOW_RXO_SENDER_VERSION 3    /* :830, :838 */
#define BMPOW_RXO_STREAM_MISMATCH 4   /* :848 */
#define BMPOW_RXO_WRONG_RIPE 5        /* :882; protocol.py:497 */
#define BMPOW_RXO_WRONG_TAG 6         /* :893 */
#define BMPOW_RXO_ENCODING_0 7        /* :901 */
#define BMPOW_RXO_BAD_SIGNATURE 8     /* :916; :374; protocol.py:484 */
#define BMPOW_RXO_ADDRESS_VERSION_0 9 /* :283 */
#define BMPOW_RXO_ADDRESS_VERSION 10  /* :287 */
#define BMPOW_RXO_NEEDS_DECRYPTION 11 /* a version 4 pubkey given as BMPOW_RXO_KIND_PUBKEY: it is not this kind */
#define BMPOW_RXO_TOO_SHORT 12        /* :293, :346 */
#define BMPOW_RXO_KEY_SHORT 13        /* :304 */
/* what decides before a plaintext exists; never set by this library (as BMPOW_RX_NOT_MINE) */
#define BMPOW_RXO_NOT_SUBSCRIBED 14   /* :801, :810 */
#define BMPOW_RXO_NOT_DECRYPTED 15    /* :820; protocol.py:457 */
#define BMPOW_RXO_NOT_NEEDED 16       /* :417; protocol.py:442 */
#define BMPOW_RXO_ADDRESS_MISMATCH 17 /* protocol.py:423, :428 */
#define BMPOW_RXO_V4_TOO_SHORT 18     /* :411 */

/* One object.  The walked fields are filled as far as the reference gets before it returns and zero behind
 * that; offsets into the plaintext (the object for BMPOW_RXO_KIND_PUBKEY) are those of the slices as Python
 * cuts them.  digest, ripe, sig_hash and addr are filled for BMPOW_RXO_OK only. */
typedef struct bmpow_rx_obj_rec {
  uint64_t object_version; /* broadcast version, or the address version of a pubkey object */
  uint64_t object_stream;  /* the stream number in the object's header */
  uint64_t sender_version; /* broadcast: sendersAddressVersion; pubkeys: the address version again */
  uint64_t sender_stream;  /* broadcast: sendersStream; pubkeys: the stream again */
  uint64_t ntpb;           /* the keys' nonceTrialsPerByte (version >= 3, else 0) */
  uint64_t extra;          /* the keys' payloadLengthExtraBytes (the same) */
  uint64_t encoding;       /* messageEncodingType (broadcasts) */
  uint32_t payload_off;    /* where the header (with the tag, if there is one) ends in the object */
  uint32_t tag_off;        /* where the tag starts in the object; payload_off for a v4 broadcast, 0 for PUBKEY */
  uint32_t end_of_pubkey;  /* broadcast: endOfPubkeyPosition; pubkeys: where storedData / signedData ends */
  uint32_t msg_off, msg_len;
  uint32_t sig_off, sig_len;
  uint32_t bottom;         /* source bytes the signature covers behind the prefix (from byte 8 for PUBKEY) */
  int32_t status;          /* BMPOW_RXO_* */
  uint8_t ripe[20];
  uint8_t sig_hash[32];    /* SHA512(SHA512(signature))[32:] (:922), broadcasts only */
  uint8_t addr_len;        /* characters in addr: 1 .. 58 */
  char addr[63];           /* the address after "BM-", zero padded, not terminated */
  uint8_t behaviour[4];
  uint8_t digest;          /* BMPOW_SIG_SHA1 / BMPOW_SIG_SHA256 where a signature verified, else 0 */
  uint8_t prefix_len;      /* bytes of signedData taken from the object's header: 0 .. 62 */
  uint8_t kind;            /* BMPOW_RXO_KIND_* */
  uint8_t keys_hashed;     /* both keys lie whole in the plaintext and everything in front of the ripe / tag
                              comparison got through: status is then what follows the comparison */
} bmpow_rx_obj_rec; /* 216 bytes, no padding */

/* n rows of any kinds.  objs[i] / obj_lens[i]: the whole object; plains[i] / plain_lens[i]: the decrypted
 * payload (ignored for BMPOW_RXO_KIND_PUBKEY); expect32: one 32-byte slot per row.  An object or a plaintext
 * above 2^31 bytes and an unknown kind are BMPOW_E_ARG. */
BMPOW_API int bmpow_rx_objects(size_t n, const uint8_t *kinds, const uint8_t *const *objs, const uint64_t *obj_lens,
                               const uint8_t *const *plains, const uint64_t *plain_lens, const uint8_t *expect32,
                               bmpow_rx_obj_rec *out);

/* Host only: the walk for one row, by the code the kernel is built from.  With plain == NULL for an
 * encrypted kind only the header is walked: status is the header's (BMPOW_RXO_OK so far) beside
 * object_version, object_stream, tag_off and payload_off.  Otherwise the record holds everything but what
 * the device computes, and a row with keys_hashed set still awaits its comparison.  Returns 1 where the row
 * would go to the curve kernels as it stands (canonical DER, 1 <= r, s < n, coordinates below p), else 0. */
BMPOW_API int bmpow_rx_walk_object(int kind, const uint8_t *obj, size_t obj_len, const uint8_t *plain,
                                   size_t plain_len, const uint8_t *expect32, bmpow_rx_obj_rec *rec);

/* Counters of bmpow_rx_objects, apart from bmpow_rx_stats (which stays "msgs only"); same fields. */
typedef bmpow_rx_stats bmpow_rx_obj_stats;
BMPOW_API int bmpow_rx_obj_get_stats(bmpow_rx_obj_stats *out);
BMPOW_API void bmpow_rx_obj_reset_stats(void);

#ifdef __cplusplus
}
#endif

#endif /* BMPOW_RX_H */
