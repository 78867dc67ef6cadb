/*
 * bmpow_intake.h -- C ABI of libbmpow_hip.so's batched object intake (receive side).
 *
 * The reference's network thread does four things for every received object
 * (src/network/bmproto.py:377-441, src/network/bmobject.py:43-163): it decodes the header "QQIvv",
 * computes inventoryHash = SHA512(SHA512(object))[:32] (src/addresses.py:137-143), checks the proof of
 * work (src/protocol.py:258-286) and runs the end-of-life, stream and per-type sanity checks.  Here a
 * whole flood goes through that in one call: one upload of the padded payload pool, one launch per
 * shard computing both hash chains per object, and the header walk and checks on host threads.
 *
 * Same conventions as bmpow.h (return codes, bmpow_last_error, thread safety).  The batch calls are
 * sharded over every selected shard, as bmpow_verify_batch is, and like it return BMPOW_E_ABORTED
 * while bmpow_abort()'s flag is set.
 */
#ifndef BMPOW_INTAKE_H
#define BMPOW_INTAKE_H

#include "bmpow.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The first check of bm_command_object that fails, in the reference's order; each code names the
 * exception the reference raises there. */
#define BMPOW_INTAKE_OK 0
#define BMPOW_INTAKE_MALFORMED 1        /* struct.error / varintDecodeError: the header does not decode */
#define BMPOW_INTAKE_TOO_LARGE 2        /* BMProtoExcessiveDataError: > 2^18 bytes after the header */
#define BMPOW_INTAKE_INSUFFICIENT_POW 3 /* BMObjectInsufficientPOWError */
#define BMPOW_INTAKE_EXPIRED_FUTURE 4   /* BMObjectExpiredError: more than 28 d 3 h ahead */
#define BMPOW_INTAKE_EXPIRED_PAST 5     /* BMObjectExpiredError: more than 1 h ago */
#define BMPOW_INTAKE_INVALID_STREAM 6   /* BMObjectInvalidError (checkStream): 0 or above 2^63 - 1 */
#define BMPOW_INTAKE_UNWANTED_STREAM 7  /* BMObjectUnwantedStreamError */
#define BMPOW_INTAKE_INVALID_FOR_TYPE 8 /* BMObjectInvalidError (checkObjectByType) */

#define BMPOW_INTAKE_MAX_PAYLOAD (1u << 18) /* network/constants.py MAX_OBJECT_PAYLOAD_SIZE */
#define BMPOW_INTAKE_MAX_TTL 2430000        /* BMObject.maxTTL: 28 * 24 * 3600 + 10800 */
#define BMPOW_INTAKE_MIN_TTL (-3600)        /* BMObject.minTTL */

typedef struct bmpow_intake_rec {
  uint64_t nonce;          /* object[0:8] */
  uint64_t expires;        /* expiresTime, object[8:16] */
  uint64_t version;        /* first varint */
  uint64_t stream;         /* second varint */
  uint64_t pow;            /* the receive-side POW value (bmpow_intake_batch) */
  uint32_t object_type;    /* object[16:20] */
  uint32_t payload_offset; /* first byte after the header */
  int32_t status;          /* BMPOW_INTAKE_* (bmpow_intake_batch) */
  uint32_t reserved;
  uint8_t inv[32];         /* inventoryHash; zeros for MALFORMED and TOO_LARGE (bmpow_intake_batch) */
} bmpow_intake_rec;

typedef struct bmpow_intake_params {
  int64_t now;             /* int(time.time()) of the EOL check; 0 = the clock */
  int64_t recv_time;       /* isProofOfWorkSufficient's recvTime; 0 = now */
  uint64_t ntpb;           /* nonceTrialsPerByte (0 = the network minimum) */
  uint64_t extra;          /* payloadLengthExtraBytes (0 = the network minimum) */
  const uint64_t *streams; /* state.streamsInWhichIAmParticipating */
  size_t n_streams;
} bmpow_intake_params;

/* inv_out[32 i ..] = SHA512(SHA512(objs[i]))[:32] for n objects of lens[i] >= 8 bytes each (a shorter
 * one, or one the payload pool does not accept, is BMPOW_E_ARG). */
BMPOW_API int bmpow_inventory_hashes(size_t n, const uint8_t *const *objs, const uint64_t *lens, uint8_t *inv_out);

/* Host only.  Decode ">QQI" and two varints by addresses.decodeVarint's rules (a non-minimal or
 * truncated encoding is an error; a varint at the very end of the object decodes as (0, 0), as there).
 * Fills nonce, expires, object_type, version, stream and payload_offset, zeroes the rest, and returns
 * 1; returns 0 (out zeroed) when the header does not decode inside the object. */
BMPOW_API int bmpow_intake_header(const uint8_t *obj, size_t len, bmpow_intake_rec *out);

/* Host only.  The reference's checks over a decoded header, in its order (bmproto.py:386-419,
 * bmobject.py:71-163), the first that fails: TOO_LARGE, INSUFFICIENT_POW (pow_ok == 0), EXPIRED_FUTURE,
 * EXPIRED_PAST (against now), INVALID_STREAM, UNWANTED_STREAM (stream not among streams[0 ..
 * n_streams)), INVALID_FOR_TYPE (getpubkey < 42 bytes, pubkey < 146 or > 440 bytes, broadcast < 180
 * bytes or version < 2; len counts the whole object).  MALFORMED for a record the header walk did not
 * fill.  The already-have lookup, between the EOL and stream checks in the reference, is the caller's. */
BMPOW_API int bmpow_intake_status(const bmpow_intake_rec *rec, size_t len, int pow_ok, int64_t now,
                                  const uint64_t *streams, size_t n_streams);

/* bm_command_object's per-object work for n objects: out[i] = header fields, inventoryHash, POW value
 * and status of objs[i].  MALFORMED and TOO_LARGE objects are not uploaded (inv and pow stay zero). */
BMPOW_API int bmpow_intake_batch(size_t n, const uint8_t *const *objs, const uint64_t *lens,
                                 const bmpow_intake_params *params, bmpow_intake_rec *out);

/* Counters of the intake calls since the last reset. */
typedef struct bmpow_intake_stats {
  uint64_t calls;        /* bmpow_inventory_hashes / bmpow_intake_batch calls that launched */
  uint64_t objects;      /* objects uploaded */
  uint64_t blocks;       /* 128-byte pool blocks uploaded */
  uint64_t launches;     /* kernel launches (one per shard part) */
  double kernel_ms;      /* GPU time between events around the launches (the slowest shard of each call) */
  double host_build_ms;  /* plan, padding and upload */
  double host_run_ms;    /* launch, wait and the results' way back */
  double host_status_ms; /* header walk and checks */
} bmpow_intake_stats;

BMPOW_API int bmpow_intake_get_stats(bmpow_intake_stats *out);
BMPOW_API void bmpow_intake_reset_stats(void);

#ifdef __cplusplus
}
#endif

#endif /* BMPOW_INTAKE_H */
