/*
 * bmpow_proc.h -- C ABI of libbmpow_hip.so's object-processor dispatch (receive side).
 *
 * The reference's objectProcessor thread takes one (objectType, data) pair at a time off its queue
 * (objectProcessor.run, src/class_objectProcessor.py:64-110).  For every object it runs checkackdata (:129-154): is
 * data[16:] a key of state.ackdataForWhichImWatching?  Then it routes by type (:72-95): processgetpubkey
 * (:176-268), processonion (:156-174, with protocol.checkIPAddress, src/protocol.py:150-227), or one of the
 * handlers that the library already has as batch calls (bmpow_rx_sealed_msgs, bmpow_rx_sealed_objects).  Here a
 * dispatcher object holds the watched ack data and my addresses, and bmpow_proc_batch judges a whole queue in one
 * call: one record per object with the route, the ack verdict, and the getpubkey or onionpeer verdict.  The SQL
 * update, the UI signal, knownnodes, the worker queue and the host string stay with the caller.
 *
 * Same conventions as bmpow.h (return codes, bmpow_last_error, thread safety) and as bmpow_invset: a dispatcher
 * lives on the first selected device, its calls run on that shard's stream one at a time under the library's
 * lock, after a re-selection or bmpow_shutdown every call on it but bmpow_proc_destroy returns BMPOW_E_STATE, and
 * bmpow_proc_batch returns BMPOW_E_ABORTED while bmpow_abort()'s flag is set.
 */
#ifndef BMPOW_PROC_H
#define BMPOW_PROC_H

#include "bmpow.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bmpow_proc bmpow_proc;

/* bmpow_proc_rec.route: the branch of objectProcessor.run (:72-95) */
#define BMPOW_PROC_ROUTE_GETPUBKEY 0
#define BMPOW_PROC_ROUTE_PUBKEY 1
#define BMPOW_PROC_ROUTE_MSG 2
#define BMPOW_PROC_ROUTE_BROADCAST 3
#define BMPOW_PROC_ROUTE_ONIONPEER 4    /* objectType 0x746f72 */
#define BMPOW_PROC_ROUTE_UNKNOWN_TYPE 5 /* "Don't know how to handle object type" */

/* bmpow_proc_rec.ack: checkackdata (:129-154) */
#define BMPOW_PROC_ACK_NOT_CHECKED 0   /* len(data) < 32 */
#define BMPOW_PROC_ACK_NOT_WATCHED 1   /* data[16:] is no watched key */
#define BMPOW_PROC_ACK_FOUND 2         /* the lowest row of the call that carries this watched key; ack_aux = its aux */
#define BMPOW_PROC_ACK_FOUND_EARLIER 3 /* a later row with the same tail: the reference has deleted the key by then
                                          and says "not ... bound for me"; ack_first = the FOUND row */

/* bmpow_proc_rec.status.  0 for the routes that have no verdict here. */
#define BMPOW_PROC_NONE 0
/* processgetpubkey: the first refusal in the reference's order ... */
#define BMPOW_PROC_TOO_LONG 1          /* len(data) > 200, judged before any varint */
#define BMPOW_PROC_MALFORMED 2         /* varintDecodeError (getpubkey: either varint; onionpeer: any of three) */
#define BMPOW_PROC_VERSION_ZERO 3
#define BMPOW_PROC_VERSION_ONE 4
#define BMPOW_PROC_VERSION_TOO_HIGH 5
#define BMPOW_PROC_SHORT_HASH 6        /* the object ends inside the 20 bytes */
#define BMPOW_PROC_SHORT_TAG 7         /* the object ends inside the 32 bytes */
#define BMPOW_PROC_NOT_MINE 8
#define BMPOW_PROC_VERSION_MISMATCH 9
#define BMPOW_PROC_STREAM_MISMATCH 10
#define BMPOW_PROC_CHAN 11
#define BMPOW_PROC_SENT_RECENTLY 12    /* last_pubkey_send_time > now - 2419200 */
/* ... or the worker command */
#define BMPOW_PROC_SEND_V2 13          /* ('doPOWForMyV2Pubkey', hash) */
#define BMPOW_PROC_SEND_V3 14          /* ('sendOutOrStoreMyV3Pubkey', hash) */
#define BMPOW_PROC_SEND_V4 15          /* ('sendOutOrStoreMyV4Pubkey', address) */
/* processonion */
#define BMPOW_PROC_NO_HOST 16          /* checkIPAddress gives False */
#define BMPOW_PROC_RAISES 17           /* an IPv4-mapped prefix before other than 4 bytes: ValueError out of
                                          socket.inet_ntop escapes to the run loop's `except Exception` */
#define BMPOW_PROC_PEER 18             /* knownnodes.addKnownNode(stream, Peer(host, port)) */

/* bmpow_proc_rec.host_class */
#define BMPOW_PROC_HOST_NONE 0
#define BMPOW_PROC_HOST_V4 1    /* the 4 bytes at host_off + 12 */
#define BMPOW_PROC_HOST_ONION 2 /* base32 of the bytes at host_off + 6, whatever their count */
#define BMPOW_PROC_HOST_V6 3    /* the 16 bytes at host_off */

#define BMPOW_PROC_NO_ROW 0xffffffffu /* address / ack_first where there is none */

typedef struct bmpow_proc_rec {
  uint64_t version;    /* getpubkey: requestedAddressVersionNumber (0 where it was not reached) */
  uint64_t stream;     /* getpubkey: streamNumber; onionpeer: stream */
  uint64_t port;       /* onionpeer: the full varint */
  uint32_t route;      /* BMPOW_PROC_ROUTE_* */
  uint32_t ack;        /* BMPOW_PROC_ACK_* */
  uint32_t ack_aux;    /* FOUND and FOUND_EARLIER: the watched key's aux */
  uint32_t ack_first;  /* FOUND: the row itself; FOUND_EARLIER: the FOUND row; else NO_ROW */
  uint32_t status;     /* BMPOW_PROC_NONE .. PEER */
  uint32_t key_off;    /* getpubkey that reached the slice: offset of the requested hash or tag */
  uint32_t key_len;    /* the bytes of the slice that lie inside the object (20 or 32 unless SHORT_*) */
  uint32_t address;    /* the row of the address table that was found, else NO_ROW */
  uint32_t host_off;   /* PEER: the host is data[host_off : host_off + host_len] */
  uint32_t host_len;
  uint32_t host_class; /* BMPOW_PROC_HOST_* */
  uint32_t reserved;
} bmpow_proc_rec;

/* One row of shared.myAddressesByHash / myAddressesByTag (shared.reloadMyAddressHashes, src/shared.py:124-138):
 * every row is found by its ripe and by its tag, whatever its version. */
typedef struct bmpow_proc_address {
  uint8_t ripe[20];
  uint8_t tag[32];  /* SHA512(SHA512(varint(version) || varint(stream) || ripe))[32:] */
  uint32_t version; /* decodeAddress(address)[1] */
  uint64_t stream;  /* decodeAddress(address)[2] */
  int64_t last_pubkey_send_time; /* config.safeGetInt(address, 'lastpubkeysendtime') */
  uint32_t chan;    /* config.safeGetBoolean(address, 'chan') */
  uint32_t reserved;
} bmpow_proc_address;

typedef struct bmpow_proc_params {
  int64_t now;              /* stands for time.time(); 0 = the clock */
  uint32_t rows_per_launch; /* 0 = the default; tests force small values */
  uint32_t reserved;
} bmpow_proc_params;

typedef struct bmpow_proc_stats {
  uint64_t seed;
  uint64_t watch_len;      /* watched keys now */
  uint64_t watch_slots;    /* slots of the index the last upload would build */
  uint64_t watch_lengths;  /* distinct key lengths now */
  uint64_t addresses;
  uint64_t calls;          /* bmpow_proc_batch calls */
  uint64_t rows;           /* objects judged */
  uint64_t rows_uploaded;  /* device rows: ack candidates + getpubkeys + onionpeers */
  uint64_t ack_rows;       /* of those, ack candidates */
  uint64_t bytes_uploaded; /* object bytes */
  uint64_t table_uploads;  /* uploads of the watch set or the address table */
  uint64_t launches;
  uint64_t found;          /* keys that left the watch set through a batch */
  double rows_ms;          /* GPU time between events, per kernel */
  double finish_ms;
  double host_ms;          /* the batch calls' wall time */
} bmpow_proc_stats;

/* seed picks the watch index's start slots (0 = drawn at random).  host_only != 0: no device is touched and
 * none is needed; every call works but bmpow_proc_batch, which returns BMPOW_E_STATE.  NULL on failure. */
BMPOW_API bmpow_proc *bmpow_proc_create(uint64_t seed, int host_only);
/* The one call that works after a re-selection.  NULL is ignored. */
BMPOW_API void bmpow_proc_destroy(bmpow_proc *d);
BMPOW_API int bmpow_proc_stats_get(bmpow_proc *d, bmpow_proc_stats *out);
BMPOW_API int bmpow_proc_stats_reset(bmpow_proc *d);

/* state.ackdataForWhichImWatching: byte strings of any length, each with an aux of the caller's.  The
 * authoritative copy is on the host; a batch uploads it as a whole where it changed since the last one. */
/* n keys, key i = keys[offs[i] .. offs[i + 1]) (offs has n + 1 entries); aux may be NULL for zeros.  A key already
 * watched takes the new aux (ackdataForWhichImWatching[ackdata] = 0 twice).  added_out[i] (may be NULL) = 1 where
 * the key is new. */
BMPOW_API int bmpow_proc_watch_add(bmpow_proc *d, size_t n, const uint8_t *keys, const uint64_t *offs,
                                   const uint32_t *aux, uint8_t *added_out);
/* Removes the keys; present_out[i] (may be NULL) = 1 where the key was watched. */
BMPOW_API int bmpow_proc_watch_discard(bmpow_proc *d, size_t n, const uint8_t *keys, const uint64_t *offs,
                                       uint8_t *present_out);
/* present_out[i] = 1 where the key is watched; aux_out (may be NULL) its aux, 0 where absent. */
BMPOW_API int bmpow_proc_watch_contains(bmpow_proc *d, size_t n, const uint8_t *keys, const uint64_t *offs,
                                        uint8_t *present_out, uint32_t *aux_out);
BMPOW_API int64_t bmpow_proc_watch_len(bmpow_proc *d);
BMPOW_API int bmpow_proc_watch_clear(bmpow_proc *d);
/* Host only.  The slot a key's probe starts from in an index of 2^log2_slots slots under seed (3 <= log2_slots <=
 * 31; else 0).  The index of n keys has max(8, the power of two >= 2 n) slots.  Slot and tag are mixed from the
 * seed, the key's length and its first 16 bytes only: keys equal in those share both, and the resident key's
 * bytes tell them apart. */
BMPOW_API uint64_t bmpow_proc_watch_slot(uint64_t seed, uint32_t log2_slots, const uint8_t *key, size_t len);

/* The whole table at once.  Rows with an equal ripe or an equal tag, a chan above 1: BMPOW_E_ARG, and the table
 * stays as it was. */
BMPOW_API int bmpow_proc_set_addresses(bmpow_proc *d, size_t n, const bmpow_proc_address *rows);

/* n objects as the queue holds them: types[i] is objectType (from the intake's record; never re-read from the
 * bytes), objs[i] / lens[i] the data.  recs_out[i] as described above.  The ack verdicts are those of a sequential
 * run in row order, whatever order the device worked in and however the rows were cut into launches; after the
 * call the FOUND keys have left the watch set.  Two accepted getpubkeys for one address both say SEND_*: the
 * reference's worker updates lastpubkeysendtime only later.  Uploaded are the tail of an object whose len - 16
 * is some watched key's length, a getpubkey of 200 bytes or less, and the first 64 bytes of an onionpeer; every
 * other record is final on the host. */
BMPOW_API int bmpow_proc_batch(bmpow_proc *d, size_t n, const uint8_t *const *objs, const uint64_t *lens,
                               const uint32_t *types, const bmpow_proc_params *params, bmpow_proc_rec *recs_out);

/* Host only, no device.  One object's record without the ack fields (ack = NOT_CHECKED), from the functions the
 * kernel runs.  now = 0: the clock. */
BMPOW_API int bmpow_proc_walk(uint32_t type, const uint8_t *obj, uint64_t len, size_t n_addresses,
                              const bmpow_proc_address *addresses, int64_t now, bmpow_proc_rec *rec_out);

#ifdef __cplusplus
}
#endif

#endif /* BMPOW_PROC_H */
