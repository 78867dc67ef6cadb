/*
 * bmpow_inv.h -- C ABI of libbmpow_hip.so's device-resident inventory sets (receive side).
 *
 * The reference's network thread asks two sets the same question one hash at a time: what we have
 * (`inventoryHash in Inventory()`, BMObject.checkAlreadyHave and _command_inv, src/network/bmproto.py:344-367,
 * 393-435) and what has been announced to us and not yet fetched (`missingObjects`,
 * src/network/objectracker.py:88-99).  Here both are open-addressing tables of 32-byte keys on the device, and a
 * flood of `inv` / `dinv` / `getdata` packets (bmpow_inv_batch) or the intake's records (bmpow_inv_admit) are
 * judged against them in one call.  Only the membership is here: the objects' bytes, the SQL store and the
 * sockets stay with the caller.
 *
 * Same conventions as bmpow.h (return codes, bmpow_last_error, thread safety).  A set lives on the first selected
 * device and its calls run on that shard's stream, one at a time under the library's lock.  A set remembers the
 * device selection it was made under: after a re-selection or bmpow_shutdown every call on it but
 * bmpow_invset_destroy returns BMPOW_E_STATE.  The device calls return BMPOW_E_ABORTED while bmpow_abort()'s flag
 * is set.
 */
#ifndef BMPOW_INV_H
#define BMPOW_INV_H

#include "bmpow.h"
#include "bmpow_intake.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bmpow_invset bmpow_invset;

/* Per row of bmpow_invset_add (and state_out of bmpow_inv_admit). */
#define BMPOW_INV_ABSENT 0  /* the row took no part (bmpow_inv_admit: not in the store mask, or not looked up) */
#define BMPOW_INV_PRESENT 1 /* the key was in the set before the call */
#define BMPOW_INV_ADDED 2   /* the lowest row of this call that carries the key: its value is the one stored */
#define BMPOW_INV_DUP 3     /* a later row with the same key; first_out names the ADDED one */

/* The packet kinds of bmpow_inv_walk / bmpow_inv_batch. */
#define BMPOW_INV_KIND_INV 0
#define BMPOW_INV_KIND_DINV 1
#define BMPOW_INV_KIND_GETDATA 2

/* bmpow_inv_pkt.status */
#define BMPOW_INV_OK 0
#define BMPOW_INV_MALFORMED 1 /* varintDecodeError: the count does not decode */
#define BMPOW_INV_TOO_MANY 2  /* BMProtoExcessiveDataError: an inv / dinv above MAX_OBJECT_COUNT; no item is processed */
#define BMPOW_INV_IGNORED 3   /* a dinv while dandelion is off */

#define BMPOW_INV_MAX_OBJECT_COUNT 50000 /* network/constants.py MAX_OBJECT_COUNT */

/* Per item of bmpow_inv_batch. */
#define BMPOW_INV_ITEM_NOT_HAVE 0  /* getdata only: not in `have` */
#define BMPOW_INV_ITEM_HAVE 1      /* in `have` (inv / dinv: the reference skips it unless Dandelion().hasHash(i)) */
#define BMPOW_INV_ITEM_KNOWN 2     /* already in `missing` */
#define BMPOW_INV_ITEM_NEW 3       /* added to `missing` */
#define BMPOW_INV_ITEM_NEW_AGAIN 4 /* announced earlier in this call; item_first = that item */
#define BMPOW_INV_ITEM_SHORT 5     /* fewer than 32 bytes: never uploaded or stored; the caller's */

typedef struct bmpow_inv_value {
  uint64_t expires;
  uint32_t stream;
  uint32_t aux; /* the caller's (an index into its own store, say) */
} bmpow_inv_value;

/* One packet as decode_payload_content("l32s") (bmproto.py:190-315) reads it. */
typedef struct bmpow_inv_pkt {
  uint64_t count;       /* len(items) as the reference sees it: max(the varint, 1), whatever the payload holds */
  uint32_t first_item;  /* index of the packet's first item in the item arrays (bmpow_inv_batch; 0 from the walk) */
  uint32_t n_items;     /* items in the item arrays: 0 unless OK; else the full ones, the short one, and of the empty
                           ones behind the payload's end the first */
  uint32_t item_offset; /* payload offset of item 0 (the varint's length) */
  int32_t status;       /* BMPOW_INV_OK .. IGNORED */
} bmpow_inv_pkt;

/* Counters of one set since it was made or cleared. */
typedef struct bmpow_inv_stats {
  uint64_t slots;      /* the table's slot count now */
  uint64_t seed;
  uint64_t live;       /* keys held */
  uint64_t tombstones; /* removed entries not yet purged */
  uint64_t calls;
  uint64_t rows;       /* rows looked up, added or removed */
  uint64_t launches;
  uint64_t rebuilds;   /* grow, purge and sweep */
  uint64_t probes;     /* slots looked at, all rows */
  uint64_t longest_probe;
  double lookup_ms;    /* GPU time between events, per kernel */
  double claim_ms;
  double finalize_ms;
  double bury_ms;
  double rebuild_ms;
  double list_ms;
  double host_ms;      /* the calls' wall time */
} bmpow_inv_stats;

/* A set of at least slots_hint slots (a power of two, 8 at least), growing as it fills: live + tombstones +
 * a call's rows stay at or below half the slots, by a rebuild into a larger table before the call where needed.
 * seed picks the start slots (0 = drawn at random).  NULL on failure. */
BMPOW_API bmpow_invset *bmpow_invset_create(uint64_t slots_hint, uint64_t seed);
/* Frees on the set's own device; the one call that works after a re-selection.  NULL is ignored. */
BMPOW_API void bmpow_invset_destroy(bmpow_invset *set);
BMPOW_API int bmpow_invset_clear(bmpow_invset *set);
BMPOW_API int64_t bmpow_invset_len(bmpow_invset *set);
BMPOW_API int bmpow_invset_stats(bmpow_invset *set, bmpow_inv_stats *out);

/* keys[32 i ..] with value (expires[i], stream[i], aux[i]); each of the three may be NULL for zeros.  Per row
 * state_out[i] = PRESENT, ADDED or DUP and first_out[i] = the lowest row of the call carrying the same key (i
 * itself unless DUP): the answers of a sequential insert in row order, whatever order the device worked in. */
BMPOW_API int bmpow_invset_add(bmpow_invset *set, size_t n, const uint8_t *keys, const uint64_t *expires,
                               const uint32_t *stream, const uint32_t *aux, uint8_t *state_out, uint32_t *first_out);
/* present_out[i] = 1 where keys[32 i ..] is in the set; value_out (may be NULL) its value, zeros where absent. */
BMPOW_API int bmpow_invset_contains(bmpow_invset *set, size_t n, const uint8_t *keys, uint8_t *present_out,
                                    bmpow_inv_value *value_out);
/* Removes the keys; present_out[i] (may be NULL) = 1 where the key was in the set (equal rows all say 1). */
BMPOW_API int bmpow_invset_remove(bmpow_invset *set, size_t n, const uint8_t *keys, uint8_t *present_out);
/* Inventory.clean (src/storage/sqlite.py:115-120): drops every entry with expires < min_expires and every
 * tombstone by a rebuild; returns what is left. */
BMPOW_API int64_t bmpow_invset_sweep(bmpow_invset *set, uint64_t min_expires);
/* unexpired_hashes_by_stream (sqlite.py:92-101): the keys with this stream and expires > now, out[32 j ..] in no
 * particular order.  Returns their count, which may exceed cap: then only cap of them were written. */
BMPOW_API int64_t bmpow_invset_list(bmpow_invset *set, uint32_t stream, uint64_t now, uint8_t *out, size_t cap);

/* Host only.  The slot a key's probe starts from in a table of 2^log2_slots slots under seed (1 <= log2_slots <=
 * 30; else 0).  A full slot's tag is mixed from the key's first 16 bytes only: keys that differ behind them have
 * equal tags, and the resident key tells them apart. */
BMPOW_API uint64_t bmpow_invset_slot(uint64_t seed, uint32_t log2_slots, const uint8_t key[32]);

/* Host only.  One payload of kind BMPOW_INV_KIND_* as the reference's handler reads it: out->count, item_offset,
 * n_items and status (first_item 0).  A count of 0 and an empty payload each yield one item, a payload that ends
 * early one short item and then empty ones, and bytes behind the last item are not looked at -- the parser's own
 * behaviour.  MAX_OBJECT_COUNT and the dandelion switch bind inv / dinv only. */
BMPOW_API int bmpow_inv_walk(const uint8_t *payload, uint64_t len, int kind, int dandelion_on, bmpow_inv_pkt *out);

/* _command_inv / bm_command_getdata's membership work for n_pkt packets: one upload of the payloads as they are,
 * a lookup in `have`, then for the inv / dinv items we do not have an add into `missing` with expires = now
 * (missingObjects[hashId] = time.time()).  pkt_recs[p] as bmpow_inv_walk fills it, first_item set; the items of
 * all packets in packet order, then item order: item_state[j] = BMPOW_INV_ITEM_*, item_first[j] = for NEW_AGAIN
 * the index of the first item of this call with the same hash, else j.  getdata items are HAVE or NOT_HAVE
 * (skipUntil is the caller's).  The Dandelion exception of bmproto.py:361 is the caller's: it knows its few stem
 * hashes, and HAVE tells it where to ask.  `missing` may be NULL when every packet is a getdata.  Returns the
 * item count; BMPOW_E_ARG when it exceeds cap (size the arrays with bmpow_inv_walk). */
BMPOW_API int64_t bmpow_inv_batch(bmpow_invset *have, bmpow_invset *missing, size_t n_pkt, const uint8_t *const *payloads,
                                  const uint64_t *lens, const uint8_t *kinds, uint64_t now, int dandelion_on,
                                  bmpow_inv_pkt *pkt_recs, uint8_t *item_state, uint32_t *item_first, size_t cap);

/* store_mask of bmpow_inv_admit */
#define BMPOW_INV_ADMIT_LOOKUP 0 /* look the row up, store nothing */
#define BMPOW_INV_ADMIT_STORE 1  /* and store it where we do not have it */
#define BMPOW_INV_ADMIT_SKIP 2   /* no object at all (a packet of another command, its record zeroed): no part */

/* The step behind bmpow_intake_batch / bmpow_packets_batch, for n intake records (stride bytes apart; 0 =
 * sizeof(bmpow_intake_rec)).  A record whose status lets the reference reach checkAlreadyHave (OK,
 * INVALID_STREAM, UNWANTED_STREAM, INVALID_FOR_TYPE: bmproto.py:393-419) is looked up in `have`
 * (already_out[i] = 1 where found) unless store_mask[i] is SKIP.  Of those, the rows with store_mask[i] ==
 * STORE that we do not have are added
 * to `have` with the record's expires and stream (above 2^32 - 1: that) and aux = i; state_out[i] as
 * bmpow_invset_add's, ABSENT for the others.  Every looked-up row's hash leaves `missing`
 * (stopDownloadingObject and `del missingObjects[...]`, :399-424, :646-662).  missing may be NULL. */
BMPOW_API int bmpow_inv_admit(bmpow_invset *have, bmpow_invset *missing, size_t n, const void *intake_recs, size_t stride,
                              const uint8_t *store_mask, uint8_t *already_out, uint8_t *state_out);

#ifdef __cplusplus
}
#endif

#endif /* BMPOW_INV_H */
