/*
 * bmpow_packets.h -- C ABI of libbmpow_hip.so's packet framing (receive side, in front of the intake).
 *
 * The reference's network thread sees connection read buffers.  For every packet in them it unpacks the
 * header "!L12sL4s" and checks the magic and the length (state_bm_header, src/network/bmproto.py:85-104),
 * hashes the payload with SHA-512 and compares the first four bytes with the header's checksum
 * (state_bm_command, :106-111), and only then runs the command's handler (:113-156).  Here whole buffers
 * go through that in one call: the walk over the headers on host threads, one upload of the raw bytes, the
 * padded block pool written on the device, and per packet the checksum -- for an `object` packet out of
 * the same chain that gives its inventory hash and POW value, so it also gets the record
 * bmpow_intake_batch (bmpow_intake.h) would fill for its payload.
 *
 * Same conventions as bmpow_intake.h (return codes, bmpow_last_error, thread safety, BMPOW_E_ABORTED while
 * bmpow_abort()'s flag is set).  The device calls run on shard 0's stream.
 */
#ifndef BMPOW_PACKETS_H
#define BMPOW_PACKETS_H

#include "bmpow_intake.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BMPOW_PKT_MAGIC 0xE9BEB4D9u
#define BMPOW_PKT_HEADER 24            /* protocol.Header.size */
#define BMPOW_PKT_MAX_MESSAGE 1600100u /* network/constants.py MAX_MESSAGE_SIZE */
/* the longest payload hashed on the device: the longest object the intake accepts (a 38-byte header and
 * 2^18 bytes behind it); longer ones are hashed on host threads while the device works */
#define BMPOW_PKT_MAX_DEVICE (BMPOW_INTAKE_MAX_PAYLOAD + 38u)

/* bmpow_packet_rec.status: 0, or the reasons the reference sets self.invalid for, in its order */
#define BMPOW_PKT_OK 0u
#define BMPOW_PKT_TOO_LONG 1u        /* payloadLength > MAX_MESSAGE_SIZE (:99-100); such a payload is not hashed */
#define BMPOW_PKT_BAD_CHECKSUM 2u    /* :109-111 */
#define BMPOW_PKT_NOT_ESTABLISHED 4u /* not fullyEstablished and not "error" / "version" / "verack" (:113-118) */

/* bmpow_packet_rec.command: the handler getattr(self, "bm_command_" + command.lower()) finds (:121-122) */
#define BMPOW_PKT_UNIMPLEMENTED 0 /* AttributeError: valid, ignored (:123-125) */
#define BMPOW_PKT_ERROR 1
#define BMPOW_PKT_GETDATA 2
#define BMPOW_PKT_INV 3
#define BMPOW_PKT_DINV 4
#define BMPOW_PKT_OBJECT 5
#define BMPOW_PKT_ADDR 6
#define BMPOW_PKT_PORTCHECK 7
#define BMPOW_PKT_PING 8
#define BMPOW_PKT_PONG 9
#define BMPOW_PKT_VERACK 10
#define BMPOW_PKT_VERSION 11

/* conn_flags */
#define BMPOW_PKT_CONN_ESTABLISHED 1u /* fullyEstablished */
#define BMPOW_PKT_CONN_DATAGRAM 2u    /* socket.SOCK_DGRAM */
/* bmpow_packets_frame only: walk on behind a version / verack, so that the count bounds what
 * bmpow_packets_batch can return for the buffer whatever the checksums turn out to be */
#define BMPOW_PKT_CONN_ALL 4u

/* bmpow_packet_conn.close */
#define BMPOW_PKT_OPEN 0
#define BMPOW_PKT_BAD_MAGIC 1       /* close_reason "Bad magic" (:95-98) */
#define BMPOW_PKT_INVALID_COMMAND 2 /* close_reason "Invalid command ..." (:147-151) */
#define BMPOW_PKT_HANDSHAKE 3       /* a valid version / verack: the caller runs its handler and calls again */

typedef struct bmpow_packet_rec {
  uint32_t conn;     /* index of the buffer */
  uint32_t offset;   /* of the header in its buffer; the payload follows at offset + 24 */
  uint32_t length;   /* payloadLength */
  uint8_t command;   /* BMPOW_PKT_* handler, matched without regard to case */
  uint8_t exact;     /* 1: the command is spelled as the handler's name, in lower case */
  uint16_t reserved;
  uint32_t checksum; /* the header's, as a big-endian number */
  uint32_t computed; /* SHA512(payload)[:4] the same way (bmpow_packets_batch; 0 for TOO_LONG) */
  uint32_t status;   /* BMPOW_PKT_* reasons, or'ed; bmpow_packets_frame knows no BAD_CHECKSUM */
  uint32_t reserved2;
  bmpow_intake_rec intake; /* of the payload, for a valid `object` packet (bmpow_packets_batch); else zeros */
} bmpow_packet_rec;

typedef struct bmpow_packet_conn {
  uint64_t consumed; /* offset of the first byte not dealt with; of the offending header after a close */
  uint32_t first;    /* the connection's first record */
  uint32_t count;    /* ... and how many */
  uint32_t close;    /* BMPOW_PKT_OPEN, BAD_MAGIC, INVALID_COMMAND or HANDSHAKE */
  uint32_t reserved;
} bmpow_packet_conn;

/*
 * Host only.  Walk one buffer by the reference's rules, the checksums taken for good:
 *   - fewer than 24 bytes left, or fewer than the payload: stop, consumed at the packet's start;
 *   - wrong magic: a stream socket closes with BAD_MAGIC, a datagram socket skips one byte and goes on;
 *   - a packet with a reason in status closes a stream socket with INVALID_COMMAND, its record the
 *     last; a datagram socket skips it;
 *   - the command is the 12 bytes without their trailing NULs; an unknown one is UNIMPLEMENTED and the
 *     walk goes on;
 *   - a valid version or verack ends the walk with HANDSHAKE, consumed behind it.
 * Returns the number of packets framed (which may exceed cap; only cap records are written, recs may be
 * null when cap is 0) and fills *conn (first = 0).  The records carry the header fields and status only.
 * BMPOW_E_ARG for a buffer of 4 GiB or more.
 */
BMPOW_API int64_t bmpow_packets_frame(const uint8_t *buf, uint64_t len, uint32_t conn_flags, bmpow_packet_rec *recs,
                                      size_t cap, bmpow_packet_conn *conn);

/* Host only.  The packets bmpow_packets_frame counts under BMPOW_PKT_CONN_ALL over n_conn buffers, on host
 * threads: the record capacity bmpow_packets_batch needs for them.  BMPOW_E_ARG as there. */
BMPOW_API int64_t bmpow_packets_count(size_t n_conn, const uint8_t *const *bufs, const uint64_t *lens,
                                      const uint32_t *conn_flags);

/* Host only.  The 128-byte pool blocks the row plan gives a payload of len bytes: as an object row
 * (object != 0: object[8:] padded; 0 where len < 8) or as a sum row (the whole payload padded). */
BMPOW_API uint32_t bmpow_packets_row_blocks(int object, uint64_t len);

/*
 * Frame n_conn buffers, hash every framed payload and judge: recs[conns[c].first .. + count) are buffer
 * c's packets up to the first one that closes it, with computed, the full status and, for a valid object
 * packet, the intake record of its payload under *params -- exactly what bmpow_intake_batch fills for the
 * same bytes (MALFORMED and TOO_LARGE objects keep their packet OK and the connection open).  The sum of
 * lens must stay below 2^32 and cap must hold every packet bmpow_packets_count counts (BMPOW_E_ARG
 * otherwise).  Returns the number of records written.
 */
BMPOW_API int64_t bmpow_packets_batch(size_t n_conn, const uint8_t *const *bufs, const uint64_t *lens,
                                      const uint32_t *conn_flags, const bmpow_intake_params *params,
                                      bmpow_packet_rec *recs, size_t cap, bmpow_packet_conn *conns);

/*
 * objectProcessor.ackDataHasAValidHeader (src/class_objectProcessor.py:1020-1054) for n acks: valid_out[i]
 * = 1 where ack i is at least 24 bytes, has the magic, a payloadLength equal to what is left of it and at
 * most 1,600,100, the right checksum and, its NULs stripped, the command "object" in exactly that
 * spelling.  intake_recs_out[i] (may be null) = the intake record of acks[i][24:] for the valid ones,
 * zeros for the others.
 */
BMPOW_API int bmpow_packets_ack_batch(size_t n, const uint8_t *const *acks, const uint64_t *lens,
                                      const bmpow_intake_params *params, uint8_t *valid_out,
                                      bmpow_intake_rec *intake_recs_out);

/* Counters of bmpow_packets_batch / bmpow_packets_ack_batch since the last reset. */
typedef struct bmpow_packets_stats {
  uint64_t calls;        /* calls that launched or hashed */
  uint64_t packets;      /* packets framed */
  uint64_t object_rows;  /* hashed by the object kernel: checksum, POW value and inventory hash */
  uint64_t sum_rows;     /* hashed by the sum kernel: checksum alone */
  uint64_t host_rows;    /* payloads above BMPOW_PKT_MAX_DEVICE, hashed on host threads */
  uint64_t empty_rows;   /* payloads of 0 bytes, answered from the constant */
  uint64_t blocks;       /* 128-byte pool blocks written on the device */
  double pack_ms;        /* kernel_ms: GPU time between events, per kernel */
  double object_ms;
  double sum_ms;
  double host_frame_ms;  /* the walk over the headers and the objects' header decode */
  double host_build_ms;  /* plan, row list and upload of the raw bytes */
  double host_run_ms;    /* launches, the host's own hashing, wait and the results' way back */
  double host_status_ms; /* the verdicts and the connections' tables */
} bmpow_packets_stats;

BMPOW_API int bmpow_packets_get_stats(bmpow_packets_stats *out);
BMPOW_API void bmpow_packets_reset_stats(void);

#ifdef __cplusplus
}
#endif

#endif /* BMPOW_PACKETS_H */
