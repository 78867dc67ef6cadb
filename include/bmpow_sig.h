/*
 * bmpow_sig.h -- C ABI of libbmpow_hip.so's batched ECDSA signature verification (receive side).
 *
 * The reference checks the signature of every v3 / v4 pubkey, every decrypted msg and every broadcast
 * it receives with highlevelcrypto.verify (src/highlevelcrypto.py:88-108;
 * src/class_objectProcessor.py:345-375, :557-568, :916; src/protocol.py:484): two
 * pyelliptic.ECC.verify calls (src/pyelliptic/ecc.py:387-440), one with SHA-1, then one with SHA-256
 * unless the first passed.  For a public key Q on secp256k1, a DER signature (r, s) and a digest e:
 *     w = s^-1, u1 = e w, u2 = r w (mod n, the group order);  R = u1 G + u2 Q
 *     valid iff R is not the point at infinity and x(R) mod n == r
 * Here a batch goes through that in one call; u2 Q, the expensive half, is computed once per
 * signature and serves both digests.
 *
 * Same conventions as bmpow.h (return codes, bmpow_last_error, thread safety); bmpow_abort() is
 * honoured between launches.  The calls run on the first selected device.
 */
#ifndef BMPOW_SIG_H
#define BMPOW_SIG_H

#include "bmpow.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BMPOW_SIG_INVALID 0
#define BMPOW_SIG_SHA1 1   /* valid under SHA-1 */
#define BMPOW_SIG_SHA256 2 /* valid under SHA-256 only */

/* Host only.  Returns 1 and writes r || s (32 big-endian bytes each) iff sig[0 .. len) is exactly one
 * canonical DER SEQUENCE { INTEGER r, INTEGER s } with 1 <= r, s <= n - 1: short-form lengths, minimal
 * non-negative integers, no trailing bytes (what the reference's ECDSA_verify accepts: it re-encodes
 * the decoded signature and compares).  Returns 0 otherwise, rs_out untouched. */
BMPOW_API int bmpow_sig_parse(const uint8_t *sig, size_t len, uint8_t rs_out[64]);

/* The raw equation for n (key, r || s, digest) triples: pub is X || Y (64 bytes), rs is r || s (64
 * bytes), e the digest as a 32-byte big-endian integer (a SHA-1 digest left-padded with zeros; any value
 * below 2^256 is taken mod n).  ok[i] = 1 iff both coordinates are < p, the point is on the curve,
 * 1 <= r, s < n, R = (e / s) G + (r / s) Q is not the point at infinity and x(R) mod n == r; else 0. */
BMPOW_API int bmpow_ecdsa_verify_digest(size_t n, const uint8_t *pub, const uint8_t *rs, const uint8_t *e, uint8_t *ok);

/* highlevelcrypto.verify for a batch: verdict[i] = BMPOW_SIG_SHA1 when sigs[i] is a valid signature of
 * msgs[i] by pubkeys[64 i ..] (X || Y) under SHA-1, BMPOW_SIG_SHA256 when it is valid under SHA-256
 * only, BMPOW_SIG_INVALID otherwise -- also for a signature bmpow_sig_parse refuses and for a key with
 * a coordinate >= p or off the curve, where the reference's `except:` returns False.  Messages may be
 * empty; one above 2^31 bytes is BMPOW_E_ARG.  n == 0 succeeds with nothing launched. */
BMPOW_API int bmpow_sig_verify(size_t n, const uint8_t *const *msgs, const uint64_t *msg_lens,
                               const uint8_t *const *sigs, const uint64_t *sig_lens, const uint8_t *pubkeys,
                               uint8_t *verdict);

/* Counters of the signature calls since the last reset.  The times are GPU time between events
 * recorded around the launches of each phase. */
typedef struct bmpow_sig_stats {
  uint64_t calls;     /* bmpow_sig_verify / bmpow_ecdsa_verify_digest calls that launched */
  uint64_t submitted; /* signatures the calls were given */
  uint64_t uploaded;  /* signatures parsed, with coordinates < p, and sent to the device */
  uint64_t ladders;   /* variable-base multiplications u2 Q run: one per uploaded signature */
  uint64_t launches;  /* kernel launches */
  double hash_ms;     /* SHA-1 + SHA-256 of the messages */
  double scalar_ms;   /* s^-1, u1, u2 mod n and u2's digits */
  double curve_ms;    /* key tables, ladder, combs and the final test */
  double host_ms;     /* wall time of the calls: parsing, padding, upload and the launches */
} bmpow_sig_stats;

BMPOW_API int bmpow_sig_get_stats(bmpow_sig_stats *out);
BMPOW_API void bmpow_sig_reset_stats(void);

#ifdef __cplusplus
}
#endif

#endif /* BMPOW_SIG_H */
