/*
 * bmpow_ecies.h -- C ABI of libbmpow_hip.so's batched ECIES trial decryption (receive side).
 *
 * The reference tries every received msg (and broadcast) against every private key the user holds,
 * one pyelliptic.ECC.decrypt per try (src/class_objectProcessor.py:459-477, :779-790;
 * src/pyelliptic/ecc.py:484-501).  For a payload `data` (the object's bytes from its encrypted part
 * on) and a 32-byte private key k:
 *     iv = data[0:16]; then curve (2 B, ignored) | xlen (2 B, big-endian) | X | ylen (2 B) | Y;
 *     then the ciphertext, then a 32-byte MAC
 *     key = SHA512(x(k * (X, Y))) with x as 32 big-endian bytes; key_e = key[:32], key_m = key[32:]
 *     k matches iff HMAC_SHA256(key_m, data[:-32]) == data[-32:]
 *     plaintext = AES-256-CBC(key_e, iv) of the ciphertext, PKCS#7 padded
 * X and Y are integers of any length, reduced mod p as the reference's OpenSSL does.  A payload whose
 * key header does not lie inside data[:-32], or whose point is not on secp256k1, matches no key.
 *
 * Same conventions as bmpow.h (return codes, bmpow_last_error, thread safety); bmpow_abort() is
 * honoured between launches.  The calls run on the first selected device.
 */
#ifndef BMPOW_ECIES_H
#define BMPOW_ECIES_H

#include "bmpow.h"
#include "bmpow_seal.h" /* bmpow_aes256_cbc: the raw cipher on the device */

#ifdef __cplusplus
extern "C" {
#endif

/* Raw ECDH, strict: x_out[32 i ..] = x(priv_i * pub_i) as 32 big-endian bytes for n (key, point)
 * pairs; pub is X || Y, 32 big-endian bytes each.  ok[i] = 0 (and x_out zeroed) for a coordinate
 * >= p, a point off the curve, or a key that is 0 or >= n (the group order); else 1. */
BMPOW_API int bmpow_ecdh(size_t n, const uint8_t *priv, const uint8_t *pub, uint8_t *x_out, uint8_t *ok);

/* Host only.  Parse a payload's key header: xy_out = X mod p || Y mod p (32 big-endian bytes each),
 * *body_off = offset of the ciphertext (data[*body_off : len - 32]).  Returns 1 for a well-formed
 * payload (the header lies inside data[:-32]), 0 for a malformed one.  The curve equation is not
 * checked here. */
BMPOW_API int bmpow_ecies_parse(const uint8_t *payload, size_t len, uint8_t xy_out[64], size_t *body_off);

/* match[i] = the lowest index of a key in privkeys[n_keys x 32] whose MAC verifies for payload i, or
 * -1 (also for a malformed or off-curve payload).  key_e_out (n_obj x 32 bytes, or NULL) receives
 * key_e of the matching pair, zeros where none matches.  Every key is tried against every object.
 * A key that is 0 or >= the group order gives BMPOW_E_ARG.  n_obj == 0 or n_keys == 0 succeeds with
 * nothing launched (match all -1). */
BMPOW_API int bmpow_ecies_match(size_t n_obj, const uint8_t *const *payloads, const uint64_t *lens, size_t n_keys,
                                const uint8_t *privkeys, int32_t *match, uint8_t *key_e_out);

/* Host only.  AES-256-CBC decryption of the payload's ciphertext with key_e and the payload's iv
 * into out[0 .. out_cap); out_cap must be at least the ciphertext's length.  Returns the plaintext's
 * length, or BMPOW_E_ARG for a malformed payload, a ciphertext that is empty or no multiple of 16
 * bytes, or bad PKCS#7 padding (where the reference's decrypt raises). */
BMPOW_API int64_t bmpow_ecies_decrypt(const uint8_t *payload, size_t len, const uint8_t key_e[32], uint8_t *out,
                                      size_t out_cap);

/* Counters of the ECIES calls since the last reset.  The times are GPU time between events recorded
 * around each launch. */
typedef struct bmpow_ecies_stats {
  uint64_t calls;      /* bmpow_ecies_match calls that launched */
  uint64_t objects;    /* well-formed objects uploaded */
  uint64_t pairs;      /* (object, key) tries */
  uint64_t launches;   /* ladder launches (each followed by one MAC launch) */
  double prep_ms;      /* on-curve check + tables, once per object */
  double ecdh_ms;      /* ladder + SHA-512 */
  double mac_ms;       /* HMAC-SHA256 + compare (+ the key_e gather) */
  double host_ms;      /* wall time of the calls: parsing, padding, upload and the launches */
} bmpow_ecies_stats;

BMPOW_API int bmpow_ecies_get_stats(bmpow_ecies_stats *out);
BMPOW_API void bmpow_ecies_reset_stats(void);

#ifdef __cplusplus
}
#endif

#endif /* BMPOW_ECIES_H */
