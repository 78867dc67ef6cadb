/*
 * bmpow_send.h -- C ABI of libbmpow_hip.so's batched ECDSA signing and ECIES encryption (send side).
 *
 * The reference signs and encrypts every outgoing msg, broadcast and pubkey with highlevelcrypto.sign /
 * encrypt (src/highlevelcrypto.py:54-85; src/class_singleWorker.py:1224-1234), one pyelliptic call
 * per object: a fixed-base multiplication k G for the signature (src/pyelliptic/ecc.py:319-385), and
 * for ECIES a fresh key pair (r, R = r G), the shared x(r Q) with the recipient's key Q, SHA-512 of it
 * as key_e || key_m, AES-256-CBC and HMAC-SHA256 (ECC.raw_encrypt, :462-482).  Its addresses' public
 * keys come from highlevelcrypto.pointMult (:111-146).  Here a batch goes through each in one call: the
 * curve and scalar arithmetic on the device, and the AES / HMAC pass either on the host's threads
 * (libcrypto) or on the device as well (sl_seal_kernel), by bmpow_send_set_seal / BMPOW_SEAL.
 *
 * Same conventions as bmpow_sig.h / bmpow_ecies.h (return codes, bmpow_last_error, thread safety);
 * bmpow_abort() is honoured between launches.  The calls run on the first selected device.  n == 0
 * succeeds with nothing launched.
 */
#ifndef BMPOW_SEND_H
#define BMPOW_SEND_H

#include "bmpow.h"
#include "bmpow_seal.h" /* the device seal's calls, the mode knob and its counters */
#include "bmpow_sig.h"

#ifdef __cplusplus
extern "C" {
#endif

/* highlevelcrypto.pointMult without the 0x04: pub_out[64 i ..] = X || Y (32 big-endian bytes each) of
 * priv[32 i ..] G, ok[i] = 1.  A key that is 0 or >= n (the group order) gives ok[i] = 0 and zeros. */
BMPOW_API int bmpow_ec_pubkeys(size_t n, const uint8_t *priv, uint8_t *pub_out, uint8_t *ok);

/* The raw signing equation for n (key d, nonce k, digest e) triples of 32 big-endian bytes each:
 * r = x(k G) mod n, s = (e + r d) / k mod n, rs_out[64 i ..] = r || s, ok[i] = 1.  e is any value below
 * 2^256, taken mod n as bmpow_ecdsa_verify_digest takes it.  d or k equal to 0 or >= n, r == 0 or
 * s == 0 give ok[i] = 0 and zeros.  s is not normalised to the low half (the reference's ECDSA_sign
 * does not either). */
BMPOW_API int bmpow_ecdsa_sign_digest(size_t n, const uint8_t *priv, const uint8_t *k, const uint8_t *e,
                                      uint8_t *rs_out, uint8_t *ok);

/* Host only.  The canonical DER SEQUENCE { INTEGER r, INTEGER s } of rs = r || s (what bmpow_sig_parse
 * accepts: minimal integers, a 0x00 in front when the top bit is set), at most 72 bytes; *len its
 * length.  r or s equal to 0 is BMPOW_E_ARG. */
BMPOW_API int bmpow_sig_der(const uint8_t rs[64], uint8_t out[72], size_t *len);

/* highlevelcrypto.sign for a batch: sig_out[72 i ..] = the DER signature of msgs[i] by privkeys[32 i ..]
 * under digest (BMPOW_SIG_SHA1 or BMPOW_SIG_SHA256: the reference's digestalg setting, sha256 by
 * default), sig_len[i] its length.  A private key that is 0 or >= n is BMPOW_E_ARG; a message above
 * 2^31 bytes too.  nonces == NULL: each k is drawn from [1, n - 1] with libcrypto's RAND_bytes by
 * rejection; a row that comes back with r == 0 or s == 0 is redrawn and rerun, at most three passes,
 * then sig_len[i] = 0.  With nonces (32 big-endian bytes per row) one that is 0 or >= n is
 * BMPOW_E_ARG, and a row with r == 0 or s == 0 gets sig_len[i] = 0. */
BMPOW_API int bmpow_sig_sign(size_t n, const uint8_t *const *msgs, const uint64_t *msg_lens, const uint8_t *privkeys,
                             int digest, const uint8_t *nonces, uint8_t *sig_out, uint8_t *sig_len);

/* The bound on an ECIES blob of a len-byte plaintext: 16 IV + 2 curve + 2 x (2 + 32) key + the padded
 * ciphertext + 32 MAC. */
#define BMPOW_ECIES_BLOB_CAP(len) (118 + 16 * ((size_t)(len) / 16 + 1))

/* Host only: everything of ECC.raw_encrypt after the key derivation.  key = SHA512(shared x) =
 * key_e || key_m, R_xy = X || Y of the ephemeral public key.  Writes
 *     iv | 0x02CA | len X | X | len Y | Y | AES-256-CBC(key_e, iv, PKCS#7(plain)) | HMAC-SHA256(key_m, all before)
 * with X and Y at minimal length (leading zero bytes stripped, as BN_bn2bin leaves them in the
 * reference's get_pubkey()) and returns the blob's length; BMPOW_E_ARG when out_cap is smaller than
 * that or the plaintext above 2^31 - 16 bytes. */
BMPOW_API int64_t bmpow_ecies_seal(const uint8_t *plain, size_t len, const uint8_t iv[16], const uint8_t R_xy[64],
                                   const uint8_t key[64], uint8_t *out, size_t out_cap);

/* highlevelcrypto.encrypt for a batch: outs[i][0 .. out_lens[i]) = the blob of plains[i] to the
 * recipient key pubkeys[64 i ..] (X || Y).  out_lens[i] = 0 for a recipient key with a coordinate >= p
 * or off the curve (the reference raises there and sendMsg logs "encrypt didn't work").  out_caps[i]
 * below BMPOW_ECIES_BLOB_CAP(lens[i]) is BMPOW_E_ARG.  ephem (32 big-endian bytes per row) are the
 * ephemeral private keys, ivs (16 bytes per row) the IVs; either may be NULL: drawn from RAND_bytes,
 * the keys from [1, n - 1] by rejection.  A supplied ephemeral key that is 0 or >= n is BMPOW_E_ARG. */
BMPOW_API int bmpow_ecies_encrypt(size_t n, const uint8_t *const *plains, const uint64_t *lens, const uint8_t *pubkeys,
                                  const uint8_t *ephem, const uint8_t *ivs, uint8_t *const *outs,
                                  const uint64_t *out_caps, uint64_t *out_lens);

/* Counters of the send-side calls since the last reset.  The GPU times are between events recorded
 * around the launches of each phase. */
typedef struct bmpow_send_stats {
  uint64_t calls;    /* bmpow_ec_pubkeys / bmpow_ecdsa_sign_digest / bmpow_sig_sign / bmpow_ecies_encrypt calls that launched */
  uint64_t rows;     /* rows sent to the device (a redrawn signature counts again) */
  uint64_t sets;     /* sets of at most 2^18 rows the calls went through the device in */
  uint64_t launches; /* kernel launches */
  double hash_ms;    /* SHA-1 + SHA-256 of the messages */
  double comb_ms;    /* k G by the comb, and its inversion */
  double scalar_ms;  /* r, k^-1 and s mod n; the ephemeral key's digits */
  double ladder_ms;  /* recipient tables, r Q, its inversion and SHA-512 */
  double seal_ms;    /* host: AES-256-CBC and HMAC-SHA256 (wall time over the host's threads) */
  double host_ms;    /* wall time of the calls */
} bmpow_send_stats;

BMPOW_API int bmpow_send_get_stats(bmpow_send_stats *out);
BMPOW_API void bmpow_send_reset_stats(void);

#ifdef __cplusplus
}
#endif

#endif /* BMPOW_SEND_H */
