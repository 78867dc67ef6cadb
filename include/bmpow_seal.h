/*
 * bmpow_seal.h -- C ABI of libbmpow_hip.so's AES-256-CBC and HMAC-SHA256 on the device: the seal of outgoing
 * ECIES blobs and the raw cipher.  Included by bmpow_send.h and bmpow_ecies.h, whose calls it extends.
 *
 * The reference finishes every blob in ECC.raw_encrypt (src/pyelliptic/ecc.py:472-482): AES-256-CBC of the
 * PKCS#7-padded plaintext under key_e, HMAC-SHA256 of everything before under key_m; ECC.decrypt runs the
 * cipher the other way (:499-501).  bmpow_ecies_encrypt (bmpow_send.h) does that pass on the host's
 * threads or, by bmpow_send_set_seal, on the device behind its ladder, where the derived keys stay.
 *
 * Same conventions as bmpow.h (return codes, bmpow_last_error, thread safety); bmpow_abort() is honoured
 * between sets.  The calls run on the first selected device.  n == 0 succeeds with nothing launched.
 * The AES tables are indexed by key-dependent bytes: not constant-time (send side).
 */
#ifndef BMPOW_SEAL_H
#define BMPOW_SEAL_H

#include "bmpow.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bmpow_ecies_seal for n rows, on the device: outs[i][0 .. out_lens[i]) = the blob of plains[i] under
 * ivs[16 i ..], R_xy[64 i ..] and keys[64 i ..], byte for byte what bmpow_ecies_seal writes.  The rows are
 * sorted by block count and go through sl_seal_kernel in sets of at most 2^18 rows and 256 MB of pool; a
 * row above 256 KiB (the protocol's object limit) is sealed by the host's code instead.  R_xy is taken as
 * bytes: no curve check.  out_caps[i] below BMPOW_ECIES_BLOB_CAP(lens[i]) or a plaintext above 2^31 - 16
 * bytes is BMPOW_E_ARG.  Runs whatever bmpow_send_set_seal says. */
BMPOW_API int bmpow_ecies_seal_batch(size_t n, const uint8_t *const *plains, const uint64_t *lens, const uint8_t *ivs,
                                     const uint8_t *R_xy, const uint8_t *keys, uint8_t *const *outs,
                                     const uint64_t *out_caps, uint64_t *out_lens);

/* Where bmpow_ecies_encrypt seals its blobs: 0 on the host's threads (libcrypto), 1 on the device, where the
 * derived keys and the ephemeral points never reach host memory.  The blobs are the same bytes either way.
 * -1 (or any other value) only queries.  Returns the previous mode; touches no device.  The initial mode
 * is BMPOW_SEAL=host|device from the environment, device without it. */
BMPOW_API int bmpow_send_set_seal(int mode);

/* Host only: the set planner of the device seal.  Row i of n, in the given order, goes to set set_out[i]
 * (counted from 0) at offset off_out[i] of that set's pool: slots of 16-byte multiples at 16-byte
 * multiples, a new set after max_rows rows or when the next slot would pass max_bytes (a slot larger
 * than max_bytes gets a set of its own).  Returns the number of sets; BMPOW_E_ARG for a null pointer, a
 * zero limit or a length above 2^31 - 16. */
BMPOW_API int64_t bmpow_seal_plan(size_t n, const uint64_t *lens, uint64_t max_rows, uint64_t max_bytes,
                                  uint32_t *set_out, uint64_t *off_out);

/* Counters of the device seal and the raw CBC call (bmpow_aes256_cbc) since the last reset. */
typedef struct bmpow_seal_stats {
  uint64_t calls;        /* bmpow_ecies_encrypt (device mode) / bmpow_ecies_seal_batch / bmpow_aes256_cbc calls that launched */
  uint64_t rows_device;  /* rows sealed, encrypted or decrypted by a kernel */
  uint64_t rows_host;    /* rows above 256 KiB, sealed by the host's code */
  uint64_t sets;         /* sets of at most 2^18 rows and 256 MB */
  uint64_t launches;     /* seal / CBC kernel launches */
  double seal_kernel_ms; /* GPU time of those kernels, between events */
  double pack_ms;        /* host: copying the inputs into the staging pool (wall time over the host's threads) */
  double copy_ms;        /* the pool's upload and download, between events */
  double scatter_ms;     /* host: copying the outputs out of the staging pool */
} bmpow_seal_stats;

BMPOW_API int bmpow_seal_get_stats(bmpow_seal_stats *out);
BMPOW_API void bmpow_seal_reset_stats(void);

/* Raw AES-256-CBC with PKCS#7 padding of n messages on the device, each under its own key (keys[32 i ..])
 * and IV (ivs[16 i ..]).  Encrypt: out[i] receives 16 (in_lens[i] / 16 + 1) bytes.  Decrypt: out[i]
 * receives the plaintext; out_lens[i] = -1 (and out[i] untouched) for an input that is empty or no
 * multiple of 16 bytes, or whose padding EVP_DecryptFinal_ex refuses (last byte not in 1 .. 16, or pad
 * bytes that differ).  out_lens[i] is the output's length otherwise.  out_caps[i] must be at least the
 * padded length (encrypt) or in_lens[i] (decrypt), else BMPOW_E_ARG; a message above 2^31 - 16 bytes
 * too.  n == 0 succeeds with nothing launched.  Counted in bmpow_seal_stats. */
BMPOW_API int bmpow_aes256_cbc(size_t n, int decrypt, const uint8_t *keys, const uint8_t *ivs, const uint8_t *const *in,
                               const uint64_t *in_lens, uint8_t *const *out, const uint64_t *out_caps, int64_t *out_lens);

#ifdef __cplusplus
}
#endif

#endif /* BMPOW_SEAL_H */
