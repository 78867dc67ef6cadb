// bmpow_rxopen_rows.h -- one lane's work in the opening kernel (bmpow_rxopen.hip): AES-256-CBC decryption of
// a matched msg's ciphertext from where it lies in the MAC pool into its slot of the plaintext pool, as a plain
// function over byte pointers and the table pointer, so that tests/native/rxopen_sim.cpp runs the very same code
// on the host against libcrypto (in the manner of bmpow_seal_rows.h).
//
// Source and destination are different buffers.  The ciphertext starts at any byte: it lies at
// 64 blk + 22 + xl + yl of the pool, and the coordinates' lengths are whatever the sender wrote.  It is read
// with aligned 16-byte loads funnelled through shifts (as rxf::pack_chunk reads the plaintext): with
// sh = src mod 16, block b is bytes [sh, sh + 16) of the aligned chunks b and b + 1 behind src - sh; a chunk is
// loaded once and carried to the next block, and chunk b + 1 is not loaded at all where sh == 0.
//
// What is read: the aligned chunks that hold a ciphertext byte, [src - sh, src + clen rounded up to 16), and
// nothing else.  Both ends lie inside the row's nblk * 64 bytes of pool: the row starts on a 64-byte boundary
// at least 22 bytes in front of src, so rounding src down to 16 stays behind the row's start; and the padded
// pool row ends on a 64-byte boundary at least 9 bytes behind the ciphertext's end (0x80 and the bit length),
// so rounding the end up to 16 stays in front of the row's end.
//
// The destination slot is 16-byte aligned and clen bytes long; it ends up holding the plaintext and zeros
// behind it (all zeros where the padding is refused).  No register array is indexed by a run-time value.
#pragma once
#include <stdint.h>

#include "aes256_dev.h"
#include "bmpow_seal_rows.h"  // sl::store16

namespace rxs {

BM_DEV void load_chunk(uint32_t (&w)[4], const uint8_t* p) {  // 16-byte aligned; words in memory order
  __builtin_memcpy(w, __builtin_assume_aligned(p, 16), 16);
}

// Bytes [sh, sh + 16) of lo || hi as four big-endian words; hi is not looked at where sh == 0.
BM_DEV void funnel(uint32_t (&out)[4], const uint32_t (&lo)[4], const uint32_t (&hi)[4], uint32_t sh) {
  const uint32_t ws = sh >> 2, bs = 8 * (sh & 3u);
  uint32_t w[8], t[5];
#pragma unroll
  for (int i = 0; i < 4; ++i) w[i] = lo[i], w[4 + i] = hi[i];
#pragma unroll
  for (int i = 0; i < 5; ++i)
    t[i] = ws == 0 ? w[i] : ws == 1 ? w[i + 1 < 8 ? i + 1 : 7] : ws == 2 ? w[i + 2 < 8 ? i + 2 : 7] : w[i + 3 < 8 ? i + 3 : 7];
#pragma unroll
  for (int i = 0; i < 4; ++i) out[i] = __builtin_bswap32(bs ? (t[i] >> bs) | (t[i + 1] << ((32 - bs) & 31)) : t[i]);
}

// AES-256-CBC of src[0 .. clen), clen a positive multiple of 16 (the host's check), under key and iv
// (big-endian words, the top word first) into dst.  Returns the plaintext's length, or -1 for padding
// EVP_DecryptFinal_ex refuses (the rule of sl::cbc_decrypt_row): the last byte not in 1 .. 16, or the pad bytes
// not all it.
BM_DEV int32_t open_row(const uint8_t* src, uint32_t clen, const uint32_t (&key)[8], const uint32_t (&iv)[4], uint8_t* dst,
                        const aes::DecTab& l) {
  uint32_t dk[60], prev[4], ct[4], p[4], lo[4], hi[4];
  aes::expand_dec_key(dk, key, l);
  const uint32_t sh = (uint32_t)((uintptr_t)src & 15u), nblk = clen / 16;
  const uint8_t* base = src - sh;
#pragma unroll
  for (int i = 0; i < 4; ++i) prev[i] = iv[i], p[i] = 0, hi[i] = 0;
  load_chunk(lo, base);
  for (uint32_t b = 0; b < nblk; ++b) {
    if (sh) load_chunk(hi, base + 16 * (size_t)(b + 1));
    funnel(ct, lo, hi, sh);
#pragma unroll
    for (int i = 0; i < 4; ++i) p[i] = ct[i];
    aes::decrypt_block(p, dk, l);
#pragma unroll
    for (int i = 0; i < 4; ++i) p[i] ^= prev[i], prev[i] = ct[i];
    if (b + 1 < nblk) {
      sl::store16(dst + 16 * (size_t)b, p);
      if (sh) {
#pragma unroll
        for (int i = 0; i < 4; ++i) lo[i] = hi[i];
      } else {
        load_chunk(lo, base + 16 * (size_t)(b + 1));
      }
    }
  }
  const uint32_t pad = p[3] & 0xffu;
  bool good = pad >= 1 && pad <= 16;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const uint32_t byte = (p[k / 4] >> (24 - 8 * (k % 4))) & 0xffu;
    if ((uint32_t)k >= 16u - pad && byte != pad) good = false;
  }
  if (!good) {
    const uint32_t zero[4] = {0, 0, 0, 0};
    for (uint32_t b = 0; b < nblk; ++b) sl::store16(dst + 16 * (size_t)b, zero);
    return -1;
  }
  const uint32_t keep = 16u - pad;  // plaintext bytes of the last block, from the top of p[0]
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t kb = keep > 4u * j ? (keep - 4u * j >= 4u ? 4u : keep - 4u * j) : 0u;
    p[j] &= kb == 4u ? 0xffffffffu : (kb == 0u ? 0u : ~(0xffffffffu >> (8u * kb)));
  }
  sl::store16(dst + 16 * (size_t)(nblk - 1), p);
  return (int32_t)(clen - pad);
}

}  // namespace rxs
