// bmpow_intake_dev.h -- the per-object hash chains of the intake (device): the receive-side POW value and the
// inventory hash from one pass over the padded payload pool, shared by the intake kernels (bmpow_intake.hip)
// and the packet kernels (bmpow_packets.hip), which also take the packet's checksum out of the same chain.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bmpow_layout.h"
#include "sha512_dev.h"

namespace bm {

// ---------------------------------------------------------------------------------------
// One lane per object, over the verification's pool: object[8:] SHA-512-padded to nblk blocks.  The
// lane runs bv_pow_kernel's chain (nblk payload blocks, then the trial's two), and then the inventory
// chain over the same pool words: the full object is the payload stream shifted by one 64-bit word with
// the nonce in front, so with L the object's length and nblk2 = ceil((L + 17) / 128) (nblk or nblk + 1)
// word k of its padded message is
//     the nonce            k == 0
//     8 L                  k == 16 nblk2 - 1
//     0                    k >= 16 nblk        (the pool's own length word must not shift in)
//     P[k - 1]             otherwise
// (the 0x80 byte shifts with the payload; checked on the CPU against direct padding for every L in
// tests/test_intake.py).  The digest's own one-block hash follows.  One copy of the compression body
// serves all nblk + 2 + nblk2 + 1 blocks, as in pow_of: the message words come from selects, and the
// state restarts at the IV wherever a chain begins.
//
// The inventory chain reads each pool block once more, with the same aligned 16-B loads (L2 hits for
// all but the longest objects), and carries the block's last word into the next block's word 0: no
// unaligned access, 2 VGPRs.  BI_SHIFTED_LOADS (A/B) reads words k - 1 .. k + 14 with sixteen 8-B
// loads instead.
//
// kSum (the packet kernels): SHA512(object)[:4], the checksum of the `object` packet whose payload the
// object is, is the high half of the inventory chain's first digest word.  It is stored to *sum_out where
// that chain hands its digest to the last block, not carried across the last compression: the binned
// kernel has no register to spare.
// ---------------------------------------------------------------------------------------
template <bool kSum>
BM_DEV void intake_chain(const bv_obj& o, uint32_t L, const uint4* __restrict__ pool, uint64_t& pow,
                         uint64_t (&inv)[4], uint32_t* __restrict__ sum_out) {
  uint64_t h[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) h[i] = IV(i);
  const uint4* base = pool + (uint64_t)o.blk * 8;
  const uint32_t nb = o.nblk;
  const uint32_t nb2 = (uint32_t)(((uint64_t)L + 17 + 127) >> 7);
  const uint32_t i0 = nb + 2;              // first block of the inventory chain
  const uint32_t total = i0 + nb2 + 1;     // ... and the digest's block after it
  const uint64_t nonce = o.nonce;
#ifndef BI_SHIFTED_LOADS
  uint64_t carry = 0;  // the previous block's last pool word
#endif
  pow = 0;
  for (uint32_t b = 0; b < total; ++b) {
    const bool pay = b < nb, t1 = b == nb;
    const uint32_t c = b - i0;             // block of the inventory chain (when ich)
    const bool ich = b >= i0 && c < nb2;
    const uint32_t lb = pay ? b : (ich && c < nb ? c : nb - 1);  // never past the object's blocks
    uint64_t w[16];
#ifdef BI_SHIFTED_LOADS
    if (ich) {
      const uint2* q = (const uint2*)base;
      const uint32_t k0 = 16 * lb;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const uint2 v = q[k0 + i > 0 ? k0 + i - 1 : 0];
        w[i] = be64(v.x, v.y);
      }
    } else
#endif
    {
      const uint4* p = base + (uint64_t)lb * 8;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const uint4 v = p[j];
        w[2 * j] = be64(v.x, v.y);
        w[2 * j + 1] = be64(v.z, v.w);
      }
    }
    if (!pay) {
      // a chain begins: trial block 1 and 2, the inventory chain's first block, the digest's block
      const bool restart = !ich || c == 0;
      uint64_t d[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) d[i] = h[i], h[i] = restart ? IV(i) : h[i];
      if (b == i0) pow = d[0];             // the trial's second digest
      if (kSum && b == total - 1) *sum_out = hi32(d[0]);  // the inventory chain's first digest
      if (ich) {
        const bool zero = c >= nb, last = c == nb2 - 1;
#ifdef BI_SHIFTED_LOADS
        if (c == 0) w[0] = nonce;
#else
        const uint64_t w15 = w[15];
#pragma unroll
        for (int i = 15; i > 0; --i) w[i] = w[i - 1];
        w[0] = c == 0 ? nonce : carry;
        carry = w15;
#endif
#pragma unroll
        for (int i = 0; i < 16; ++i) w[i] = zero ? 0 : w[i];
        if (last) w[15] = (uint64_t)L << 3;
      } else {
        // trial block 1: nonce || payload digest || padding (72 B); else a digest || padding (64 B)
        w[0] = t1 ? nonce : d[0];
#pragma unroll
        for (int i = 1; i < 8; ++i) w[i] = t1 ? d[i - 1] : d[i];
        w[8] = t1 ? d[7] : PAD;
        w[9] = t1 ? PAD : 0;
#pragma unroll
        for (int i = 10; i < 15; ++i) w[i] = 0;
        w[15] = t1 ? 72 * 8 : 64 * 8;
      }
    }
    compress(h, w);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) inv[i] = h[i];
}

BM_DEV void intake_of(const bv_obj& o, uint32_t L, const uint4* __restrict__ pool, uint64_t& pow,
                      uint64_t (&inv)[4]) {
  intake_chain<false>(o, L, pool, pow, inv, nullptr);
}

}  // namespace bm
