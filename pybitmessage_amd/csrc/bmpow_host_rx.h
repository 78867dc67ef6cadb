// bmpow_host_rx.h -- what the host units that run the msg-processing kernels share (internal): one call's
// device buffers, and a set's nine launches over a plaintext pool that is already on the device.  Used by
// bmpow_host_rx.hip (bmpow_rx_msgs, which uploads the plaintexts) and bmpow_host_rxopen.hip
// (bmpow_rx_sealed_msgs, whose opening kernel leaves them there).
#pragma once
#include "bmpow_host_sig.h"

#include "../../include/bmpow_rx.h"
#include "bmpow_ident_kernels.h"
#include "bmpow_rx_kernels.h"

namespace bmhost {

struct RxBufs {
  DevBuf<rx_row> rows;
  DevBuf<uint4> plain, keys;
  DevBuf<bmpow_rx_msg_rec> recs;
  DevBuf<uint64_t> versions, streams;
  DevBuf<rx_pk> pk;
  DevBuf<uint8_t> flags;
  DevBuf<bmpow_ident_rec> ident;
  Event ev[7];
};

// Room for a set of stride rows (a multiple of SG_BLOCK), pool_chunks of padded signed data and plain_chunks
// of plaintext, both in 16-byte units.
int rx_grow_set(Shard& sh, SigBufs& b, RxBufs& x, uint32_t stride, uint64_t pool_chunks, uint64_t plain_chunks);

// The nine launches of a set on sh.stream, with x.ev[0 .. 6] recorded around their six phases: walk, pack, hash,
// scalars, prep, ladder, comb, derive, finish.  x.rows[0 .. n) and the plaintext pool x.plain are on the device
// (an upload, or kernels, enqueued on the same stream before); the records end up in x.recs[0 .. n).
int rx_launch_set(Shard& sh, SigBufs& b, RxBufs& x, const ec::ge* comb, uint32_t n, uint32_t stride, uint64_t plain_chunks,
                  uint64_t pool_chunks);

// The six phase times of the last rx_launch_set (its events have completed), added to st.
int rx_phase_times(const RxBufs& x, bmpow_rx_stats& st);

}  // namespace bmhost
