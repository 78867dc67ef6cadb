// bmpow_host_vbatch.h -- the verification batch (pool, descriptors, bins per shard) as the host units
// that launch over it see it: bmpow_host_verify.hip builds and runs it, bmpow_host_intake.hip runs the
// intake kernels over the same build.  Internal, like bmpow_host.h.
#pragma once
#include "bmpow_host.h"

// ---------------------------------------------------------------------------------------
// Receive-side verification session.  Layout per shard, device resident:
//   pool[blocks]  : every payload (object[8:]) SHA-512-padded to whole 128-B blocks, objects
//                   back to back in sorted order (so one lane reads one contiguous run)
//   obj[k]        : {first block, block count, nonce} of the k-th object in sorted order
//   pow[k]        : result
// Objects are sorted by block count (descending) so a wave's lanes iterate alike, and the
// sorted list is cut into per-shard slices of equal block totals.
// ---------------------------------------------------------------------------------------
struct bmpow_vbatch {
  size_t n = 0;
  struct Part : bmsched::VPart {  // shard, sorted order, bv_obj list, blocks (bmpow_sched.h)
    bv_obj* d_obj = nullptr;
    uint4* d_pool = nullptr;
    uint64_t* d_pow = nullptr;
    uint64_t* h_pow = nullptr;  // pinned
    uint32_t* d_bins = nullptr; // plan_bins' offsets + group lists (binned kernel), or null
    // The pointers above are what the kernels read: a session's own buffers, held here, or (the one-shot
    // path, these left empty) plain pointers into the shard's buffers (VerifyShard).
    struct Own {
      bmown::DevBuf<bv_obj> obj;
      bmown::DevBuf<uint4> pool;
      bmown::DevBuf<uint64_t> pow;
      bmown::PinBuf<uint64_t> h_pow;
      bmown::DevBuf<uint32_t> bins;
    } own;
  };
  std::vector<Part> parts;
  uint64_t blocks = 0;
  uint64_t generation = ~0ULL;  // g_generation of the shard set the parts were built for (vbatch_build)
};

namespace bmhost {

// Plan, pad and upload objs (bmpow_host_verify.hip).  transient: the one-shot path, into the shards'
// grow-only buffers through their pinned staging chunks; the plan's vectors then go back with
// vbatch_release_plan before the batch is freed.  Under g_mu.
int vbatch_build(bmpow_vbatch* vb, const std::vector<bmsched::Span>& objs, bool transient = false);
void vbatch_release_plan(bmpow_vbatch* vb);

}  // namespace bmhost
