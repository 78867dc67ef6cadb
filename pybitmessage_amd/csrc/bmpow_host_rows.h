// bmpow_host_rows.h -- the one host pipeline of the signed rows the receive side processes (internal): msgs
// (bmpow_host_rx.hip, bmpow_host_rxopen.hip) and broadcasts and pubkeys (bmpow_host_rxobj.hip).  Both families
// take the same nine launches over the same buffers -- walk, pack, hash, scalars, key tables, ladder, combs,
// identification, finish -- and differ in their row, pack and record types and in the three kernels of their
// own.  A family is a small struct that names those:
//
//   struct Family {
//     using Row = ...;  using Pk = ...;  using Rec = ...;   // rows have poff, plen and blk
//     static constexpr auto walk = ..._launch_walk;         // and pack and finish: the family's launchers
//   };
//
// and run_rows drives a whole call for a policy that knows where a row's bytes come from.
#pragma once
#include "bmpow_host_sig.h"

#include "bmpow_ident_kernels.h"

namespace bmhost {

template <class F>
struct RowBufs {  // one call's buffers on the device, beside its SigBufs
  DevBuf<typename F::Row> rows;
  DevBuf<uint4> plain, keys;
  DevBuf<typename F::Rec> recs;
  DevBuf<uint64_t> versions, streams;
  DevBuf<typename F::Pk> pk;
  DevBuf<uint8_t> flags;
  DevBuf<bmpow_ident_rec> ident;
  Event ev[7];
};

// Room for a set of stride rows (a multiple of SG_BLOCK), pool_chunks of padded signed data and plain_chunks
// of plaintext, both in 16-byte units.
template <class F>
int grow_set(Shard& sh, SigBufs& b, RowBufs<F>& x, uint32_t stride, uint64_t pool_chunks, uint64_t plain_chunks) {
  HIPTRY(x.rows.grow(sh.dev, stride));
  HIPTRY(x.plain.grow(sh.dev, plain_chunks));
  HIPTRY(x.keys.grow(sh.dev, (size_t)8 * stride));
  HIPTRY(x.recs.grow(sh.dev, stride));
  HIPTRY(x.versions.grow(sh.dev, stride));
  HIPTRY(x.streams.grow(sh.dev, stride));
  HIPTRY(x.pk.grow(sh.dev, stride));
  HIPTRY(x.flags.grow(sh.dev, stride));
  HIPTRY(x.ident.grow(sh.dev, stride));
  return b.grow(sh, stride, pool_chunks);
}

// The nine launches of a set on sh.stream, with x.ev[0 .. 6] recorded around their six phases.  x.rows[0 .. n)
// and the plaintext pool x.plain are on the device (an upload, or kernels, enqueued on the same stream before);
// the records end up in x.recs[0 .. n).
template <class F>
int launch_set(Shard& sh, SigBufs& b, RowBufs<F>& x, const ec::ge* comb, uint32_t n, uint32_t stride, uint64_t plain_chunks,
               uint64_t pool_chunks) {
  const uint8_t* d_plain = reinterpret_cast<const uint8_t*>(x.plain.get());
  HIPTRY(hipEventRecord(x.ev[0].get(), sh.stream));
  HIPTRY(F::walk(sh.stream, x.rows.get(), d_plain, n, stride, x.recs.get(), b.sigs.get(), b.pts.get(), x.keys.get(),
                 x.versions.get(), x.streams.get(), x.pk.get(), x.flags.get()));
  HIPTRY(F::pack(sh.stream, x.rows.get(), x.plain.get(), plain_chunks, b.sigs.get(), x.pk.get(), n, b.pool.get(),
                 pool_chunks));
  HIPTRY(hipEventRecord(x.ev[1].get(), sh.stream));
  HIPTRY(sg_launch_hash(sh.stream, b.sigs.get(), b.pool.get(), n, stride, b.e.get()));
  HIPTRY(hipEventRecord(x.ev[2].get(), sh.stream));
  if (const int rc = sig_launch_verify(sh, b, comb, n, stride, 2, x.ev[3]); rc < 0) return rc;
  HIPTRY(hipEventRecord(x.ev[4].get(), sh.stream));
  HIPTRY(id_launch_derive(sh.stream, x.keys.get(), x.versions.get(), x.streams.get(), n, x.ident.get()));
  HIPTRY(hipEventRecord(x.ev[5].get(), sh.stream));
  HIPTRY(F::finish(sh.stream, x.rows.get(), d_plain, b.verdict.get(), x.flags.get(), x.ident.get(), n, x.recs.get()));
  HIPTRY(hipEventRecord(x.ev[6].get(), sh.stream));
  return 0;
}

// The six phase times of the last launch_set (its events have completed), added to st.
template <class F, class Stats>
int phase_times(const RowBufs<F>& x, Stats& st) {
  double* const acc[6] = {&st.walk_ms, &st.hash_ms, &st.scalar_ms, &st.curve_ms, &st.ident_ms, &st.finish_ms};
  return elapsed_phases(acc, x.ev, 6);
}

// One call over rows 0 .. n_all (under g_mu).  The rows, sorted by the upper bound of their signed data's
// block count (descending, so a wave's 64 lanes hash alike), go through the device in sets of at most
// kSigSetObjects rows and kSigSetPoolBytes of padded blocks.  Per set the host copies the sources side by side
// into one staging buffer (each at a multiple of 16 bytes) and uploads it with the row descriptors; nothing
// else crosses: launch_set follows, then one download, scattered to out[] by the rows' input index.  The abort
// flag is read between sets.  The buffers are the call's own (DevBuf owners); everything runs on the first
// shard's device and stream.  The policy p supplies, for input row i:
//   p.bound(i)               the blocks to reserve for its signed data
//   p.source(i), p.len(i)    its bytes for the plaintext pool
//   p.fill(row, i)           the family's fields of the row beside poff, plen and blk
//   p.stats                  the counters: calls, sets, launches and the six phase times
template <class F, class Policy>
int run_rows(size_t n_all, const Policy& p, typename F::Rec* out) {
  using Row = typename F::Row;
  using Rec = typename F::Rec;
  struct Item {
    uint32_t orig;
    uint32_t bound;
  };
  std::vector<Item> items(n_all);
  for (size_t i = 0; i < n_all; ++i) items[i] = {(uint32_t)i, p.bound(i)};
  std::stable_sort(items.begin(), items.end(), [](const Item& a, const Item& b) { return a.bound > b.bound; });
  Shard& sh = g_shards[0];
  HIPTRY(hipSetDevice(sh.dev));
  const ec::ge* comb = nullptr;
  if (const int rc = addr_comb16_table(sh, &comb); rc < 0) return rc;
  SigBufs b;
  RowBufs<F> x;
  for (Event& e : x.ev) HIPTRY(e.alloc(sh.dev));
  p.stats.calls++;

  std::vector<Row> rows;
  std::vector<uint8_t> stage;
  std::vector<Rec> recs;
  size_t i0 = 0;
  while (i0 < items.size()) {
    if (g_abort.load()) return set_err(BMPOW_E_ABORTED, "aborted");
    const SetCut cut = plan_set(items, i0, [](const Item& it) { return it.bound; }, kSigSetObjects, kSigSetPoolBytes);
    if (cut.blocks > 0xffffffffull) return set_err(BMPOW_E_ARG, "message pool above 2^32 blocks");
    const uint32_t n = (uint32_t)(cut.i1 - i0), stride = (n + SG_BLOCK - 1) / SG_BLOCK * SG_BLOCK;
    rows.assign(n, Row{});
    uint64_t poff = 0;
    uint32_t blk = 0;
    for (uint32_t j = 0; j < n; ++j) {
      const Item& it = items[i0 + j];
      Row& r = rows[j];
      r.poff = poff;
      r.plen = (uint32_t)p.len(it.orig);
      r.blk = blk;
      p.fill(r, it.orig);
      poff += ((uint64_t)r.plen + 15) & ~15ull;
      blk += it.bound;
    }
    const uint64_t plain_bytes = std::max<uint64_t>(poff, 16);
    stage.resize(plain_bytes);
    bmsched::parallel_for(n, 1024, [&](size_t a, size_t z) {
      for (size_t j = a; j < z; ++j) {
        const Row& r = rows[j];
        uint8_t* dst = stage.data() + r.poff;
        if (r.plen) std::memcpy(dst, p.source(items[i0 + j].orig), r.plen);
        std::memset(dst + r.plen, 0, (size_t)(-(int64_t)r.plen & 15));
      }
    });
    const uint64_t pool_chunks = std::max<uint64_t>(cut.blocks * 4, 4), plain_chunks = plain_bytes / 16;
    if (const int rc = grow_set(sh, b, x, stride, pool_chunks, plain_chunks); rc < 0) return rc;
    HIPTRY(hipMemcpyAsync(x.rows.get(), rows.data(), n * sizeof(Row), hipMemcpyHostToDevice, sh.stream));
    HIPTRY(hipMemcpyAsync(x.plain.get(), stage.data(), plain_bytes, hipMemcpyHostToDevice, sh.stream));
    if (const int rc = launch_set(sh, b, x, comb, n, stride, plain_chunks, pool_chunks); rc < 0) return rc;
    recs.resize(n);
    HIPTRY(hipMemcpyAsync(recs.data(), x.recs.get(), n * sizeof(Rec), hipMemcpyDeviceToHost, sh.stream));
    HIPTRY(hipStreamSynchronize(sh.stream));
    if (const int rc = phase_times(x, p.stats); rc < 0) return rc;
    for (uint32_t j = 0; j < n; ++j) out[items[i0 + j].orig] = recs[j];
    p.stats.sets++;
    p.stats.launches += 9;
    i0 = cut.i1;
  }
  return 0;
}

}  // namespace bmhost
