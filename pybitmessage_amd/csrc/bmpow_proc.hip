// bmpow_proc.hip -- object-processor dispatch kernels (gfx950): checkackdata against the uploaded watch set,
// processgetpubkey against my addresses, processonion's walk and IP class (include/bmpow_proc.h).
//
// Reference: objectProcessor.run and its three handlers (src/class_objectProcessor.py:64-268),
// protocol.checkIPAddress (src/protocol.py:150-227).  Host side: bmpow_host_proc.hip; every byte-level step is
// bmpow_proc_fmt.h's, the text the host walk and the stand-alone test run.
//
//   proc_rows_kernel       : one lane per device row.  The host grouped the rows by class, so a wave is all ack
//                            candidates, all getpubkeys or all onionpeers (but for the two waves at the seams).
//   proc_ack_finish_kernel : one lane per ack row, after the call's last rows launch.
//
// The tables are read-only here: the host built and uploaded them.  The one word shared inside a launch is
// first[entry], through a relaxed agent-scope atomic minimum; it is read by the finish kernel, a later launch.
// Nothing waits on another thread; every probe ends after at most `slots` steps.  Every index is checked against
// its array's size before it is used, every byte is read through ivf::load_word, which never touches a byte at
// or past the pool's end, and lanes past the range do nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bmpow_proc_kernels.h"

using namespace pcf;

namespace {

constexpr uint32_t kBlock = 256;

__global__ __launch_bounds__(kBlock) void proc_rows_kernel(pc_call c, uint32_t begin, uint32_t end) {
  const uint32_t i = begin + blockIdx.x * kBlock + threadIdx.x;
  if (i >= end || i >= c.n_rows) return;
  const pc_row row = c.rows[i];
  if ((uint64_t)row.off + row.avail > c.pool_bytes) return;  // never: the host planned every row inside the pool
  if (i < c.n_ack) {
    uint32_t e = PC_NONE;
    if (row.kind == PC_ROW_ACK && row.avail == row.len) e = watch_find(c.watch, c.pool, c.pool_bytes, row.off, row.len);
    c.ack_entry[i] = e;
    if (e < c.watch.n) ivf::min_u32(c.first + e, i);
    return;
  }
  pc_rec r{};
  r.address = PC_NONE;
  const Bytes b{c.pool, c.pool_bytes, row.off, row.avail, row.len};
  if (row.kind == PC_ROW_GETPUBKEY) walk_getpubkey(b, c.addrs, c.now, &r);
  else if (row.kind == PC_ROW_ONION) walk_onion(b, &r);
  c.recs[i - c.n_ack] = r;
}

__global__ __launch_bounds__(kBlock) void proc_ack_finish_kernel(pc_call c, pc_ack* __restrict__ out) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= c.n_ack) return;
  pc_ack a{PC_ACK_NOT_WATCHED, 0, PC_NONE};
  const uint32_t e = c.ack_entry[i];
  if (e < c.watch.n) {
    uint32_t f = c.first[e];
    if (f >= c.n_ack) f = i;  // never: row i itself put its number there
    a.state = f == i ? PC_ACK_FOUND : PC_ACK_FOUND_EARLIER;
    a.aux = c.watch.entries[e].aux;
    a.first = f;
  }
  out[i] = a;
}

bool call_ok(const pc_call& c) {
  if (!c.rows || c.n_ack > c.n_rows || (c.pool_bytes && !c.pool)) return false;
  if (c.n_ack && !c.ack_entry) return false;
  if (c.n_rows > c.n_ack && !c.recs) return false;
  const WatchTable& w = c.watch;
  if (w.n && (!w.tags || !w.slot_entry || !w.entries || !w.pool || !c.first || w.log2 < 3 || w.log2 > 31)) return false;
  const AddrTable& a = c.addrs;
  if (a.n && (!a.rows || !a.by_ripe || !a.by_tag || a.log2 < 1 || a.log2 > 31)) return false;
  return true;
}

}  // namespace

// ---------------------------------------------------------------------------------------
// Launch wrappers (C++ linkage, used by bmpow_host_proc.hip).
// ---------------------------------------------------------------------------------------
hipError_t pc_launch_rows(hipStream_t st, const pc_call& c, uint32_t begin, uint32_t end) {
  if (begin >= end) return hipSuccess;
  if (!call_ok(c) || end > c.n_rows) return hipErrorInvalidValue;
  hipLaunchKernelGGL(proc_rows_kernel, dim3((end - begin + kBlock - 1) / kBlock), dim3(kBlock), 0, st, c, begin, end);
  return hipGetLastError();
}

hipError_t pc_launch_ack_finish(hipStream_t st, const pc_call& c, pc_ack* out) {
  if (c.n_ack == 0) return hipSuccess;
  if (!call_ok(c) || !out) return hipErrorInvalidValue;
  hipLaunchKernelGGL(proc_ack_finish_kernel, dim3((c.n_ack + kBlock - 1) / kBlock), dim3(kBlock), 0, st, c, out);
  return hipGetLastError();
}
