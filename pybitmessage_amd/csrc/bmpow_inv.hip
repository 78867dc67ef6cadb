// bmpow_inv.hip -- inventory-set kernels (gfx950): an open-addressing table of 32-byte keys on the device
// (include/bmpow_inv.h), linear probing from a seeded start slot over a power-of-two slot count.
//
// Reference: `inventoryHash in Inventory()` / `Inventory()[hash] = ...` of BMObject.checkAlreadyHave and
// bm_command_object (src/network/bmproto.py:393-435), `i in Inventory()` and handleReceivedInventory of
// _command_inv (:344-367, src/network/objectracker.py:88-99).  Host side: bmpow_host_inv.hip; the slot steps
// themselves are bmpow_inv_fmt.h's, the text the host test runs.
//
//   iv_lookup_kernel   : one lane per row, the probe over resident keys; changes nothing.
//   iv_claim_kernel    : one lane per row; empty -> pending + row by a 64-bit compare-and-swap, equal keys of the
//                        call meeting at the claimant's row through atomicMin into first[].
//   iv_finalize_kernel : the launch behind it; the claimants write key, value and the full word, every row
//                        reads its answer.
//   iv_bury_kernel     : the tombstones behind a lookup launch.
//   iv_rebuild_kernel  : one lane per old slot, empty -> full in a fresh table (grow, purge, sweep).
//   iv_list_kernel     : one lane per slot, the matching keys appended through one counter add per wave.
//
// No thread reads a key or value byte that another thread wrote in the same launch: claim compares against
// resident keys (earlier launches) and against the call's read-only input rows, and what finalize and rebuild
// write is first read by a later launch.  The state words are the only words shared inside a launch, all through
// relaxed agent-scope 64-bit atomics; nothing waits on another thread, and every probe loop ends after at most
// `slots` steps.  Every index is checked against its array's size before it is used; lanes past n do nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bmpow_inv.h"
#include "bmpow_inv_kernels.h"

using namespace ivf;

namespace {

constexpr uint32_t kBlock = 256;

// The wave's probe counts into the call's counters: one add and one max per wave.  Every lane of the wave calls it.
__device__ __forceinline__ void tally(uint64_t* ctr, uint32_t probes, bool bad) {
  unsigned long long sum = probes;
  uint32_t longest = probes;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sum += __shfl_xor(sum, o);
    const uint32_t other = __shfl_xor(longest, o);
    longest = other > longest ? other : longest;
  }
  const bool any_bad = __any(bad ? 1 : 0) != 0;
  if ((threadIdx.x & 63u) == 0) {
    if (sum) atomicAdd(reinterpret_cast<unsigned long long*>(ctr + IV_CTR_PROBES), sum);
    if (longest) atomicMax(reinterpret_cast<unsigned long long*>(ctr + IV_CTR_LONGEST), (unsigned long long)longest);
    if (any_bad) atomicOr(reinterpret_cast<unsigned long long*>(ctr + IV_CTR_BAD), 1ull);
  }
}

// a count of lanes into ctr[which]: one add per wave
__device__ __forceinline__ void tally_count(uint64_t* ctr, int which, bool hit) {
  const unsigned long long m = __ballot(hit ? 1 : 0);
  if (m && (threadIdx.x & 63u) == (uint32_t)(__ffsll((long long)m) - 1))
    atomicAdd(reinterpret_cast<unsigned long long*>(ctr + which), (unsigned long long)__popcll(m));
}

__global__ __launch_bounds__(kBlock) void iv_lookup_kernel(Table t, Rows rows, const uint8_t* __restrict__ flags,
                                                           uint32_t need, uint32_t* __restrict__ slot_out,
                                                           iv_val* __restrict__ val_out, uint64_t* ctr) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  uint32_t probes = 0;
  bool bad = false;
  if (i < rows.n) {
    uint32_t s = IV_NONE;
    uint64_t k[4];
    if ((!flags || (flags[i] & need)) && row_key(rows, i, k)) s = lookup(t, k, &probes, &bad);
    slot_out[i] = s;
    if (val_out) val_out[i] = s != IV_NONE ? t.vals[s] : iv_val{0, 0, 0};
  }
  tally(ctr, probes, bad);
}

__global__ __launch_bounds__(kBlock) void iv_claim_kernel(Table t, Rows rows, const uint8_t* __restrict__ flags,
                                                          const uint32_t* __restrict__ skip, uint32_t* first,
                                                          uint32_t* __restrict__ claim_out, uint32_t* __restrict__ slot_out,
                                                          uint64_t* ctr) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  uint32_t probes = 0;
  bool bad = false;
  if (i < rows.n) {
    uint32_t c = IV_NONE, s = IV_NONE;
    uint64_t k[4];
    if ((!flags || (flags[i] & IV_ROW_ADD)) && (!skip || skip[i] == IV_NONE) && row_key(rows, i, k))
      c = claim(t, rows, i, k, first, &s, &probes, &bad);
    claim_out[i] = c;
    slot_out[i] = s;
  }
  tally(ctr, probes, bad);
}

__global__ __launch_bounds__(kBlock) void iv_finalize_kernel(Table t, Rows rows, const uint32_t* __restrict__ first,
                                                             const uint32_t* __restrict__ claim_in,
                                                             const uint32_t* __restrict__ slot_in,
                                                             const uint64_t* __restrict__ expires, uint64_t expires_all,
                                                             const uint32_t* __restrict__ stream,
                                                             const uint32_t* __restrict__ aux, uint8_t* __restrict__ state_out,
                                                             uint32_t* __restrict__ first_out, uint64_t* ctr) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  bool added = false;
  if (i < rows.n) {
    const uint32_t c = claim_in[i];
    uint8_t state = BMPOW_INV_ABSENT;
    uint32_t f = IV_NONE;
    if (c == IV_PRESENT) {
      state = BMPOW_INV_PRESENT, f = i;
    } else if (c < rows.n) {
      f = first[c];  // the claim launch's minimum over every row that carries this key
      if (f >= rows.n) f = i;  // never: row c itself put its index there
      state = f == i ? BMPOW_INV_ADDED : BMPOW_INV_DUP;
      const uint32_t s = slot_in[i];
      uint64_t k[4];
      if (c == i && s < slots_of(t) && row_key(rows, i, k)) {
        const iv_val v{expires ? expires[f] : expires_all, stream ? stream[f] : 0u, aux ? aux[f] : 0u};
        finalize_slot(t, s, k, v);
        added = true;
      }
    }
    state_out[i] = state;
    first_out[i] = f;
  }
  tally_count(ctr, IV_CTR_ADDED, added);
}

__global__ __launch_bounds__(kBlock) void iv_bury_kernel(Table t, const uint32_t* __restrict__ slot, uint32_t n,
                                                         uint64_t* ctr) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  bool removed = false;
  if (i < n) {
    const uint32_t s = slot[i];
    if (s < slots_of(t)) removed = bury(t, s);
  }
  tally_count(ctr, IV_CTR_REMOVED, removed);
}

__global__ __launch_bounds__(kBlock) void iv_rebuild_kernel(Table from, Table to, uint64_t min_expires, uint64_t* ctr) {
  const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
  uint32_t probes = 0;
  bool bad = false, kept = false;
  if (s < slots_of(from) && is_full(from.state[s])) {
    const iv_val v = from.vals[s];
    if (v.expires >= min_expires) {
      const uint64_t* r = from.keys + 4ull * s;
      const uint64_t k[4] = {r[0], r[1], r[2], r[3]};
      kept = reinsert(to, k, v, &probes);
      bad = !kept;
    }
  }
  tally(ctr, probes, bad);
  tally_count(ctr, IV_CTR_KEPT, kept);
}

__global__ __launch_bounds__(kBlock) void iv_list_kernel(Table t, uint32_t stream, uint64_t now, uint8_t* __restrict__ out,
                                                         uint64_t cap, uint64_t* ctr) {
  const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
  bool hit = false;
  if (s < slots_of(t) && is_full(t.state[s])) {
    const iv_val v = t.vals[s];
    hit = v.stream == stream && v.expires > now;
  }
  const unsigned long long m = __ballot(hit ? 1 : 0);
  if (m == 0) return;  // the whole wave
  const uint32_t lane = threadIdx.x & 63u, leader = (uint32_t)(__ffsll((long long)m) - 1);
  unsigned long long base = 0;
  if (lane == leader)
    base = atomicAdd(reinterpret_cast<unsigned long long*>(ctr + IV_CTR_LISTED), (unsigned long long)__popcll(m));
  base = __shfl(base, (int)leader);
  const uint64_t at = base + (uint64_t)__popcll(m & ((1ull << lane) - 1ull));
  if (hit && at < cap) {
    const uint64_t* r = t.keys + 4ull * s;
    uint64_t* o = reinterpret_cast<uint64_t*>(out) + 4 * at;
    for (int q = 0; q < 4; ++q) o[q] = r[q];
  }
}

bool table_ok(const Table& t) { return t.state && t.keys && t.vals && t.log2 >= 1 && t.log2 <= 31; }
bool rows_ok(const Rows& r) { return r.buf && (r.offs || 32ull * r.n <= r.nbytes); }
dim3 grid_for(uint32_t n) { return dim3((n + kBlock - 1) / kBlock); }

}  // namespace

// ---------------------------------------------------------------------------------------
// Launch wrappers (C++ linkage, used by bmpow_host_inv.hip).
// ---------------------------------------------------------------------------------------
hipError_t iv_launch_lookup(hipStream_t st, Table t, Rows rows, const uint8_t* flags, uint32_t need, uint32_t* slot_out,
                            iv_val* val_out, uint64_t* ctr) {
  if (rows.n == 0) return hipSuccess;
  if (!table_ok(t) || !rows_ok(rows) || !slot_out || !ctr) return hipErrorInvalidValue;
  hipLaunchKernelGGL(iv_lookup_kernel, grid_for(rows.n), dim3(kBlock), 0, st, t, rows, flags, need, slot_out, val_out, ctr);
  return hipGetLastError();
}

hipError_t iv_launch_claim(hipStream_t st, Table t, Rows rows, const uint8_t* flags, const uint32_t* skip, uint32_t* first,
                           uint32_t* claim, uint32_t* slot, uint64_t* ctr) {
  if (rows.n == 0) return hipSuccess;
  if (!table_ok(t) || !rows_ok(rows) || !first || !claim || !slot || !ctr) return hipErrorInvalidValue;
  hipLaunchKernelGGL(iv_claim_kernel, grid_for(rows.n), dim3(kBlock), 0, st, t, rows, flags, skip, first, claim, slot, ctr);
  return hipGetLastError();
}

hipError_t iv_launch_finalize(hipStream_t st, Table t, Rows rows, const uint32_t* first, const uint32_t* claim,
                              const uint32_t* slot, const uint64_t* expires, uint64_t expires_all, const uint32_t* stream,
                              const uint32_t* aux, uint8_t* state_out, uint32_t* first_out, uint64_t* ctr) {
  if (rows.n == 0) return hipSuccess;
  if (!table_ok(t) || !rows_ok(rows) || !first || !claim || !slot || !state_out || !first_out || !ctr)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(iv_finalize_kernel, grid_for(rows.n), dim3(kBlock), 0, st, t, rows, first, claim, slot, expires,
                     expires_all, stream, aux, state_out, first_out, ctr);
  return hipGetLastError();
}

hipError_t iv_launch_bury(hipStream_t st, Table t, const uint32_t* slot, uint32_t n, uint64_t* ctr) {
  if (n == 0) return hipSuccess;
  if (!table_ok(t) || !slot || !ctr) return hipErrorInvalidValue;
  hipLaunchKernelGGL(iv_bury_kernel, grid_for(n), dim3(kBlock), 0, st, t, slot, n, ctr);
  return hipGetLastError();
}

hipError_t iv_launch_rebuild(hipStream_t st, Table from, Table to, uint64_t min_expires, uint64_t* ctr) {
  if (!table_ok(from) || !table_ok(to) || !ctr || from.state == to.state) return hipErrorInvalidValue;
  hipLaunchKernelGGL(iv_rebuild_kernel, grid_for(slots_of(from)), dim3(kBlock), 0, st, from, to, min_expires, ctr);
  return hipGetLastError();
}

hipError_t iv_launch_list(hipStream_t st, Table t, uint32_t s, uint64_t now, uint8_t* out, uint64_t cap, uint64_t* ctr) {
  if (!table_ok(t) || !ctr || (cap && !out)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(iv_list_kernel, grid_for(slots_of(t)), dim3(kBlock), 0, st, t, s, now, out, cap, ctr);
  return hipGetLastError();
}
