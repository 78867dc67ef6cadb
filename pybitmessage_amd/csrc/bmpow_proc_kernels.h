// bmpow_proc_kernels.h -- launch wrappers of the object-processor dispatch kernels (bmpow_proc.hip), used by
// bmpow_host_proc.hip.  Tables and rows as bmpow_proc_fmt.h lays them out.  Every wrapper checks its pointers and
// launches nothing for an empty range.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bmpow_proc_fmt.h"

// One device row: `avail` uploaded bytes at byte offset off of the call's pool, of an object (or, for an ack
// candidate, a tail) of len bytes.
#define PC_ROW_ACK 0u
#define PC_ROW_GETPUBKEY 1u
#define PC_ROW_ONION 2u
struct pc_row {
  uint32_t off, avail, len, kind;
};

// What the finish kernel writes per ack row.
struct pc_ack {
  uint32_t state, aux, first;
};

struct pc_call {
  const uint64_t* pool;  // the call's uploaded bytes, back to back
  uint64_t pool_bytes;
  const pc_row* rows;    // [n_rows]: the ack rows first, in input order, then getpubkeys, then onionpeers
  uint32_t n_rows, n_ack;
  pcf::WatchTable watch;
  pcf::AddrTable addrs;
  int64_t now;
  uint32_t* first;       // [watch.n]: the lowest ack row that carries the entry's key (PC_NONE before the call)
  uint32_t* ack_entry;   // [n_ack]: the entry an ack row's tail equals, PC_NONE where none
  pc_rec* recs;          // [n_rows - n_ack]: the record of row n_ack + j
};

// Rows [begin, end): an ack row probes the watch index and takes the minimum of its row number into
// first[entry]; a getpubkey or onionpeer row writes its record.
hipError_t pc_launch_rows(hipStream_t st, const pc_call& c, uint32_t begin, uint32_t end);
// After the call's last rows launch: out[i] = FOUND where first[ack_entry[i]] == i, else FOUND_EARLIER with
// first; NOT_WATCHED where ack_entry[i] is PC_NONE.
hipError_t pc_launch_ack_finish(hipStream_t st, const pc_call& c, pc_ack* out);
