// bmpow_inv_kernels.h -- launch wrappers of the inventory-set kernels (bmpow_inv.hip), used by
// bmpow_host_inv.hip.  Tables and rows as bmpow_inv_fmt.h lays them out.  Every wrapper checks its pointers and
// launches nothing for n == 0.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bmpow_inv_fmt.h"

// The words every launch adds to (zeroed by the host before a call's first launch).
enum {
  IV_CTR_PROBES = 0,  // slots looked at, all rows
  IV_CTR_LONGEST,     // the longest probe of one row
  IV_CTR_BAD,         // != 0: a probe loop ran out, or a lookup met a pending word
  IV_CTR_ADDED,       // slots finalize made full
  IV_CTR_REMOVED,     // slots the tombstone launch found full
  IV_CTR_KEPT,        // entries the rebuild carried over
  IV_CTR_LISTED,      // entries the list kernel matched (may exceed its cap)
  IV_CTR_WORDS = 8
};

// Row flags (flags null: every row takes part).
#define IV_ROW_LOOKUP 1u  // the lookup launch looks the row up
#define IV_ROW_ADD 2u     // the claim / finalize launches insert the row

// slot_out[i] = the slot holding row i's key, IV_NONE where absent or where the row lacks `need` in flags;
// val_out (may be null) the slot's value, zeros where absent.
hipError_t iv_launch_lookup(hipStream_t st, ivf::Table t, ivf::Rows rows, const uint8_t* flags, uint32_t need,
                            uint32_t* slot_out, iv_val* val_out, uint64_t* ctr);
// claim[i] / slot[i] as ivf::claim gives them for the rows with IV_ROW_ADD whose skip[i] (may be null: another
// set's lookup) is IV_NONE; IV_NONE for the others.  first[] was set to IV_NONE before the launch.
hipError_t iv_launch_claim(hipStream_t st, ivf::Table t, ivf::Rows rows, const uint8_t* flags, const uint32_t* skip,
                           uint32_t* first, uint32_t* claim, uint32_t* slot, uint64_t* ctr);
// Behind the claim: the claimants write key, value and the full word; state_out[i] = BMPOW_INV_PRESENT / ADDED /
// DUP (ABSENT for a row that took no part), first_out[i] = the lowest row carrying row i's key (i for PRESENT).
// expires / stream / aux may each be null: then expires_all, 0 and 0.
hipError_t iv_launch_finalize(hipStream_t st, ivf::Table t, ivf::Rows rows, const uint32_t* first, const uint32_t* claim,
                              const uint32_t* slot, const uint64_t* expires, uint64_t expires_all, const uint32_t* stream,
                              const uint32_t* aux, uint8_t* state_out, uint32_t* first_out, uint64_t* ctr);
// The tombstone into every slot[i] != IV_NONE (slots a lookup launch found).
hipError_t iv_launch_bury(hipStream_t st, ivf::Table t, const uint32_t* slot, uint32_t n, uint64_t* ctr);
// Every full entry of `from` with expires >= min_expires into `to` (fresh: every state word empty).
hipError_t iv_launch_rebuild(hipStream_t st, ivf::Table from, ivf::Table to, uint64_t min_expires, uint64_t* ctr);
// Every full entry with stream == s and expires > now: its key appended to out[32 x cap] through ctr[IV_CTR_LISTED].
hipError_t iv_launch_list(hipStream_t st, ivf::Table t, uint32_t s, uint64_t now, uint8_t* out, uint64_t cap, uint64_t* ctr);
