// sgr_group.h -- the stable grouping of csrc/field.hip (launch_group_by_key: LSD radix sort of M entries by an integer key in
// [-P, P), entries outside left out) for the other translation units that sum per-Gaussian gradients in a fixed order.
//   *list_out = entry numbers, key-major, ascending inside a key; start[0..P] = offsets into it (uint32, P + 1 entries, caller's memory).
//   scratch: sgr_group_scratch_bytes(M) bytes of device memory, 256-byte aligned.  Enqueued on s; no host synchronisation.  M < 2^32.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

size_t sgr_group_scratch_bytes(size_t M);
int sgr_group_by_key(long long M, const long long* keys64, int P, char* scratch, uint32_t* start, const uint32_t** list_out, hipStream_t s);
