// sgr_group.h -- what csrc/group.hip offers the translation units that sum per-Gaussian gradients in a fixed order.
//
// sgr_group_by_key: stable grouping (LSD radix sort) of M entries by an integer key in [-P, P); negative keys wrap once, entries
// outside are left out.
//   *list_out = entry numbers, key-major, ascending inside a key; start[0..P] = offsets into it (uint32, P + 1 entries, caller's memory).
//   scratch: sgr_group_scratch_bytes(M) bytes of device memory, 256-byte aligned.  Enqueued on s; no host synchronisation.  M < 2^32.
//   M <= 0: start is zeroed, *list_out = NULL, the scratch is not touched.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

size_t sgr_group_scratch_bytes(size_t M);
int sgr_group_by_key(long long M, const long long* keys64, int P, char* scratch, uint32_t* start, const uint32_t** list_out, hipStream_t s);

// ---- the SGR_GROUP_ATOMICS=1 variant (same-box A/B): ranks by one returning integer atomic per entry, a scan, a fill ----------------
bool sgr_group_by_atomics();
// exclusive scan of cnt[0..n) into start[0..n], start[n] = total  (n > 0; block_sums: scratch, see SgrRankedScratch)
void sgr_launch_scan(int n, const uint32_t* cnt, uint32_t* block_sums, uint32_t* start, hipStream_t s);
// scratch of an operation that keeps both groupings, for M entries and P groups:
//   cnt u32[P+1] | start u32[P+1] | block sums of the scan | rank u32[M] | list u32[M] | sgr_group_scratch_bytes(M)   (each 256-byte aligned)
struct SgrRankedScratch { uint32_t *cnt, *start, *block_sums, *rank, *list; char* group; size_t total; };
SgrRankedScratch sgr_carve_ranked(char* base, size_t M, int P);
