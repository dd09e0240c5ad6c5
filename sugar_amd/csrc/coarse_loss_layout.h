// coarse_loss_layout.h -- the scratch layouts of csrc/coarse_loss.hip as plain host C++ (no HIP): one place for the size arithmetic,
// so that a stand-alone host program can check it under a sanitizer (tests/host/coarse_loss_layout_main.cpp).
//
//   estimation forward  : partial f64[3][ceil(N / 256)]                       (estimation term | on-surface term | projected count)
//   better-normal fwd   : partial f64[blocks]                                 (blocks = ceil(N / 16) at K = 16, ceil(N / 256) otherwise)
//   better-normal bwd   : keys i64[E] | start u32[P + 1] | rows f32[E][W] | the grouping's scratch for E entries
//                         E = N * (K + 1) entries (the pairs, then each sample's own Gaussian), W = 3 (normals) or 6 (+ points)
//   projection forward  : partial f64[2][ceil(N / 256)]                       (estimation term | on-surface term)
//   projection backward : dest f32[N] | start u32[P + 1] | the grouping's scratch for N entries
// Every part starts 256-byte aligned.
#pragma once
#include <stddef.h>
#include <stdint.h>

static inline size_t cl_align(size_t x) { return (x + 255) / 256 * 256; }
static inline size_t cl_blocks(size_t n, size_t per_block) { return (n + per_block - 1) / per_block; }

static inline size_t cl_estimation_blocks(long long N) { return cl_blocks((size_t)(N > 0 ? N : 0), 256); }
static inline size_t cl_estimation_scratch_bytes(long long N) { return cl_align(3 * cl_estimation_blocks(N) * sizeof(double)); }

// opacity entropy: partial f64[2][ceil(P / 256)]   (the sum of the visible rows' terms | their count)
static inline size_t cl_entropy_scratch_bytes(int P) { return cl_align(2 * cl_blocks((size_t)(P > 0 ? P : 0), 256) * sizeof(double)); }

static inline size_t cl_normal_blocks(long long N, int K) { return cl_blocks((size_t)(N > 0 ? N : 0), K == 16 ? 16 : 256); }
static inline size_t cl_normal_fwd_scratch_bytes(long long N, int K) { return cl_align(cl_normal_blocks(N, K) * sizeof(double)); }

// false when N * (K + 1) does not fit the grouping's 32-bit entry numbers
static inline bool cl_normal_entries(long long N, int K, size_t* entries)
{
    if (N < 0 || K < 1) return false;
    const unsigned long long e = (unsigned long long)N * (unsigned long long)(K + 1);
    if ((unsigned long long)N > 0xFFFFFFFFull || e >= 0x100000000ull) return false;
    *entries = (size_t)e;
    return true;
}

struct ClNormalBwdLayout { size_t keys, start, rows, group, total; };
// group_bytes: sgr_group_scratch_bytes(entries)
static inline ClNormalBwdLayout cl_normal_bwd_layout(size_t entries, int P, int width, size_t group_bytes)
{
    ClNormalBwdLayout L;
    size_t off = 0;
    L.keys = off;  off = cl_align(off + entries * sizeof(int64_t));
    L.start = off; off = cl_align(off + ((size_t)(P > 0 ? P : 0) + 1) * sizeof(uint32_t));
    L.rows = off;  off = cl_align(off + entries * (size_t)width * sizeof(float));
    L.group = off; off = cl_align(off + group_bytes);
    L.total = off;
    return L;
}

static inline size_t cl_projection_fwd_scratch_bytes(long long N) { return cl_align(2 * cl_estimation_blocks(N) * sizeof(double)); }

struct ClProjectionBwdLayout { size_t dest, start, group, total; };
// group_bytes: sgr_group_scratch_bytes(N)
static inline ClProjectionBwdLayout cl_projection_bwd_layout(size_t N, int P, size_t group_bytes)
{
    ClProjectionBwdLayout L;
    size_t off = 0;
    L.dest = off;  off = cl_align(off + N * sizeof(float));
    L.start = off; off = cl_align(off + ((size_t)(P > 0 ? P : 0) + 1) * sizeof(uint32_t));
    L.group = off; off = cl_align(off + group_bytes);
    L.total = off;
    return L;
}
