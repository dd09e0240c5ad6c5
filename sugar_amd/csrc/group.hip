// group.hip -- grouping of entries by a small integer key, for every translation unit that sums per-Gaussian (per-row) gradients in a
// fixed order (declared in sgr_group.h), and the one operation that is nothing but such a grouping: the row scatter.
//
//   scan         : k_fscan_*  exclusive scan of uint32 counts (block sums, scan of the block sums, block-local scans)
//   grouping     : k_grp_*    stable LSD radix sort of the entries by key, 8 bits per pass, ranks formed in LDS; no atomics on global
//                  memory, so the order inside a group -- hence of the float additions that follow -- is the order of the entries
//   row scatter  : k_rows_*   out[p, :] = sum over { n : idx[n] == p } of src[n, :], the backward of a row gather `x[idx]`
//                  (sgr_scatter_add_rows); k_rows_rank / k_rows_fill are the SGR_GROUP_ATOMICS=1 variant of its grouping
#include "../../include/sugar_raster.h"
#include "sgr_device.h"
#include "sgr_group.h"

namespace {

// exclusive scan of cnt[0..n) into start[0..n], start[n] = total: block sums, scan of the block sums, block-local scans
#define FSCAN_BLOCK 2048  // elements per 256-thread workgroup (8 per thread)
__global__ void __launch_bounds__(256) k_fscan_sums(int n, const uint32_t* __restrict__ cnt, uint32_t* __restrict__ block_sums)
{
    __shared__ uint32_t s_w[4];
    const int base = blockIdx.x * FSCAN_BLOCK + threadIdx.x * 8;
    uint32_t sum = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) sum += (base + i < n) ? cnt[base + i] : 0u;
    for (int o = 32; o > 0; o >>= 1) sum += (uint32_t)__shfl_xor((int)sum, o);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) block_sums[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

__global__ void __launch_bounds__(1024) k_fscan_top(int n_blocks, uint32_t* __restrict__ block_sums, uint32_t* __restrict__ total)
{
    __shared__ uint32_t s_part[1024];
    const int tid = threadIdx.x;
    const int per = (n_blocks + 1023) / 1024;
    const int b = tid * per, e = min(n_blocks, b + per);
    uint32_t sum = 0;
    for (int i = b; i < e; i++) sum += block_sums[i];
    s_part[tid] = sum;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const uint32_t v = (tid >= o) ? s_part[tid - o] : 0;
        __syncthreads();
        s_part[tid] += v;
        __syncthreads();
    }
    uint32_t run = s_part[tid] - sum;
    for (int i = b; i < e; i++) { const uint32_t v = block_sums[i]; block_sums[i] = run; run += v; }
    if (tid == 1023) *total = s_part[1023];
}

__global__ void __launch_bounds__(256) k_fscan_apply(int n, const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ block_sums,
                                                     uint32_t* __restrict__ start)
{
    __shared__ uint32_t s_w[4];
    const int base = blockIdx.x * FSCAN_BLOCK + threadIdx.x * 8;
    uint32_t v[8], sum = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) { v[i] = (base + i < n) ? cnt[base + i] : 0u; sum += v[i]; }
    uint32_t run;
    sgr_block_scan<4>(sum, s_w, run);
    run += block_sums[blockIdx.x];
#pragma unroll
    for (int i = 0; i < 8; i++) { if (base + i < n) start[base + i] = run; run += v[i]; }
}

// ---- stable grouping of M entries by a small integer key: LSD radix sort, 8 bits per pass, ranks formed in LDS -----------------------
// Replaces "one returning integer atomic per entry for its rank" (16M of them per call in a trainer's SDF phase: ~20 G atomics/s whatever
// the contention, 0.85 ms) and makes the order of the entries inside a group -- hence of the float additions that follow -- the
// order of the entries themselves: the backward is reproducible run to run.
//   per pass: k_grp_hist (digit counts per chunk of 2048 entries, LDS atomics) -> exclusive scan over [digit][chunk] (k_fscan_*) ->
//             k_grp_scatter (each wave ranks its 64 entries per digit with eight ballots; one leader lane per (unit, digit) publishes
//             the unit's count, thread d scans digit d over the chunk's 32 units (8 rounds x 4 waves), entries go to offset + rank)
//   then    : k_grp_bounds  start[g] = first sorted position whose key is >= g   (binary search; keys past P-1 are the ignored entries)
#define GRP_CHUNK 2048
#define GRP_ROUNDS 8
#define GRP_UNITS (GRP_ROUNDS * 4)

__device__ __forceinline__ uint32_t grp_key64(long long k, int P)  // Python-style wrap once; anything else -> the sentinel P
{
    if (k < 0) k += P;
    return (k >= 0 && k < P) ? (uint32_t)k : (uint32_t)P;
}

template <bool FIRST>
__global__ void __launch_bounds__(256) k_grp_hist(long long M, const long long* __restrict__ keys64, const uint32_t* __restrict__ key_in,
                                                  int P, int shift, uint32_t n_chunks, uint32_t* __restrict__ hist)
{
    __shared__ uint32_t s_h[256];
    const int tid = threadIdx.x;
    s_h[tid] = 0;
    __syncthreads();
    const long long base = (long long)blockIdx.x * GRP_CHUNK;
#pragma unroll
    for (int r = 0; r < GRP_ROUNDS; r++) {
        const long long i = base + r * 256 + tid;
        if (i < M) {
            const uint32_t key = FIRST ? grp_key64(keys64[i], P) : key_in[i];
            atomicAdd(&s_h[(key >> shift) & 255u], 1u);
        }
    }
    __syncthreads();
    hist[(size_t)tid * n_chunks + blockIdx.x] = s_h[tid];
}

template <bool FIRST>
__global__ void __launch_bounds__(256) k_grp_scatter(long long M, const long long* __restrict__ keys64, const uint32_t* __restrict__ key_in,
                                                     const uint32_t* __restrict__ val_in, int P, int shift, uint32_t n_chunks,
                                                     const uint32_t* __restrict__ offs, uint32_t* __restrict__ key_out,
                                                     uint32_t* __restrict__ val_out)
{
    __shared__ uint32_t s_u[GRP_UNITS * 256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < GRP_UNITS * 256; i += 256) s_u[i] = 0;
    __syncthreads();
    const long long base = (long long)blockIdx.x * GRP_CHUNK;
    uint32_t key[GRP_ROUNDS], val[GRP_ROUNDS], rk[GRP_ROUNDS];
#pragma unroll
    for (int r = 0; r < GRP_ROUNDS; r++) {
        const long long i = base + r * 256 + tid;
        const bool valid = i < M;
        key[r] = valid ? (FIRST ? grp_key64(keys64[i], P) : key_in[i]) : 0u;
        val[r] = valid ? (FIRST ? (uint32_t)i : val_in[i]) : 0u;
        const uint32_t d = (key[r] >> shift) & 255u;
        unsigned long long mask = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; b++) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long bb = __ballot(bit);
            mask &= bit ? bb : ~bb;
        }
        const unsigned long long below = mask & ((1ull << lane) - 1ull);
        rk[r] = (uint32_t)__popcll(below);
        if (valid && below == 0ull) s_u[(r * 4 + wave) * 256 + d] = (uint32_t)__popcll(mask);  // the group's first lane publishes its size
    }
    __syncthreads();
    {
        uint32_t run = offs[(size_t)tid * n_chunks + blockIdx.x];
#pragma unroll 8
        for (int u = 0; u < GRP_UNITS; u++) {
            const uint32_t t = s_u[u * 256 + tid];
            s_u[u * 256 + tid] = run;
            run += t;
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < GRP_ROUNDS; r++) {
        const long long i = base + r * 256 + tid;
        if (i < M) {
            const uint32_t d = (key[r] >> shift) & 255u;
            const uint32_t pos = s_u[(r * 4 + wave) * 256 + d] + rk[r];
            key_out[pos] = key[r];
            val_out[pos] = val[r];
        }
    }
}

__global__ void __launch_bounds__(256) k_grp_bounds(int P, long long M, const uint32_t* __restrict__ sorted_keys, uint32_t* __restrict__ start)
{
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g > P) return;
    long long lo = 0, hi = M;   // first position with key >= g
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (sorted_keys[mid] < (uint32_t)g) lo = mid + 1; else hi = mid;
    }
    start[g] = (uint32_t)lo;
}

struct GroupScratch { uint32_t *key_a, *val_a, *key_b, *val_b, *hist, *offs, *block_sums; size_t total; };
GroupScratch carve_group(char* base, size_t M)
{
    GroupScratch g;
    const size_t n_chunks = (M + GRP_CHUNK - 1) / GRP_CHUNK, H = 256 * (n_chunks ? n_chunks : 1);
    size_t off = 0;
    auto take = [&](size_t bytes) { uint32_t* p = reinterpret_cast<uint32_t*>(base + off); off = sgr_align(off + bytes); return p; };
    g.key_a = take(M * 4); g.val_a = take(M * 4); g.key_b = take(M * 4); g.val_b = take(M * 4);
    g.hist = take((H + 1) * 4); g.offs = take((H + 1) * 4); g.block_sums = take(((H + FSCAN_BLOCK - 1) / FSCAN_BLOCK + 2) * 4);
    g.total = off;
    return g;
}

// ---- out[p, :] = sum over { n : idx[n] == p } of src[n, :]  -- the backward of a row gather `x[idx]` --------------------------------
// What autograd runs for every `tensor[index]` of the regulariser (sugar_model.py:922-925: points / quaternions / scaling of 1M sampled
// Gaussians; coarse_sdf.py:690-692: the normals of 1M x 16 neighbours): stock PyTorch sorts the indices and reduces segments, 1.3 ms per
// call on average and six calls per iteration.  Same scheme as the density backward of field.hip: the entries are grouped by row
// (sgr_group_by_key; k_rows_rank / k_rows_fill are the SGR_GROUP_ATOMICS=1 variant), sixteen lanes per row add its entries up.
// Negative indices wrap once (Python semantics); entries outside [-P, P) are ignored.
__global__ void __launch_bounds__(256) k_rows_rank(long long N, const long long* __restrict__ idx, int P, uint32_t* __restrict__ cnt,
                                                   uint32_t* __restrict__ rank)
{
    const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const long long g = wrap_row(idx[n], P);
    if (g >= 0 && g < P) rank[n] = atomicAdd(&cnt[g], 1u);
}

__global__ void __launch_bounds__(256) k_rows_fill(long long N, const long long* __restrict__ idx, int P, const uint32_t* __restrict__ start,
                                                   const uint32_t* __restrict__ rank, uint32_t* __restrict__ list)
{
    const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const long long g = wrap_row(idx[n], P);
    if (g >= 0 && g < P) list[start[g] + rank[n]] = (uint32_t)n;
}

template <int W>
__global__ void __launch_bounds__(256) k_rows_gather(int P, const float* __restrict__ src, const uint32_t* __restrict__ start,
                                                     const uint32_t* __restrict__ list, float* __restrict__ out)
{
    const int t = (int)(((size_t)blockIdx.x * 256 + threadIdx.x) >> 4);
    const uint32_t sub = threadIdx.x & 15;
    if (t >= P) return;
    float acc[W];
#pragma unroll
    for (int c = 0; c < W; c++) acc[c] = 0.f;
    const uint32_t e0 = start[t], e1 = start[t + 1];
    for (uint32_t e = e0 + sub; e < e1; e += 16) {
        const float* r = src + (size_t)list[e] * W;
#pragma unroll
        for (int c = 0; c < W; c++) acc[c] += r[c];
    }
#pragma unroll
    for (int c = 0; c < W; c++) acc[c] = row_sum16(acc[c]);
    if (sub < (uint32_t)W) {
        float v = acc[0];
#pragma unroll
        for (int c = 1; c < W; c++) v = (sub == (uint32_t)c) ? acc[c] : v;
        out[(size_t)t * W + sub] = v;
    }
}

}  // namespace

void sgr_launch_scan(int n, const uint32_t* cnt, uint32_t* block_sums, uint32_t* start, hipStream_t s)
{
    const int n_blocks = (n + FSCAN_BLOCK - 1) / FSCAN_BLOCK;
    hipLaunchKernelGGL(k_fscan_sums, dim3(n_blocks), dim3(256), 0, s, n, cnt, block_sums);
    hipLaunchKernelGGL(k_fscan_top, dim3(1), dim3(1024), 0, s, n_blocks, block_sums, start + n);
    hipLaunchKernelGGL(k_fscan_apply, dim3(n_blocks), dim3(256), 0, s, n, cnt, block_sums, start);
}

size_t sgr_group_scratch_bytes(size_t M) { return carve_group(nullptr, M).total; }

int sgr_group_by_key(long long M, const long long* keys64, int P, char* scratch, uint32_t* start, const uint32_t** list_out, hipStream_t s)
{
    if (M <= 0) {   // nothing to group: every group is empty
        *list_out = nullptr;
        return hipMemsetAsync(start, 0, ((size_t)P + 1) * 4, s) == hipSuccess ? 0 : SGR_E_HIP;
    }
    const GroupScratch g = carve_group(scratch, (size_t)M);
    const uint32_t n_chunks = (uint32_t)(((size_t)M + GRP_CHUNK - 1) / GRP_CHUNK);
    const size_t H = 256 * (size_t)n_chunks;
    int bits = 0;
    while (bits < 32 && ((unsigned long long)P >> bits) != 0ull) bits++;   // P itself (the sentinel) must fit
    const int passes = (bits + 7) / 8 > 0 ? (bits + 7) / 8 : 1;
    uint32_t *kin = nullptr, *vin = nullptr, *kout = g.key_a, *vout = g.val_a;
    for (int pass = 0; pass < passes; pass++) {
        const int shift = 8 * pass;
        if (pass == 0) hipLaunchKernelGGL(k_grp_hist<true>, dim3(n_chunks), dim3(256), 0, s, M, keys64, kin, P, shift, n_chunks, g.hist);
        else hipLaunchKernelGGL(k_grp_hist<false>, dim3(n_chunks), dim3(256), 0, s, M, keys64, kin, P, shift, n_chunks, g.hist);
        sgr_launch_scan((int)H, g.hist, g.block_sums, g.offs, s);
        if (pass == 0) hipLaunchKernelGGL(k_grp_scatter<true>, dim3(n_chunks), dim3(256), 0, s, M, keys64, kin, vin, P, shift, n_chunks, g.offs, kout, vout);
        else hipLaunchKernelGGL(k_grp_scatter<false>, dim3(n_chunks), dim3(256), 0, s, M, keys64, kin, vin, P, shift, n_chunks, g.offs, kout, vout);
        kin = kout; vin = vout;
        kout = (kin == g.key_a) ? g.key_b : g.key_a;
        vout = (vin == g.val_a) ? g.val_b : g.val_a;
    }
    hipLaunchKernelGGL(k_grp_bounds, dim3((unsigned)((P + 1 + 255) / 256)), dim3(256), 0, s, P, M, kin, start);
    *list_out = vin;
    return sgr_launch_status();
}

bool sgr_group_by_atomics()
{
    static const bool v = [] { const char* e = getenv("SGR_GROUP_ATOMICS"); return e && e[0] == '1'; }();
    return v;
}

SgrRankedScratch sgr_carve_ranked(char* base, size_t M, int P)
{
    SgrRankedScratch r;
    const size_t p = (size_t)(P > 0 ? P : 0);
    size_t off = 0;
    auto take = [&](size_t bytes) { uint32_t* q = reinterpret_cast<uint32_t*>(base + off); off += sgr_align(bytes); return q; };
    r.cnt = take((p + 1) * 4); r.start = take((p + 1) * 4);
    r.block_sums = take(((p + FSCAN_BLOCK - 1) / FSCAN_BLOCK + 1) * 4);
    r.rank = take(M * 4); r.list = take(M * 4);
    r.group = base + off;
    r.total = off + carve_group(nullptr, M).total;
    return r;
}

extern "C" {

size_t sgr_scatter_add_rows_scratch_bytes(long long N, int P) { return sgr_carve_ranked(nullptr, (size_t)(N > 0 ? N : 0), P).total; }

int sgr_scatter_add_rows(long long N, const int64_t* idx, const float* src, int W, int P, float* out, char* scratch, void* stream)
{
    if (P <= 0) return 0;
    if (N < 0 || W < 1 || W > 4 || (N > 0 && (!idx || !src)) || !out || !scratch || (unsigned long long)N > 0xFFFFFFFFull)
        return SGR_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const SgrRankedScratch sc = sgr_carve_ranked(scratch, (size_t)N, P);
    const long long* ix = reinterpret_cast<const long long*>(idx);
    const uint32_t* entries = sc.list;
    if (sgr_group_by_atomics() || N == 0) {
        if (hipMemsetAsync(sc.cnt, 0, ((size_t)P + 1) * 4, s) != hipSuccess) return SGR_E_HIP;
        const unsigned nb = (unsigned)(((size_t)N + 255) / 256);
        if (N > 0) hipLaunchKernelGGL(k_rows_rank, dim3(nb), dim3(256), 0, s, N, ix, P, sc.cnt, sc.rank);
        sgr_launch_scan(P, sc.cnt, sc.block_sums, sc.start, s);
        if (N > 0) hipLaunchKernelGGL(k_rows_fill, dim3(nb), dim3(256), 0, s, N, ix, P, sc.start, sc.rank, sc.list);
    } else {
        const int rc = sgr_group_by_key(N, ix, P, sc.group, sc.start, &entries, s);
        if (rc < 0) return rc;
    }
    const unsigned gb = blocks256((size_t)P * 16);
    switch (W) {
        case 1: hipLaunchKernelGGL(k_rows_gather<1>, dim3(gb), dim3(256), 0, s, P, src, sc.start, entries, out); break;
        case 2: hipLaunchKernelGGL(k_rows_gather<2>, dim3(gb), dim3(256), 0, s, P, src, sc.start, entries, out); break;
        case 3: hipLaunchKernelGGL(k_rows_gather<3>, dim3(gb), dim3(256), 0, s, P, src, sc.start, entries, out); break;
        default: hipLaunchKernelGGL(k_rows_gather<4>, dim3(gb), dim3(256), 0, s, P, src, sc.start, entries, out); break;
    }
    return sgr_launch_status();
}

}  // extern "C"
