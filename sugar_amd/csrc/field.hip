// field.hip -- SuGaR's Gaussian density field and level-set surface sampler as fused gfx950 kernels that read the same
// per-Gaussian buffers as the reference's PyTorch code (centres, inverse-scaled rotations, strengths, k-NN indices).
//
//   density field : sugar_scene/sugar_model.py:1270-1281 (get_field_values) and :1998-2009 (the sampler's copy):
//                     w = B_g^T (x - mu_g);  o_g = f * strength_g * exp(-0.5 * clamp(|w|^2, 0, 1e8));  density = sum_g o_g
//                   with B_g = R_g diag(1 / max(s_g, 1e-8))  (get_covariance(return_full_matrix, return_sqrt, inverse_scales),
//                   :730-736).  The reference materialises [N,16,3,3] and [N,16,3,1] temporaries per call; here one lane
//                   owns one sample and walks its 16 neighbours.
//   backward      : gradients of sum(g_op * o) + sum(g_den * density) w.r.t. x, mu, B, strength (autograd of the above).
//   level sets    : sugar_scene/sugar_model.py:1971-2079 (compute_level_surface_points_from_camera_fast): 21 samples along
//                   the pixel's ray in +-3 sigma of the front Gaussian, density at each (normalised where >= 1), first
//                   crossing per level with linear interpolation, normal = -normalize(grad density) at the crossing.
//                   One lane per pixel; a_g = B_g^T (p - mu_g) and b_g = B_g^T dir are formed once per neighbour, so a
//                   sample costs 3 FMAs + |.|^2 + one exp per neighbour instead of a 3x3 product.
#include "../../include/sugar_raster.h"
#include "sgr_device.h"
#include "sgr_group.h"

namespace {

struct GaussNbr {
    float mx, my, mz;
    float B[9];  // row-major 3x3: B[3*i + j]
    float s;
};

// `packed` (optional): one 64-byte record per Gaussian {mu.xyz, strength, B[0..8], pad} written by k_pack_gaussians -- four
// 16-byte loads from one cache line instead of thirteen scalar loads from three arrays.
__device__ __forceinline__ GaussNbr load_nbr(long long g, const float* __restrict__ centers, const float* __restrict__ B,
                                             const float* __restrict__ strengths, const float4* __restrict__ packed = nullptr)
{
    GaussNbr n;
    if (packed) {
        const float4* r = packed + 4 * g;
        const float4 r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3];
        n.mx = r0.x; n.my = r0.y; n.mz = r0.z; n.s = r0.w;
        n.B[0] = r1.x; n.B[1] = r1.y; n.B[2] = r1.z; n.B[3] = r1.w;
        n.B[4] = r2.x; n.B[5] = r2.y; n.B[6] = r2.z; n.B[7] = r2.w; n.B[8] = r3.x;
        return n;
    }
    n.mx = centers[3 * g]; n.my = centers[3 * g + 1]; n.mz = centers[3 * g + 2];
#pragma unroll
    for (int i = 0; i < 9; i++) n.B[i] = B[9 * g + i];
    n.s = strengths[g];
    return n;
}

__global__ void __launch_bounds__(256) k_pack_gaussians(int P, const float* __restrict__ centers, const float* __restrict__ B,
                                                        const float* __restrict__ strengths, float4* __restrict__ packed)
{
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= P) return;
    const GaussNbr n = load_nbr(g, centers, B, strengths);
    float4* r = packed + 4 * (size_t)g;
    r[0] = make_float4(n.mx, n.my, n.mz, n.s);
    r[1] = make_float4(n.B[0], n.B[1], n.B[2], n.B[3]);
    r[2] = make_float4(n.B[4], n.B[5], n.B[6], n.B[7]);
    r[3] = make_float4(n.B[8], 0.f, 0.f, 0.f);
}

// w = B^T d  (w_j = sum_i B[i][j] d_i)
__device__ __forceinline__ void bt_mul(const float* Bm, float dx, float dy, float dz, float& w0, float& w1, float& w2)
{
    w0 = Bm[0] * dx + Bm[3] * dy + Bm[6] * dz;
    w1 = Bm[1] * dx + Bm[4] * dy + Bm[7] * dz;
    w2 = Bm[2] * dx + Bm[5] * dy + Bm[8] * dz;
}

// sum over the 16 lanes of a DPP row, returned to every lane of the row (row_ror:8 / 4 / 2 / 1 fold into the adds)
__device__ __forceinline__ float row_sum16(float x)
{
    x += __uint_as_float((uint32_t)__builtin_amdgcn_update_dpp(0, (int)__float_as_uint(x), 0x128, 0xF, 0xF, false));
    x += __uint_as_float((uint32_t)__builtin_amdgcn_update_dpp(0, (int)__float_as_uint(x), 0x124, 0xF, 0xF, false));
    x += __uint_as_float((uint32_t)__builtin_amdgcn_update_dpp(0, (int)__float_as_uint(x), 0x122, 0xF, 0xF, false));
    x += __uint_as_float((uint32_t)__builtin_amdgcn_update_dpp(0, (int)__float_as_uint(x), 0x121, 0xF, 0xF, false));
    return x;
}

// K == 16 (SuGaR's neighbour count): a lane per (sample, neighbour) PAIR, the sixteen pairs of a sample in one DPP row.  The
// lane-per-sample loops below issue their sixteen record gathers one after the other (each waits for its index): 0.54 ms for 16M pairs
// against records that fit the L2; with a lane per pair all gathers of a wave are in flight at once.
__global__ void __launch_bounds__(256) k_density_fwd16(long long NK, const float* __restrict__ x, const long long* __restrict__ nbr,
                                                       const float* __restrict__ centers, const float* __restrict__ B,
                                                       const float* __restrict__ strengths, const float4* __restrict__ packed, float factor,
                                                       float* __restrict__ opac, float* __restrict__ density)
{
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= NK) return;   // (NK is a multiple of 16: rows leave whole)
    const size_t n = (size_t)(p >> 4);
    const GaussNbr g = load_nbr(nbr[p], centers, B, strengths, packed);
    float w0, w1, w2;
    bt_mul(g.B, x[3 * n] - g.mx, x[3 * n + 1] - g.my, x[3 * n + 2] - g.mz, w0, w1, w2);
    const float q = fminf(fmaxf(w0 * w0 + w1 * w1 + w2 * w2, 0.f), 1e8f);
    const float o = factor * g.s * __expf(-0.5f * q);
    if (opac) opac[p] = o;
    const float sum = row_sum16(o);
    if ((threadIdx.x & 15) == 0) density[n] = sum;
}

// the gradient of the sample positions, same mapping (the per-Gaussian gradients are the gather kernel's)
__global__ void __launch_bounds__(256) k_density_dx16(long long NK, const float* __restrict__ x, const long long* __restrict__ nbr,
                                                      const float* __restrict__ centers, const float* __restrict__ B,
                                                      const float* __restrict__ strengths, const float4* __restrict__ packed, float factor,
                                                      const float* __restrict__ g_opac, const float* __restrict__ g_den,
                                                      float* __restrict__ dx_out)
{
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= NK) return;
    const size_t n = (size_t)(p >> 4);
    const GaussNbr g = load_nbr(nbr[p], centers, B, strengths, packed);
    float w0, w1, w2;
    bt_mul(g.B, x[3 * n] - g.mx, x[3 * n + 1] - g.my, x[3 * n + 2] - g.mz, w0, w1, w2);
    const float q_raw = w0 * w0 + w1 * w1 + w2 * w2;
    const float e = __expf(-0.5f * fminf(fmaxf(q_raw, 0.f), 1e8f));
    const float go = (g_opac ? g_opac[p] : 0.f) + (g_den ? g_den[n] : 0.f);
    const float dq = (q_raw > 0.f && q_raw < 1e8f) ? -0.5f * factor * g.s * e * go : 0.f;
    const float dw0 = 2.f * w0 * dq, dw1 = 2.f * w1 * dq, dw2 = 2.f * w2 * dq;
    const float ax = row_sum16(g.B[0] * dw0 + g.B[1] * dw1 + g.B[2] * dw2);
    const float ay = row_sum16(g.B[3] * dw0 + g.B[4] * dw1 + g.B[5] * dw2);
    const float az = row_sum16(g.B[6] * dw0 + g.B[7] * dw1 + g.B[8] * dw2);
    if ((threadIdx.x & 15) == 0) { dx_out[3 * n] = ax; dx_out[3 * n + 1] = ay; dx_out[3 * n + 2] = az; }
}

__global__ void __launch_bounds__(256) k_density_fwd(int N, int K, const float* __restrict__ x, const long long* __restrict__ nbr,
                                                     const float* __restrict__ centers, const float* __restrict__ B,
                                                     const float* __restrict__ strengths, const float4* __restrict__ packed, float factor,
                                                     float* __restrict__ opac, float* __restrict__ density)
{
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const float px = x[3 * (size_t)n], py = x[3 * (size_t)n + 1], pz = x[3 * (size_t)n + 2];
    float sum = 0.f;
    for (int k = 0; k < K; k++) {
        const GaussNbr g = load_nbr(nbr[(size_t)n * K + k], centers, B, strengths, packed);
        float w0, w1, w2;
        bt_mul(g.B, px - g.mx, py - g.my, pz - g.mz, w0, w1, w2);
        const float q = fminf(fmaxf(w0 * w0 + w1 * w1 + w2 * w2, 0.f), 1e8f);
        const float o = factor * g.s * __expf(-0.5f * q);
        if (opac) opac[(size_t)n * K + k] = o;
        sum += o;
    }
    density[n] = sum;
}

__global__ void __launch_bounds__(256) k_density_bwd(int N, int K, const float* __restrict__ x, const long long* __restrict__ nbr,
                                                     const float* __restrict__ centers, const float* __restrict__ B,
                                                     const float* __restrict__ strengths, const float4* __restrict__ packed, float factor,
                                                     const float* __restrict__ g_opac, const float* __restrict__ g_den,
                                                     float* __restrict__ dx_out, float* __restrict__ dcenters,
                                                     float* __restrict__ dB, float* __restrict__ dstrengths)
{
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const float px = x[3 * (size_t)n], py = x[3 * (size_t)n + 1], pz = x[3 * (size_t)n + 2];
    const float gd = g_den ? g_den[n] : 0.f;
    float ax = 0.f, ay = 0.f, az = 0.f;
    for (int k = 0; k < K; k++) {
        const long long gi = nbr[(size_t)n * K + k];
        const GaussNbr g = load_nbr(gi, centers, B, strengths, packed);
        const float dx = px - g.mx, dy = py - g.my, dz = pz - g.mz;
        float w0, w1, w2;
        bt_mul(g.B, dx, dy, dz, w0, w1, w2);
        const float q_raw = w0 * w0 + w1 * w1 + w2 * w2;
        const float q = fminf(fmaxf(q_raw, 0.f), 1e8f);
        const float e = __expf(-0.5f * q);
        const float go = (g_opac ? g_opac[(size_t)n * K + k] : 0.f) + gd;  // dL/do
        atomicAdd(&dstrengths[gi], go * factor * e);
        // d o / d q = -0.5 o inside the clamp range, 0 outside (torch.clamp gradient)
        const float dq = (q_raw > 0.f && q_raw < 1e8f) ? -0.5f * factor * g.s * e * go : 0.f;
        const float dw0 = 2.f * w0 * dq, dw1 = 2.f * w1 * dq, dw2 = 2.f * w2 * dq;
        // d = x - mu;  w_j = sum_i B[i][j] d_i  ->  dL/dd_i = sum_j B[i][j] dw_j ;  dL/dB[i][j] = d_i dw_j
        const float dd0 = g.B[0] * dw0 + g.B[1] * dw1 + g.B[2] * dw2;
        const float dd1 = g.B[3] * dw0 + g.B[4] * dw1 + g.B[5] * dw2;
        const float dd2 = g.B[6] * dw0 + g.B[7] * dw1 + g.B[8] * dw2;
        ax += dd0; ay += dd1; az += dd2;
        if (dq != 0.f) {
            atomicAdd(&dcenters[3 * gi], -dd0); atomicAdd(&dcenters[3 * gi + 1], -dd1); atomicAdd(&dcenters[3 * gi + 2], -dd2);
            float* b = dB + 9 * gi;
            atomicAdd(&b[0], dx * dw0); atomicAdd(&b[1], dx * dw1); atomicAdd(&b[2], dx * dw2);
            atomicAdd(&b[3], dy * dw0); atomicAdd(&b[4], dy * dw1); atomicAdd(&b[5], dy * dw2);
            atomicAdd(&b[6], dz * dw0); atomicAdd(&b[7], dz * dw1); atomicAdd(&b[8], dz * dw2);
        }
    }
    if (dx_out) { dx_out[3 * (size_t)n] = ax; dx_out[3 * (size_t)n + 1] = ay; dx_out[3 * (size_t)n + 2] = az; }
}

// ---- gather formulation of the backward ---------------------------------------------------------------------------
// The kernel above spends 13 float atomics per (sample, neighbour) pair (208 M at 1M x 16: ~10 ms, L2 atomic rate).  Here the
// pairs are first laid out per Gaussian -- by launch_group_by_key below (stable radix grouping; until the end of round 4, and with
// SGR_GROUP_ATOMICS=1, by ONE returning integer atomic per pair for its rank, a scan and a fill) -- and sixteen lanes per Gaussian
// then sum its pairs in registers and write its 13 outputs once.  This kernel: the gradient of the sample positions (a lane per
// sample), plus the ranks in the atomics mode (cnt != NULL).
__global__ void __launch_bounds__(256) k_density_bwd_rank(int N, int K, const float* __restrict__ x, const long long* __restrict__ nbr,
                                                          const float* __restrict__ centers, const float* __restrict__ B,
                                                          const float* __restrict__ strengths, const float4* __restrict__ packed, float factor,
                                                          const float* __restrict__ g_opac, const float* __restrict__ g_den,
                                                          float* __restrict__ dx_out, uint32_t* __restrict__ cnt,
                                                          uint32_t* __restrict__ rank)
{
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const float px = x[3 * (size_t)n], py = x[3 * (size_t)n + 1], pz = x[3 * (size_t)n + 2];
    const float gd = g_den ? g_den[n] : 0.f;
    float ax = 0.f, ay = 0.f, az = 0.f;
    for (int k = 0; k < K; k++) {
        const size_t p = (size_t)n * K + k;
        const long long gi = nbr[p];
        if (cnt) rank[p] = atomicAdd(&cnt[gi], 1u);   // (cnt == NULL: the pairs are grouped by launch_group_by_key instead)
        if (dx_out) {
            const GaussNbr g = load_nbr(gi, centers, B, strengths, packed);
            float w0, w1, w2;
            bt_mul(g.B, px - g.mx, py - g.my, pz - g.mz, w0, w1, w2);
            const float q_raw = w0 * w0 + w1 * w1 + w2 * w2;
            const float e = __expf(-0.5f * fminf(fmaxf(q_raw, 0.f), 1e8f));
            const float go = (g_opac ? g_opac[p] : 0.f) + gd;
            const float dq = (q_raw > 0.f && q_raw < 1e8f) ? -0.5f * factor * g.s * e * go : 0.f;
            const float dw0 = 2.f * w0 * dq, dw1 = 2.f * w1 * dq, dw2 = 2.f * w2 * dq;
            ax += g.B[0] * dw0 + g.B[1] * dw1 + g.B[2] * dw2;
            ay += g.B[3] * dw0 + g.B[4] * dw1 + g.B[5] * dw2;
            az += g.B[6] * dw0 + g.B[7] * dw1 + g.B[8] * dw2;
        }
    }
    if (dx_out) { dx_out[3 * (size_t)n] = ax; dx_out[3 * (size_t)n + 1] = ay; dx_out[3 * (size_t)n + 2] = az; }
}

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

// groups the M entries of keys64 (values in [-P, P); others are left out) by key: *list_out = entry numbers, key-major, ascending
// inside a key; start[0..P] = offsets into it.  Enqueued on s; no host synchronisation.
int launch_group_by_key(long long M, const long long* keys64, int P, char* scratch, uint32_t* start, const uint32_t** list_out, hipStream_t s)
{
    const GroupScratch g = carve_group(scratch, (size_t)M);
    const uint32_t n_chunks = (uint32_t)(((size_t)M + GRP_CHUNK - 1) / GRP_CHUNK);
    const size_t H = 256 * (size_t)n_chunks;
    const int n_blocks = (int)((H + FSCAN_BLOCK - 1) / FSCAN_BLOCK);
    int bits = 0;
    while (bits < 32 && ((unsigned long long)P >> bits) != 0ull) bits++;   // P itself (the sentinel) must fit
    const int passes = (bits + 7) / 8 > 0 ? (bits + 7) / 8 : 1;
    uint32_t *kin = nullptr, *vin = nullptr, *kout = g.key_a, *vout = g.val_a;
    for (int pass = 0; pass < passes; pass++) {
        const int shift = 8 * pass;
        if (pass == 0) hipLaunchKernelGGL(k_grp_hist<true>, dim3(n_chunks), dim3(256), 0, s, M, keys64, kin, P, shift, n_chunks, g.hist);
        else hipLaunchKernelGGL(k_grp_hist<false>, dim3(n_chunks), dim3(256), 0, s, M, keys64, kin, P, shift, n_chunks, g.hist);
        hipLaunchKernelGGL(k_fscan_sums, dim3(n_blocks), dim3(256), 0, s, (int)H, g.hist, g.block_sums);
        hipLaunchKernelGGL(k_fscan_top, dim3(1), dim3(1024), 0, s, n_blocks, g.block_sums, g.offs + H);
        hipLaunchKernelGGL(k_fscan_apply, dim3(n_blocks), dim3(256), 0, s, (int)H, g.hist, g.block_sums, g.offs);
        if (pass == 0) hipLaunchKernelGGL(k_grp_scatter<true>, dim3(n_chunks), dim3(256), 0, s, M, keys64, kin, vin, P, shift, n_chunks, g.offs, kout, vout);
        else hipLaunchKernelGGL(k_grp_scatter<false>, dim3(n_chunks), dim3(256), 0, s, M, keys64, kin, vin, P, shift, n_chunks, g.offs, kout, vout);
        kin = kout; vin = vout;
        kout = (kin == g.key_a) ? g.key_b : g.key_a;
        vout = (vin == g.val_a) ? g.val_b : g.val_a;
    }
    hipLaunchKernelGGL(k_grp_bounds, dim3((unsigned)((P + 1 + 255) / 256)), dim3(256), 0, s, P, M, kin, start);
    *list_out = vin;
    return hipGetLastError() == hipSuccess ? 0 : SGR_E_HIP;
}

// SGR_GROUP_ATOMICS=1: the round-4 grouping by returning atomics (same-box A/B)
bool group_by_atomics()
{
    static const bool v = [] { const char* e = getenv("SGR_GROUP_ATOMICS"); return e && e[0] == '1'; }();
    return v;
}

__global__ void __launch_bounds__(256) k_density_bwd_fill(long long NK, const long long* __restrict__ nbr,
                                                          const uint32_t* __restrict__ start, const uint32_t* __restrict__ rank,
                                                          uint32_t* __restrict__ pair_list)
{
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= NK) return;
    pair_list[start[nbr[p]] + rank[p]] = (uint32_t)p;
}

// SIXTEEN lanes (one DPP row) per Gaussian: they stride over its pairs and fold their 13 partial sums with row rotates.  (One lane
// per Gaussian, until round 4, walked its list alone -- 280 dependent gathers on average when 1M samples x 16 neighbours meet 57k
// Gaussians, on 900 waves: 2.0 ms; a trainer's SDF phase has exactly that shape.)
__global__ void __launch_bounds__(256) k_density_bwd_gather(int P, int K, const float* __restrict__ x,
                                                            const float* __restrict__ centers, const float* __restrict__ B,
                                                            const float* __restrict__ strengths, const float4* __restrict__ packed, float factor,
                                                            const float* __restrict__ g_opac, const float* __restrict__ g_den,
                                                            const uint32_t* __restrict__ start,
                                                            const uint32_t* __restrict__ pair_list, float* __restrict__ dcenters,
                                                            float* __restrict__ dB, float* __restrict__ dstrengths)
{
    const int t = (int)(((size_t)blockIdx.x * 256 + threadIdx.x) >> 4);
    const uint32_t sub = threadIdx.x & 15;
    if (t >= P) return;   // (whole rows leave together: the row rotates below never cross a row)
    const GaussNbr g = load_nbr(t, centers, B, strengths, packed);
    float dc0 = 0.f, dc1 = 0.f, dc2 = 0.f, ds = 0.f;
    float b[9];
#pragma unroll
    for (int i = 0; i < 9; i++) b[i] = 0.f;
    const uint32_t e0 = start[t], e1 = start[t + 1];
    for (uint32_t e = e0 + sub; e < e1; e += 16) {
        const uint32_t p = pair_list[e];
        const uint32_t n = p / (uint32_t)K;
        const float dx = x[3 * (size_t)n] - g.mx, dy = x[3 * (size_t)n + 1] - g.my, dz = x[3 * (size_t)n + 2] - g.mz;
        float w0, w1, w2;
        bt_mul(g.B, dx, dy, dz, w0, w1, w2);
        const float q_raw = w0 * w0 + w1 * w1 + w2 * w2;
        const float ex = __expf(-0.5f * fminf(fmaxf(q_raw, 0.f), 1e8f));
        const float go = (g_opac ? g_opac[p] : 0.f) + (g_den ? g_den[n] : 0.f);
        ds += go * factor * ex;
        const float dq = (q_raw > 0.f && q_raw < 1e8f) ? -0.5f * factor * g.s * ex * go : 0.f;
        const float dw0 = 2.f * w0 * dq, dw1 = 2.f * w1 * dq, dw2 = 2.f * w2 * dq;
        dc0 -= g.B[0] * dw0 + g.B[1] * dw1 + g.B[2] * dw2;
        dc1 -= g.B[3] * dw0 + g.B[4] * dw1 + g.B[5] * dw2;
        dc2 -= g.B[6] * dw0 + g.B[7] * dw1 + g.B[8] * dw2;
        b[0] += dx * dw0; b[1] += dx * dw1; b[2] += dx * dw2;
        b[3] += dy * dw0; b[4] += dy * dw1; b[5] += dy * dw2;
        b[6] += dz * dw0; b[7] += dz * dw1; b[8] += dz * dw2;
    }
    dc0 = row_sum16(dc0); dc1 = row_sum16(dc1); dc2 = row_sum16(dc2); ds = row_sum16(ds);
#pragma unroll
    for (int i = 0; i < 9; i++) b[i] = row_sum16(b[i]);
    if (sub == 0) {
        dcenters[3 * (size_t)t] = dc0; dcenters[3 * (size_t)t + 1] = dc1; dcenters[3 * (size_t)t + 2] = dc2;
        dstrengths[t] = ds;
    }
    if (sub < 9) {   // nine lanes store the nine entries of dB (each holds all the sums)
        float v = b[0];
#pragma unroll
        for (int i = 1; i < 9; i++) v = (sub == (uint32_t)i) ? b[i] : v;
        dB[9 * (size_t)t + sub] = v;
    }
}

// ---- out[p, :] = sum over { n : idx[n] == p } of src[n, :]  -- the backward of a row gather `x[idx]` --------------------------------
// What autograd runs for every `tensor[index]` of the regulariser (sugar_model.py:922-925: points / quaternions / scaling of 1M sampled
// Gaussians; coarse_sdf.py:690-692: the normals of 1M x 16 neighbours): stock PyTorch sorts the indices and reduces segments, 1.3 ms per
// call on average and six calls per iteration.  Same scheme as the density backward above: the entries are grouped by row
// (launch_group_by_key; k_rows_rank / k_rows_fill are the SGR_GROUP_ATOMICS=1 variant), sixteen lanes per row add its entries up.
// Negative indices wrap once (Python semantics); entries outside [-P, P) are ignored.
__device__ __forceinline__ long long rows_wrap(long long i, int P) { return i < 0 ? i + P : i; }

__global__ void __launch_bounds__(256) k_rows_rank(long long N, const long long* __restrict__ idx, int P, uint32_t* __restrict__ cnt,
                                                   uint32_t* __restrict__ rank)
{
    const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const long long g = rows_wrap(idx[n], P);
    if (g >= 0 && g < P) rank[n] = atomicAdd(&cnt[g], 1u);
}

__global__ void __launch_bounds__(256) k_rows_fill(long long N, const long long* __restrict__ idx, int P, const uint32_t* __restrict__ start,
                                                   const uint32_t* __restrict__ rank, uint32_t* __restrict__ list)
{
    const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const long long g = rows_wrap(idx[n], P);
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

// ---- SuGaR.get_covariance(return_sqrt=True[, inverse_scales=True]), sugar_scene/sugar_model.py:730-736 ---------------------
// out[a][b] = R(q)[a][b] * s[b],  R = pytorch3d's quaternion_to_matrix (real part first, two_s = 2 / |q|^2: any non-zero q),
// s = scaling or 1 / clamp(scaling, 1e-8).  The reference builds it with ~25 elementwise launches (plus autograd twins) every
// time the regulariser or the level-set sampler runs.
__device__ __forceinline__ void quat_M(float r, float i, float j, float k, float M[9])
{
    M[0] = -(j * j + k * k); M[1] = i * j - k * r;     M[2] = i * k + j * r;
    M[3] = i * j + k * r;    M[4] = -(i * i + k * k);  M[5] = j * k - i * r;
    M[6] = i * k - j * r;    M[7] = j * k + i * r;     M[8] = -(i * i + j * j);
}

// the depth render's colours (sugar_model.py:1901-1911): every Gaussian's view-space z three times (`depth.expand(-1, 3)`), from the
// rasterizer's row-vector view matrix -- as torch ops a [P,3] x [3,1] GEMM, an add and an expanding copy
__global__ void __launch_bounds__(256) k_view_depth_rgb(int P, const float* __restrict__ centers, const float* __restrict__ viewmatrix,
                                                        float* __restrict__ out)
{
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= P) return;
    const float x = centers[3 * (size_t)g], y = centers[3 * (size_t)g + 1], z = centers[3 * (size_t)g + 2];
    const float d = x * viewmatrix[2] + y * viewmatrix[6] + z * viewmatrix[10] + viewmatrix[14];
    out[3 * (size_t)g] = d; out[3 * (size_t)g + 1] = d; out[3 * (size_t)g + 2] = d;
}

// ---- the two per-view preparations of the level-set sampler (sugar_model.py:1934-1972), one launch each ------------------------
// gaussian_std of :1971-1972: | scales (.) R(q)^T normalize(cam_center - centre) | with the unit quaternions the model hands out
// (`quaternion_apply(quaternion_invert(q), v)`; F.normalize: v / max(|v|, 1e-12)).  As torch ops this was ~40 launches over [P].
__global__ void __launch_bounds__(256) k_view_std(int P, const float* __restrict__ centers, const float* __restrict__ quats,
                                                  const float* __restrict__ scaling, const float* __restrict__ cam_center,
                                                  float* __restrict__ out)
{
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= P) return;
    const float4 q = reinterpret_cast<const float4*>(quats)[g];
    const float r = q.x, x = q.y, y = q.z, z = q.w;
    float vx = cam_center[0] - centers[3 * (size_t)g], vy = cam_center[1] - centers[3 * (size_t)g + 1],
          vz = cam_center[2] - centers[3 * (size_t)g + 2];
    const float inv = 1.0f / fmaxf(sqrtf(vx * vx + vy * vy + vz * vz), 1e-12f);
    vx *= inv; vy *= inv; vz *= inv;
    // rows of R^T = columns of R
    const float ox = (1 - 2 * (y * y + z * z)) * vx + 2 * (x * y + r * z) * vy + 2 * (x * z - r * y) * vz;
    const float oy = 2 * (x * y - r * z) * vx + (1 - 2 * (x * x + z * z)) * vy + 2 * (y * z + r * x) * vz;
    const float oz = 2 * (x * z + r * y) * vx + 2 * (y * z - r * x) * vy + (1 - 2 * (x * x + y * y)) * vz;
    const float sx = scaling[3 * (size_t)g] * ox, sy = scaling[3 * (size_t)g + 1] * oy, sz = scaling[3 * (size_t)g + 2] * oz;
    out[g] = sqrtf(sx * sx + sy * sy + sz * sz);
}

// World points of picked pixels (:1934-1959).  The reference lays an NDC grid over the image (x = W/m - 2 col / (m - 1), +x to the
// LEFT, +y UP, m = min(W, H)) and un-projects through a camera whose focal length in NDC units is 2 fx / m; the rasterizer's camera
// frame (+x right, +y down) is that frame with x and y negated.  `viewmatrix` is the rasterizer's (row vectors: p_view = [p 1] V);
// its inverse is taken here, in closed form, by every thread (a 4 x 4 torch.linalg.inv is a factorisation plus a host check).
__global__ void __launch_bounds__(256) k_unproject_pixels(int n, const int64_t* __restrict__ picked, const float* __restrict__ depth,
                                                          int W, int H, float f_ndc_x, float f_ndc_y,
                                                          const float* __restrict__ viewmatrix, float* __restrict__ world)
{
    // the inverse's first three columns (all the back-projection reads), by 2 x 2 sub-determinants; every thread the same few dozen
    // operations on the same 16 scalars
    const float m00 = viewmatrix[0], m01 = viewmatrix[1], m02 = viewmatrix[2], m03 = viewmatrix[3];
    const float m10 = viewmatrix[4], m11 = viewmatrix[5], m12 = viewmatrix[6], m13 = viewmatrix[7];
    const float m20 = viewmatrix[8], m21 = viewmatrix[9], m22 = viewmatrix[10], m23 = viewmatrix[11];
    const float m30 = viewmatrix[12], m31 = viewmatrix[13], m32 = viewmatrix[14], m33 = viewmatrix[15];
    const float s0 = m00 * m11 - m10 * m01, s1 = m00 * m12 - m10 * m02, s2 = m00 * m13 - m10 * m03;
    const float s3 = m01 * m12 - m11 * m02, s4 = m01 * m13 - m11 * m03, s5 = m02 * m13 - m12 * m03;
    const float c5 = m22 * m33 - m32 * m23, c4 = m21 * m33 - m31 * m23, c3 = m21 * m32 - m31 * m22;
    const float c2 = m20 * m33 - m30 * m23, c1 = m20 * m32 - m30 * m22, c0 = m20 * m31 - m30 * m21;
    const float idet = 1.0f / (s0 * c5 - s1 * c4 + s2 * c3 + s3 * c2 - s4 * c1 + s5 * c0);
    const float i00 = (m11 * c5 - m12 * c4 + m13 * c3) * idet, i01 = (-m01 * c5 + m02 * c4 - m03 * c3) * idet, i02 = (m31 * s5 - m32 * s4 + m33 * s3) * idet;
    const float i10 = (-m10 * c5 + m12 * c2 - m13 * c1) * idet, i11 = (m00 * c5 - m02 * c2 + m03 * c1) * idet, i12 = (-m30 * s5 + m32 * s2 - m33 * s1) * idet;
    const float i20 = (m10 * c4 - m11 * c2 + m13 * c0) * idet, i21 = (-m00 * c4 + m01 * c2 - m03 * c0) * idet, i22 = (m30 * s4 - m31 * s2 + m33 * s0) * idet;
    const float i30 = (-m10 * c3 + m11 * c1 - m12 * c0) * idet, i31 = (m00 * c3 - m01 * c1 + m02 * c0) * idet, i32 = (-m30 * s3 + m31 * s1 - m32 * s0) * idet;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const int64_t pix = picked[t];
    const int row = (int)(pix / W), col = (int)(pix - (int64_t)row * W);
    const int mm = W < H ? W : H;
    const float ndc_x = (float)W / (float)mm - ((float)col / (float)(mm - 1)) * 2.0f;
    const float ndc_y = (float)H / (float)mm - ((float)row / (float)(mm - 1)) * 2.0f;
    const float z = depth[pix];
    const float xc = -ndc_x * z / f_ndc_x, yc = -ndc_y * z / f_ndc_y;
    world[3 * (size_t)t] = xc * i00 + yc * i10 + z * i20 + i30;
    world[3 * (size_t)t + 1] = xc * i01 + yc * i11 + z * i21 + i31;
    world[3 * (size_t)t + 2] = xc * i02 + yc * i12 + z * i22 + i32;
}

__global__ void __launch_bounds__(256) k_scaled_rotation_fwd(int P, const float* __restrict__ quats, const float* __restrict__ scaling,
                                                             int inverse, float* __restrict__ out)
{
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= P) return;
    const float4 q = reinterpret_cast<const float4*>(quats)[g];
    float s[3] = {scaling[3 * (size_t)g], scaling[3 * (size_t)g + 1], scaling[3 * (size_t)g + 2]};
    if (inverse) { for (int b = 0; b < 3; b++) s[b] = 1.0f / fmaxf(s[b], 1e-8f); }
    const float t = 2.0f / (q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
    float M[9];
    quat_M(q.x, q.y, q.z, q.w, M);
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) out[9 * (size_t)g + 3 * a + b] = ((a == b ? 1.0f : 0.0f) + t * M[3 * a + b]) * s[b];
}

__global__ void __launch_bounds__(256) k_scaled_rotation_bwd(int P, const float* __restrict__ quats, const float* __restrict__ scaling,
                                                             int inverse, const float* __restrict__ g_out,
                                                             float* __restrict__ d_quats, float* __restrict__ d_scaling)
{
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= P) return;
    const float4 q = reinterpret_cast<const float4*>(quats)[g];
    const float r = q.x, i = q.y, j = q.z, k = q.w;
    float raw[3] = {scaling[3 * (size_t)g], scaling[3 * (size_t)g + 1], scaling[3 * (size_t)g + 2]};
    float s[3];
    for (int b = 0; b < 3; b++) s[b] = inverse ? 1.0f / fmaxf(raw[b], 1e-8f) : raw[b];
    const float n = r * r + i * i + j * j + k * k;
    const float t = 2.0f / n;
    float M[9];
    quat_M(r, i, j, k, M);
    float G[9], ds[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) {
            const float go = g_out[9 * (size_t)g + 3 * a + b];
            ds[b] += go * ((a == b ? 1.0f : 0.0f) + t * M[3 * a + b]);
            G[3 * a + b] = go * s[b];  // dL/dR
        }
    float GM = 0.f;
#pragma unroll
    for (int e = 0; e < 9; e++) GM += G[e] * M[e];
    // dL/dq = t * sum G : dM/dq  +  (G : M) * dt/dq,   dt/dq = -t^2 q
    const float dr = t * (-k * G[1] + j * G[2] + k * G[3] - i * G[5] - j * G[6] + i * G[7]) - GM * t * t * r;
    const float di = t * (j * G[1] + k * G[2] + j * G[3] - 2.f * i * G[4] - r * G[5] + k * G[6] + r * G[7] - 2.f * i * G[8]) - GM * t * t * i;
    const float dj = t * (-2.f * j * G[0] + i * G[1] + r * G[2] + i * G[3] + k * G[5] - r * G[6] + k * G[7] - 2.f * j * G[8]) - GM * t * t * j;
    const float dk = t * (-2.f * k * G[0] - r * G[1] + i * G[2] + r * G[3] - 2.f * k * G[4] + j * G[5] + i * G[6] + j * G[7]) - GM * t * t * k;
    reinterpret_cast<float4*>(d_quats)[g] = make_float4(dr, di, dj, dk);
#pragma unroll
    for (int b = 0; b < 3; b++) {
        float v = ds[b];
        if (inverse) v = raw[b] > 1e-8f ? -v * s[b] * s[b] : 0.f;  // d (1 / clamp(x, 1e-8)) = -1/x^2 inside the clamp range
        d_scaling[3 * (size_t)g + b] = v;
    }
}

#define LS_MAX_RANGE 32
#define LS_MAX_LEVELS 8
struct LevelArgs { int n; float v[LS_MAX_LEVELS]; };

// MAXR: samples held in registers (the reference's 21, or up to LS_MAX_RANGE): 144 VGPRs with 32 of them, what round 5's verdict flagged
template <int MAXR>
__global__ void __launch_bounds__(128) k_level_set(int N, int K, const float* __restrict__ world_points,
                                                   const long long* __restrict__ nbr, const float* __restrict__ cam_center,
                                                   const float* __restrict__ centers, const float* __restrict__ B,
                                                   const float* __restrict__ strengths, const float4* __restrict__ packed, const float* __restrict__ gaussian_std,
                                                   LevelArgs levels, int n_range, float range_size, float factor,
                                                   uint8_t* __restrict__ valid, float* __restrict__ points, float* __restrict__ normals)
{
    const int n = blockIdx.x * 128 + threadIdx.x;
    if (n >= N) return;
    const float wx = world_points[3 * (size_t)n], wy = world_points[3 * (size_t)n + 1], wz = world_points[3 * (size_t)n + 2];
    // camera_to_samples = normalize(p - camera_center)  (:1978); F.normalize divides by max(|v|, 1e-12)
    float dirx = wx - cam_center[0], diry = wy - cam_center[1], dirz = wz - cam_center[2];
    const float dn = fmaxf(sqrtf(dirx * dirx + diry * diry + dirz * dirz), 1e-12f);
    dirx /= dn; diry /= dn; dirz /= dn;
    const long long* my_nbr = nbr + (size_t)n * K;
    const float sigma = gaussian_std[my_nbr[0]];  // points_stds (:1973)
    // points_range = linspace(-range, range, n_range) * sigma  (:1976-1977); torch.linspace: start + i * step
    const float step = n_range > 1 ? (2.f * range_size) / (float)(n_range - 1) : 0.f;
    float dens[MAXR];
#pragma unroll
    for (int i = 0; i < MAXR; i++) dens[i] = 0.f;
    for (int k = 0; k < K; k++) {
        const GaussNbr g = load_nbr(my_nbr[k], centers, B, strengths, packed);
        float a0, a1, a2, b0, b1, b2;
        bt_mul(g.B, wx - g.mx, wy - g.my, wz - g.mz, a0, a1, a2);
        bt_mul(g.B, dirx, diry, dirz, b0, b1, b2);
        const float fs = factor * g.s;
#pragma unroll
        for (int i = 0; i < MAXR; i++) {
            if (i < n_range) {
                const float t = (-range_size + (float)i * step) * sigma;
                const float w0 = a0 + t * b0, w1 = a1 + t * b1, w2 = a2 + t * b2;
                const float q = fminf(fmaxf(w0 * w0 + w1 * w1 + w2 * w2, 0.f), 1e8f);
                dens[i] += fs * __expf(-0.5f * q);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < MAXR; i++)
        if (dens[i] >= 1.f) dens[i] = dens[i] / (dens[i] + 1e-12f);  // :2007-2008
#pragma clang loop unroll(disable)
    for (int l = 0; l < levels.n; l++) {
        const float L = levels.v[l];  // (run-time index into the kernel arguments: scalar loads, no registers held)
        // first sample above the level (argmax of a boolean row: 0 when none is above), :2019-2020
        int first = 0;
        float d_first = 0.f, d_prev = 0.f;
        bool found = false;
#pragma unroll
        for (int i = 0; i < MAXR; i++) {
            if (i < n_range && !found && (dens[i] - L > 0.f)) {
                found = true; first = i; d_first = dens[i];
                d_prev = (i > 0) ? dens[i - 1] : 0.f;
            }
        }
        const bool under0 = (dens[0] - L < 0.f);
        const bool empty = (!under0) || (first == 0);  // :2021
        const size_t o = (size_t)l * N + n;
        valid[o] = empty ? 0 : 1;
        float ix = 0.f, iy = 0.f, iz = 0.f, nx = 0.f, ny = 0.f, nz = 0.f;
        if (!empty) {
            const float t_first = (-range_size + (float)first * step) * sigma;
            const float t_prev = (-range_size + (float)(first - 1) * step) * sigma;
            const float t = (L - d_prev) / (d_first - d_prev) * (t_first - t_prev) + t_prev;  // :2035
            ix = wx + t * dirx; iy = wy + t * diry; iz = wz + t * dirz;                    // :2036
            if (normals) {
                float gx = 0.f, gy = 0.f, gz = 0.f;  // density_grad = sum_g o_g * B_g w_g  (:2069)
                for (int k = 0; k < K; k++) {
                    const GaussNbr g = load_nbr(my_nbr[k], centers, B, strengths, packed);
                    float w0, w1, w2;
                    bt_mul(g.B, ix - g.mx, iy - g.my, iz - g.mz, w0, w1, w2);
                    const float q = fminf(fmaxf(w0 * w0 + w1 * w1 + w2 * w2, 0.f), 1e8f);
                    const float oo = factor * g.s * __expf(-0.5f * q);
                    gx += oo * (g.B[0] * w0 + g.B[1] * w1 + g.B[2] * w2);
                    gy += oo * (g.B[3] * w0 + g.B[4] * w1 + g.B[5] * w2);
                    gz += oo * (g.B[6] * w0 + g.B[7] * w1 + g.B[8] * w2);
                }
                const float gn = fmaxf(sqrtf(gx * gx + gy * gy + gz * gz), 1e-12f);
                nx = -gx / gn; ny = -gy / gn; nz = -gz / gn;  // :2078
            }
        }
        points[3 * o] = ix; points[3 * o + 1] = iy; points[3 * o + 2] = iz;
        if (normals) { normals[3 * o] = nx; normals[3 * o + 1] = ny; normals[3 * o + 2] = nz; }
    }
}

}  // namespace

// the stable grouping above with external linkage, for csrc/sdf_regulariser.hip (declared in sgr_group.h)
size_t sgr_group_scratch_bytes(size_t M) { return carve_group(nullptr, M).total; }
int sgr_group_by_key(long long M, const long long* keys64, int P, char* scratch, uint32_t* start, const uint32_t** list_out, hipStream_t s)
{
    return launch_group_by_key(M, keys64, P, scratch, start, list_out, s);
}

extern "C" {

int sgr_density_field_forward(int N, int K, const float* x, const int64_t* nbr_idx, const float* centers,
                              const float* inv_scaled_rot, const float* strengths, float density_factor,
                              float* neighbor_opacities, float* density, const float* packed, void* stream)
{
    if (N <= 0) return 0;
    if (K <= 0 || !x || !nbr_idx || !centers || !inv_scaled_rot || !strengths || !density) return SGR_E_INVALID;
    if (K == 16) {
        const long long nk = (long long)N * 16;
        hipLaunchKernelGGL(k_density_fwd16, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, (hipStream_t)stream, nk, x,
                           reinterpret_cast<const long long*>(nbr_idx), centers, inv_scaled_rot, strengths, reinterpret_cast<const float4*>(packed),
                           density_factor, neighbor_opacities, density);
    } else {
        hipLaunchKernelGGL(k_density_fwd, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, N, K, x,
                           reinterpret_cast<const long long*>(nbr_idx), centers, inv_scaled_rot, strengths, reinterpret_cast<const float4*>(packed),
                           density_factor, neighbor_opacities, density);
    }
    return hipGetLastError() == hipSuccess ? 0 : SGR_E_HIP;
}

int sgr_density_field_backward(int N, int K, const float* x, const int64_t* nbr_idx, const float* centers,
                               const float* inv_scaled_rot, const float* strengths, float density_factor,
                               const float* dL_dopacities, const float* dL_ddensity, float* dL_dx, float* dL_dcenters,
                               float* dL_dinv_scaled_rot, float* dL_dstrengths, const float* packed, void* stream)
{
    if (N <= 0) return 0;
    if (K <= 0 || !x || !nbr_idx || !centers || !inv_scaled_rot || !strengths || !dL_dcenters || !dL_dinv_scaled_rot ||
        !dL_dstrengths || (!dL_dopacities && !dL_ddensity))
        return SGR_E_INVALID;
    hipLaunchKernelGGL(k_density_bwd, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, N, K, x,
                       reinterpret_cast<const long long*>(nbr_idx), centers, inv_scaled_rot, strengths, reinterpret_cast<const float4*>(packed),
                       density_factor, dL_dopacities, dL_ddensity, dL_dx, dL_dcenters, dL_dinv_scaled_rot, dL_dstrengths);
    return hipGetLastError() == hipSuccess ? 0 : SGR_E_HIP;
}

int sgr_scaled_rotation_forward(int P, const float* quaternions, const float* scaling, int inverse_scales, float* out, void* stream)
{
    if (P <= 0) return 0;
    if (!quaternions || !scaling || !out || ((uintptr_t)quaternions & 15)) return SGR_E_INVALID;
    hipLaunchKernelGGL(k_scaled_rotation_fwd, dim3((P + 255) / 256), dim3(256), 0, (hipStream_t)stream, P, quaternions, scaling,
                       inverse_scales, out);
    return hipGetLastError() == hipSuccess ? 0 : SGR_E_HIP;
}

int sgr_scaled_rotation_backward(int P, const float* quaternions, const float* scaling, int inverse_scales, const float* dL_dout,
                                 float* dL_dquaternions, float* dL_dscaling, void* stream)
{
    if (P <= 0) return 0;
    if (!quaternions || !scaling || !dL_dout || !dL_dquaternions || !dL_dscaling ||
        (((uintptr_t)quaternions | (uintptr_t)dL_dquaternions) & 15))
        return SGR_E_INVALID;
    hipLaunchKernelGGL(k_scaled_rotation_bwd, dim3((P + 255) / 256), dim3(256), 0, (hipStream_t)stream, P, quaternions, scaling,
                       inverse_scales, dL_dout, dL_dquaternions, dL_dscaling);
    return hipGetLastError() == hipSuccess ? 0 : SGR_E_HIP;
}

int sgr_view_depth_rgb(int P, const float* centers, const float* viewmatrix, float* out, void* stream)
{
    if (P <= 0) return 0;
    if (!centers || !viewmatrix || !out) return SGR_E_INVALID;
    hipLaunchKernelGGL(k_view_depth_rgb, dim3((P + 255) / 256), dim3(256), 0, (hipStream_t)stream, P, centers, viewmatrix, out);
    return hipGetLastError() == hipSuccess ? 0 : SGR_E_HIP;
}

int sgr_view_std(int P, const float* centers, const float* quaternions, const float* scaling, const float* cam_center, float* out,
                 void* stream)
{
    if (P <= 0) return 0;
    if (!centers || !quaternions || !scaling || !cam_center || !out || ((uintptr_t)quaternions & 15)) return SGR_E_INVALID;
    hipLaunchKernelGGL(k_view_std, dim3((P + 255) / 256), dim3(256), 0, (hipStream_t)stream, P, centers, quaternions, scaling, cam_center,
                       out);
    return hipGetLastError() == hipSuccess ? 0 : SGR_E_HIP;
}

int sgr_unproject_pixels(int n, const int64_t* picked, const float* depth, int width, int height, float tanfovx, float tanfovy,
                         const float* viewmatrix, float* world, void* stream)
{
    if (n <= 0) return 0;
    if (!picked || !depth || !viewmatrix || !world || width < 2 || height < 2 || !(tanfovx > 0.f) || !(tanfovy > 0.f)) return SGR_E_INVALID;
    const int m = width < height ? width : height;
    const float f_ndc_x = ((float)width / (2.0f * tanfovx)) * 2.0f / (float)m, f_ndc_y = ((float)height / (2.0f * tanfovy)) * 2.0f / (float)m;
    hipLaunchKernelGGL(k_unproject_pixels, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, picked, depth, width, height,
                       f_ndc_x, f_ndc_y, viewmatrix, world);
    return hipGetLastError() == hipSuccess ? 0 : SGR_E_HIP;
}

int sgr_pack_gaussians(int P, const float* centers, const float* inv_scaled_rot, const float* strengths, float* packed, void* stream)
{
    if (P <= 0) return 0;
    if (!centers || !inv_scaled_rot || !strengths || !packed || ((uintptr_t)packed & 15)) return SGR_E_INVALID;
    hipLaunchKernelGGL(k_pack_gaussians, dim3((P + 255) / 256), dim3(256), 0, (hipStream_t)stream, P, centers, inv_scaled_rot,
                       strengths, reinterpret_cast<float4*>(packed));
    return hipGetLastError() == hipSuccess ? 0 : SGR_E_HIP;
}

size_t sgr_density_field_backward_scratch_bytes(int N, int K, int P)
{
    const size_t nk = (size_t)(N > 0 ? N : 0) * (size_t)(K > 0 ? K : 0), p = (size_t)(P > 0 ? P : 0);
    const size_t blocks = (p + FSCAN_BLOCK - 1) / FSCAN_BLOCK + 1;
    return sgr_align((p + 1) * 4) * 2 + sgr_align(blocks * 4) + 2 * sgr_align(nk * 4)   // cnt | start | block sums | rank | pair_list
           + carve_group(nullptr, nk).total;                                            // | the radix grouping's buffers
}

int sgr_density_field_backward_gather(int N, int K, int P, const float* x, const int64_t* nbr_idx, const float* centers,
                                      const float* inv_scaled_rot, const float* strengths, float density_factor,
                                      const float* dL_dopacities, const float* dL_ddensity, float* dL_dx, float* dL_dcenters,
                                      float* dL_dinv_scaled_rot, float* dL_dstrengths, char* scratch, const float* packed, void* stream)
{
    if (P <= 0) return 0;
    // (N == 0: no pair reads a gradient, and empty tensors hand NULL for both -- every output row is written as 0)
    if (N < 0 || K <= 0 || (N > 0 && (!x || !nbr_idx || (!dL_dopacities && !dL_ddensity))) || !centers || !inv_scaled_rot ||
        !strengths || !dL_dcenters || !dL_dinv_scaled_rot || !dL_dstrengths || !scratch || (size_t)N * K > 0xFFFFFFFFull)
        return SGR_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const size_t nk = (size_t)N * K, pa = sgr_align(((size_t)P + 1) * 4);
    const int n_blocks = (P + FSCAN_BLOCK - 1) / FSCAN_BLOCK;
    const size_t ba = sgr_align(((size_t)n_blocks + 1) * 4);
    uint32_t* cnt = reinterpret_cast<uint32_t*>(scratch);
    uint32_t* start = reinterpret_cast<uint32_t*>(scratch + pa);
    uint32_t* block_sums = reinterpret_cast<uint32_t*>(scratch + 2 * pa);
    uint32_t* rank = reinterpret_cast<uint32_t*>(scratch + 2 * pa + ba);
    uint32_t* pair_list = reinterpret_cast<uint32_t*>(scratch + 2 * pa + ba + sgr_align(nk * 4));
    const long long* nbr = reinterpret_cast<const long long*>(nbr_idx);
    const uint32_t* pairs = pair_list;
    if (group_by_atomics() || N == 0) {
        if (hipMemsetAsync(cnt, 0, ((size_t)P + 1) * 4, s) != hipSuccess) return SGR_E_HIP;
        if (N > 0) {
            hipLaunchKernelGGL(k_density_bwd_rank, dim3((N + 255) / 256), dim3(256), 0, s, N, K, x, nbr, centers, inv_scaled_rot,
                               strengths, reinterpret_cast<const float4*>(packed), density_factor, dL_dopacities, dL_ddensity, dL_dx, cnt, rank);
        }
        hipLaunchKernelGGL(k_fscan_sums, dim3(n_blocks), dim3(256), 0, s, P, cnt, block_sums);
        hipLaunchKernelGGL(k_fscan_top, dim3(1), dim3(1024), 0, s, n_blocks, block_sums, start + P);
        hipLaunchKernelGGL(k_fscan_apply, dim3(n_blocks), dim3(256), 0, s, P, cnt, block_sums, start);
        if (N > 0) {
            hipLaunchKernelGGL(k_density_bwd_fill, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, s, (long long)nk, nbr, start, rank,
                               pair_list);
        }
    } else {
        if (dL_dx && K == 16) {   // the gradient of the sample positions: a lane per pair
            hipLaunchKernelGGL(k_density_dx16, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, s, (long long)nk, x, nbr, centers,
                               inv_scaled_rot, strengths, reinterpret_cast<const float4*>(packed), density_factor, dL_dopacities,
                               dL_ddensity, dL_dx);
        } else if (dL_dx) {       // ... a lane per sample (no atomics in this mode)
            hipLaunchKernelGGL(k_density_bwd_rank, dim3((N + 255) / 256), dim3(256), 0, s, N, K, x, nbr, centers, inv_scaled_rot,
                               strengths, reinterpret_cast<const float4*>(packed), density_factor, dL_dopacities, dL_ddensity, dL_dx,
                               (uint32_t*)nullptr, rank);
        }
        char* gscratch = scratch + 2 * pa + ba + 2 * sgr_align(nk * 4);
        const int rc = launch_group_by_key((long long)nk, nbr, P, gscratch, start, &pairs, s);
        if (rc < 0) return rc;
    }
    hipLaunchKernelGGL(k_density_bwd_gather, dim3((unsigned)(((size_t)P * 16 + 255) / 256)), dim3(256), 0, s, P, K, x, centers, inv_scaled_rot, strengths,
                       reinterpret_cast<const float4*>(packed), density_factor, dL_dopacities, dL_ddensity, start, pairs, dL_dcenters, dL_dinv_scaled_rot, dL_dstrengths);
    return hipGetLastError() == hipSuccess ? 0 : SGR_E_HIP;
}

size_t sgr_scatter_add_rows_scratch_bytes(long long N, int P)
{
    const size_t n = (size_t)(N > 0 ? N : 0), p = (size_t)(P > 0 ? P : 0);
    const size_t blocks = (p + FSCAN_BLOCK - 1) / FSCAN_BLOCK + 1;
    return sgr_align((p + 1) * 4) * 2 + sgr_align(blocks * 4) + 2 * sgr_align(n * 4)   // cnt | start | block sums | rank | list
           + carve_group(nullptr, n).total;                                           // | the radix grouping's buffers
}

int sgr_scatter_add_rows(long long N, const int64_t* idx, const float* src, int W, int P, float* out, char* scratch, void* stream)
{
    if (P <= 0) return 0;
    if (N < 0 || W < 1 || W > 4 || (N > 0 && (!idx || !src)) || !out || !scratch || (unsigned long long)N > 0xFFFFFFFFull)
        return SGR_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const size_t pa = sgr_align(((size_t)P + 1) * 4);
    const int n_blocks = (P + FSCAN_BLOCK - 1) / FSCAN_BLOCK;
    const size_t ba = sgr_align(((size_t)n_blocks + 1) * 4);
    uint32_t* cnt = reinterpret_cast<uint32_t*>(scratch);
    uint32_t* start = reinterpret_cast<uint32_t*>(scratch + pa);
    uint32_t* block_sums = reinterpret_cast<uint32_t*>(scratch + 2 * pa);
    uint32_t* rank = reinterpret_cast<uint32_t*>(scratch + 2 * pa + ba);
    uint32_t* list = reinterpret_cast<uint32_t*>(scratch + 2 * pa + ba + sgr_align((size_t)N * 4));
    const long long* ix = reinterpret_cast<const long long*>(idx);
    const uint32_t* entries = list;
    if (group_by_atomics() || N == 0) {
        if (hipMemsetAsync(cnt, 0, ((size_t)P + 1) * 4, s) != hipSuccess) return SGR_E_HIP;
        const unsigned nb = (unsigned)(((size_t)N + 255) / 256);
        if (N > 0) hipLaunchKernelGGL(k_rows_rank, dim3(nb), dim3(256), 0, s, N, ix, P, cnt, rank);
        hipLaunchKernelGGL(k_fscan_sums, dim3(n_blocks), dim3(256), 0, s, P, cnt, block_sums);
        hipLaunchKernelGGL(k_fscan_top, dim3(1), dim3(1024), 0, s, n_blocks, block_sums, start + P);
        hipLaunchKernelGGL(k_fscan_apply, dim3(n_blocks), dim3(256), 0, s, P, cnt, block_sums, start);
        if (N > 0) hipLaunchKernelGGL(k_rows_fill, dim3(nb), dim3(256), 0, s, N, ix, P, start, rank, list);
    } else {
        char* gscratch = scratch + 2 * pa + ba + 2 * sgr_align((size_t)N * 4);
        const int rc = launch_group_by_key(N, ix, P, gscratch, start, &entries, s);
        if (rc < 0) return rc;
    }
    const unsigned gb = (unsigned)(((size_t)P * 16 + 255) / 256);
    switch (W) {
        case 1: hipLaunchKernelGGL(k_rows_gather<1>, dim3(gb), dim3(256), 0, s, P, src, start, entries, out); break;
        case 2: hipLaunchKernelGGL(k_rows_gather<2>, dim3(gb), dim3(256), 0, s, P, src, start, entries, out); break;
        case 3: hipLaunchKernelGGL(k_rows_gather<3>, dim3(gb), dim3(256), 0, s, P, src, start, entries, out); break;
        default: hipLaunchKernelGGL(k_rows_gather<4>, dim3(gb), dim3(256), 0, s, P, src, start, entries, out); break;
    }
    return hipGetLastError() == hipSuccess ? 0 : SGR_E_HIP;
}

int sgr_level_set_points(int N, int K, const float* world_points, const int64_t* nbr_idx, const float* cam_center,
                         const float* centers, const float* inv_scaled_rot, const float* strengths,
                         const float* gaussian_std, int n_levels, const float* levels_host, int n_range, float range_size,
                         float density_factor, uint8_t* valid, float* points, float* normals, const float* packed, void* stream)
{
    if (N <= 0) return 0;
    if (K <= 0 || n_levels <= 0 || n_levels > LS_MAX_LEVELS || n_range < 2 || n_range > LS_MAX_RANGE || !world_points ||
        !nbr_idx || !cam_center || !centers || !inv_scaled_rot || !strengths || !gaussian_std || !levels_host || !valid || !points)
        return SGR_E_INVALID;
    LevelArgs la;
    la.n = n_levels;
    for (int i = 0; i < LS_MAX_LEVELS; i++) la.v[i] = i < n_levels ? levels_host[i] : 0.f;
    if (n_range <= 21)
        hipLaunchKernelGGL(k_level_set<21>, dim3((N + 127) / 128), dim3(128), 0, (hipStream_t)stream, N, K, world_points,
                           reinterpret_cast<const long long*>(nbr_idx), cam_center, centers, inv_scaled_rot, strengths, reinterpret_cast<const float4*>(packed), gaussian_std,
                           la, n_range, range_size, density_factor, valid, points, normals);
    else
        hipLaunchKernelGGL(k_level_set<LS_MAX_RANGE>, dim3((N + 127) / 128), dim3(128), 0, (hipStream_t)stream, N, K, world_points,
                           reinterpret_cast<const long long*>(nbr_idx), cam_center, centers, inv_scaled_rot, strengths, reinterpret_cast<const float4*>(packed), gaussian_std,
                           la, n_range, range_size, density_factor, valid, points, normals);
    return hipGetLastError() == hipSuccess ? 0 : SGR_E_HIP;
}

}  // extern "C"
