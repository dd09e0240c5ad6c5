// field.hip -- SuGaR's Gaussian density field and level-set surface sampler as fused gfx950 kernels that read the same
// per-Gaussian buffers as the reference's PyTorch code (centres, inverse-scaled rotations, strengths, k-NN indices).
//
//   density field : sugar_scene/sugar_model.py:1270-1281 (get_field_values) and :1998-2009 (the sampler's copy):
//                     w = B_g^T (x - mu_g);  o_g = f * strength_g * exp(-0.5 * clamp(|w|^2, 0, 1e8));  density = sum_g o_g
//                   with B_g = R_g diag(1 / max(s_g, 1e-8))  (get_covariance(return_full_matrix, return_sqrt, inverse_scales),
//                   :730-736).  The reference materialises [N,16,3,3] and [N,16,3,1] temporaries per call; here one lane
//                   owns one sample and walks its 16 neighbours.
//   backward      : gradients of sum(g_op * o) + sum(g_den * density) w.r.t. x, mu, B, strength (autograd of the above).  The
//                   (sample, neighbour) pairs are grouped by Gaussian (csrc/group.hip) and summed in a fixed order.
//   sdf field     : sugar_scene/sugar_model.py:1247-1307 with beta_mode 'average' (the coarse stage's regulariser,
//                   sugar_trainers/coarse_sdf.py:566-716): the opacities and density above -- the same kernels, template <bool SDF> -- then
//                     d' = density < 1 ? density : density / (density + 1e-12)      (the denominator carries no gradient)
//                     beta = mean_k min_scaling[nbr_k]
//                     sdf = beta * (sqrt(-2 ln max(d', opacity_min_clamp)) - sqrt(-2 ln min(threshold, 1)))
//                   Backward: k_sdf_tail_bwd forms the per-sample gradients of density and beta, the density backward's kernels carry
//                   them on and write dmin_scaling as a fourteenth sum.  Every per-Gaussian row is written, without float atomics.
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

// ---- the SDF of the coarse stage's regulariser (sugar_model.py:1247-1307, beta_mode 'average') on top of the density -----------------
struct TailArgs { float clamp_min, offset; };  // opacity_min_clamp; sqrt(-2 ln min(threshold, 1))

TailArgs tail_args(float density_threshold, float opacity_min_clamp)
{
    const double th = density_threshold < 1.f ? (double)density_threshold : 1.0;
    return TailArgs{opacity_min_clamp, (float)sqrt(-2.0 * log(th))};   // (np.sqrt(-2 np.log(min(threshold, 1))), then float32)
}

__device__ __forceinline__ void sdf_tail(float density, float beta_sum, int K, const TailArgs ta, float& beta, float& sdf)
{
    const float dprime = density < 1.f ? density : density / (density + 1e-12f);
    const float cl = fmaxf(dprime, ta.clamp_min);
    beta = beta_sum / (float)K;
    sdf = beta * (sqrtf(-2.f * logf(cl)) - ta.offset);
}

// ---- the kernel family: template <bool SDF> ---------------------------------------------------------------------------------------
// SDF = false is the density field (sgr_density_field_*): the indices are trusted (the entry points have no P), the arguments
// P, min_scaling, ta, beta, sdf, gB and dmin_scaling are not read.  SDF = true is the SDF field (sgr_sdf_field_*): the same pair
// arithmetic from the same text -- the forward's opacities and densities are the density field's bit for bit
// (tests/test_gpu_field.py: test_sdf_field_carries_the_density_fields_bits; the backward's dx and dstrengths are not) -- and around it
//   * the index wraps once and a neighbour outside [0, P) contributes nothing;
//   * the forward sums min_scaling over the neighbours and appends sdf_tail;
//   * the backward reads the per-sample gradients that k_sdf_tail_bwd formed (g_den = gD, never NULL; gB) and writes dmin_scaling.

// K == 16 (SuGaR's neighbour count): a lane per (sample, neighbour) PAIR, the sixteen pairs of a sample in one DPP row.  The
// lane-per-sample loops below issue their sixteen record gathers one after the other (each waits for its index): 0.54 ms for 16M pairs
// against records that fit the L2; with a lane per pair all gathers of a wave are in flight at once.
template <bool SDF>
__global__ void __launch_bounds__(256) k_density_fwd16(long long NK, int P, const float* __restrict__ x, const long long* __restrict__ nbr,
                                                       const float* __restrict__ centers, const float* __restrict__ B,
                                                       const float* __restrict__ strengths, const float4* __restrict__ packed,
                                                       const float* __restrict__ min_scaling, float factor, TailArgs ta,
                                                       float* __restrict__ opac, float* __restrict__ density, float* __restrict__ beta,
                                                       float* __restrict__ sdf)
{
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= NK) return;   // (NK is a multiple of 16: rows leave whole)
    const size_t n = (size_t)(p >> 4);
    // (the forward runs its pair arithmetic for EVERY lane, on record 0 where the SDF index is out of range, and discards that lane's
    // result: under a divergent branch the compiler pairs the products into packed FP32 and the opacities lose the density field's bits)
    const long long gi = SDF ? wrap_row(nbr[p], P) : nbr[p];
    const bool in = !SDF || (gi >= 0 && gi < P);
    const GaussNbr g = load_nbr(in ? gi : 0, centers, B, strengths, packed);
    float w0, w1, w2;
    bt_mul(g.B, x[3 * n] - g.mx, x[3 * n + 1] - g.my, x[3 * n + 2] - g.mz, w0, w1, w2);
    const float q = fminf(fmaxf(w0 * w0 + w1 * w1 + w2 * w2, 0.f), 1e8f);
    float o = factor * g.s * __expf(-0.5f * q), ms = 0.f;
    if constexpr (SDF) { o = in ? o : 0.f; ms = in ? min_scaling[gi] : 0.f; }
    if (opac) opac[p] = o;
    const float sum = row_sum16(o);
    if constexpr (SDF) {
        const float bsum = row_sum16(ms);
        if ((threadIdx.x & 15) == 0) {
            float b, s;
            sdf_tail(sum, bsum, 16, ta, b, s);
            density[n] = sum; beta[n] = b; sdf[n] = s;
        }
    } else {
        if ((threadIdx.x & 15) == 0) density[n] = sum;
    }
}

// the gradient of the sample positions, same mapping (the per-Gaussian gradients are the gather kernel's)
template <bool SDF>
__global__ void __launch_bounds__(256) k_density_dx16(long long NK, int P, const float* __restrict__ x, const long long* __restrict__ nbr,
                                                      const float* __restrict__ centers, const float* __restrict__ B,
                                                      const float* __restrict__ strengths, const float4* __restrict__ packed, float factor,
                                                      const float* __restrict__ g_opac, const float* __restrict__ g_den,
                                                      float* __restrict__ dx_out)
{
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= NK) return;
    const size_t n = (size_t)(p >> 4);
    const long long gi = SDF ? wrap_row(nbr[p], P) : nbr[p];
    float ax = 0.f, ay = 0.f, az = 0.f;
    if (!SDF || (gi >= 0 && gi < P)) {
        const GaussNbr g = load_nbr(gi, centers, B, strengths, packed);
        float w0, w1, w2;
        bt_mul(g.B, x[3 * n] - g.mx, x[3 * n + 1] - g.my, x[3 * n + 2] - g.mz, w0, w1, w2);
        const float q_raw = w0 * w0 + w1 * w1 + w2 * w2;
        const float e = __expf(-0.5f * fminf(fmaxf(q_raw, 0.f), 1e8f));
        const float go = (g_opac ? g_opac[p] : 0.f) + ((SDF || g_den) ? g_den[n] : 0.f);
        const float dq = (q_raw > 0.f && q_raw < 1e8f) ? -0.5f * factor * g.s * e * go : 0.f;
        const float dw0 = 2.f * w0 * dq, dw1 = 2.f * w1 * dq, dw2 = 2.f * w2 * dq;
        ax = g.B[0] * dw0 + g.B[1] * dw1 + g.B[2] * dw2;
        ay = g.B[3] * dw0 + g.B[4] * dw1 + g.B[5] * dw2;
        az = g.B[6] * dw0 + g.B[7] * dw1 + g.B[8] * dw2;
    }
    ax = row_sum16(ax); ay = row_sum16(ay); az = row_sum16(az);
    if ((threadIdx.x & 15) == 0) { dx_out[3 * n] = ax; dx_out[3 * n + 1] = ay; dx_out[3 * n + 2] = az; }
}

// any K: a lane per sample
template <bool SDF>
__global__ void __launch_bounds__(256) k_density_fwd(int N, int K, int P, const float* __restrict__ x, const long long* __restrict__ nbr,
                                                     const float* __restrict__ centers, const float* __restrict__ B,
                                                     const float* __restrict__ strengths, const float4* __restrict__ packed,
                                                     const float* __restrict__ min_scaling, float factor, TailArgs ta,
                                                     float* __restrict__ opac, float* __restrict__ density, float* __restrict__ beta,
                                                     float* __restrict__ sdf)
{
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const float px = x[3 * (size_t)n], py = x[3 * (size_t)n + 1], pz = x[3 * (size_t)n + 2];
    float sum = 0.f, bsum = 0.f;
    for (int k = 0; k < K; k++) {
        const long long gi = SDF ? wrap_row(nbr[(size_t)n * K + k], P) : nbr[(size_t)n * K + k];
        const bool in = !SDF || (gi >= 0 && gi < P);
        const GaussNbr g = load_nbr(in ? gi : 0, centers, B, strengths, packed);
        float w0, w1, w2;
        bt_mul(g.B, px - g.mx, py - g.my, pz - g.mz, w0, w1, w2);
        const float q = fminf(fmaxf(w0 * w0 + w1 * w1 + w2 * w2, 0.f), 1e8f);
        float o = factor * g.s * __expf(-0.5f * q);
        if constexpr (SDF) { o = in ? o : 0.f; bsum += in ? min_scaling[gi] : 0.f; }
        if (opac) opac[(size_t)n * K + k] = o;
        sum += o;
    }
    if constexpr (SDF) {
        float b, s;
        sdf_tail(sum, bsum, K, ta, b, s);
        beta[n] = b; sdf[n] = s;
    }
    density[n] = sum;
}

template <bool SDF>
__global__ void __launch_bounds__(256) k_density_dx(int N, int K, int P, const float* __restrict__ x, const long long* __restrict__ nbr,
                                                    const float* __restrict__ centers, const float* __restrict__ B,
                                                    const float* __restrict__ strengths, const float4* __restrict__ packed, float factor,
                                                    const float* __restrict__ g_opac, const float* __restrict__ g_den,
                                                    float* __restrict__ dx_out)
{
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const float px = x[3 * (size_t)n], py = x[3 * (size_t)n + 1], pz = x[3 * (size_t)n + 2];
    const float gd = (SDF || g_den) ? g_den[n] : 0.f;
    float ax = 0.f, ay = 0.f, az = 0.f;
    for (int k = 0; k < K; k++) {
        const size_t p = (size_t)n * K + k;
        const long long gi = SDF ? wrap_row(nbr[p], P) : nbr[p];
        if (SDF && (gi < 0 || gi >= P)) continue;
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
    dx_out[3 * (size_t)n] = ax; dx_out[3 * (size_t)n + 1] = ay; dx_out[3 * (size_t)n + 2] = az;
}

// ---- the atomics formulation of the backward, kept for comparison (_DensityField.use_gather = False) -------------------------------

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
// pairs are first laid out per Gaussian -- by sgr_group_by_key (group.hip: stable radix grouping; until the end of round 4, and with
// SGR_GROUP_ATOMICS=1, by ONE returning integer atomic per pair for its rank, a scan and a fill: the two kernels below) -- and sixteen
// lanes per Gaussian then sum its pairs in registers and write its 13 outputs once.  The gradient of the sample positions is
// k_density_dx16 / k_density_dx above.
__global__ void __launch_bounds__(256) k_density_bwd_rank(long long NK, const long long* __restrict__ nbr, uint32_t* __restrict__ cnt,
                                                          uint32_t* __restrict__ rank)
{
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= NK) return;
    rank[p] = atomicAdd(&cnt[nbr[p]], 1u);
}

__global__ void __launch_bounds__(256) k_density_bwd_fill(long long NK, const long long* __restrict__ nbr,
                                                          const uint32_t* __restrict__ start, const uint32_t* __restrict__ rank,
                                                          uint32_t* __restrict__ pair_list)
{
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= NK) return;
    pair_list[start[nbr[p]] + rank[p]] = (uint32_t)p;
}

// SIXTEEN lanes (one DPP row) per Gaussian: they stride over its pairs and fold their 13 partial sums with row rotates (SDF: and
// dmin_scaling as the fourteenth).  (One lane per Gaussian, until round 4, walked its list alone -- 280 dependent gathers on average
// when 1M samples x 16 neighbours meet 57k Gaussians, on 900 waves: 2.0 ms; a trainer's SDF phase has exactly that shape.)
template <bool SDF>
__global__ void __launch_bounds__(256) k_density_bwd_gather(int P, int K, const float* __restrict__ x,
                                                            const float* __restrict__ centers, const float* __restrict__ B,
                                                            const float* __restrict__ strengths, const float4* __restrict__ packed, float factor,
                                                            const float* __restrict__ g_opac, const float* __restrict__ g_den,
                                                            const float* __restrict__ gB, const uint32_t* __restrict__ start,
                                                            const uint32_t* __restrict__ pair_list, float* __restrict__ dcenters,
                                                            float* __restrict__ dB, float* __restrict__ dstrengths,
                                                            float* __restrict__ dmin_scaling)
{
    const int t = (int)(((size_t)blockIdx.x * 256 + threadIdx.x) >> 4);
    const uint32_t sub = threadIdx.x & 15;
    if (t >= P) return;   // (whole rows leave together: the row rotates below never cross a row)
    const GaussNbr g = load_nbr(t, centers, B, strengths, packed);
    float dc0 = 0.f, dc1 = 0.f, dc2 = 0.f, ds = 0.f, dm = 0.f;
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
        const float go = (g_opac ? g_opac[p] : 0.f) + ((SDF || g_den) ? g_den[n] : 0.f);
        ds += go * factor * ex;
        if constexpr (SDF) dm += gB[n];
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
    if constexpr (SDF) dm = row_sum16(dm);
#pragma unroll
    for (int i = 0; i < 9; i++) b[i] = row_sum16(b[i]);
    if (sub == 0) {
        dcenters[3 * (size_t)t] = dc0; dcenters[3 * (size_t)t + 1] = dc1; dcenters[3 * (size_t)t + 2] = dc2;
        dstrengths[t] = ds;
        if constexpr (SDF) dmin_scaling[t] = dm;
    }
    if (sub < 9) {   // nine lanes store the nine entries of dB (each holds all the sums)
        float v = b[0];
#pragma unroll
        for (int i = 1; i < 9; i++) v = (sub == (uint32_t)i) ? b[i] : v;
        dB[9 * (size_t)t + sub] = v;
    }
}

// per sample: the gradient that reaches the density (its own plus the sdf's, through the tail in the reference's operation order:
// mul, sqrt, mul by -2, log, clamp, the division of the rows >= 1) and the gradient per neighbour of min_scaling (beta's / K).
// Rows with density >= 1 carry what float32 autograd gives there (sqrt(0): non-finite).
__global__ void __launch_bounds__(256) k_sdf_tail_bwd(int N, int K, const float* __restrict__ density, const float* __restrict__ beta,
                                                      const float* __restrict__ g_den, const float* __restrict__ g_beta,
                                                      const float* __restrict__ g_sdf, TailArgs ta, float* __restrict__ gD,
                                                      float* __restrict__ gB)
{
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const float D = density[n];
    const bool over = !(D < 1.f);
    const float dprime = over ? D / (D + 1e-12f) : D;
    const float cl = fmaxf(dprime, ta.clamp_min);
    const float r = sqrtf(-2.f * logf(cl));
    float gd = g_den ? g_den[n] : 0.f, gb = g_beta ? g_beta[n] : 0.f;
    if (g_sdf) {
        const float gs = g_sdf[n];
        gb += gs * (r - ta.offset);
        const float gr = gs * beta[n];
        const float gL = gr / (2.f * r);
        float gcl = (gL * -2.f) / cl;
        if (!(dprime >= ta.clamp_min)) gcl = 0.f;      // clamp(min): the gradient passes where the input is >= min
        gd += over ? gcl / (D + 1e-12f) : gcl;
    }
    gD[n] = gd;
    gB[n] = gb / (float)K;
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
    out[g] = view_std_of(g, centers, quats, scaling, cam_center);
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

// ---- SuGaR.get_covariance(return_sqrt=True[, inverse_scales=True]), sugar_scene/sugar_model.py:730-736 ---------------------
// out[a][b] = R(q)[a][b] * s[b],  R = pytorch3d's quaternion_to_matrix (real part first, two_s = 2 / |q|^2: any non-zero q; quat_M of
// sgr_device.h), s = scaling or 1 / clamp(scaling, 1e-8).  The reference builds it with ~25 elementwise launches (plus autograd twins)
// every time the regulariser or the level-set sampler runs.
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

// the forward and the gradient of the sample positions: a lane per pair when K == 16, else a lane per sample
template <bool SDF>
void launch_fwd(int N, int K, int P, const float* x, const long long* nbr, const float* centers, const float* B, const float* strengths,
                const float4* packed, const float* min_scaling, float factor, TailArgs ta, float* opac, float* density, float* beta,
                float* sdf, hipStream_t s)
{
    if (K == 16)
        hipLaunchKernelGGL(k_density_fwd16<SDF>, dim3(blocks256((size_t)N * 16)), dim3(256), 0, s, (long long)N * 16, P, x, nbr, centers, B,
                           strengths, packed, min_scaling, factor, ta, opac, density, beta, sdf);
    else
        hipLaunchKernelGGL(k_density_fwd<SDF>, dim3(blocks256((size_t)N)), dim3(256), 0, s, N, K, P, x, nbr, centers, B, strengths, packed,
                           min_scaling, factor, ta, opac, density, beta, sdf);
}

template <bool SDF>
void launch_dx(int N, int K, int P, const float* x, const long long* nbr, const float* centers, const float* B, const float* strengths,
               const float4* packed, float factor, const float* g_opac, const float* g_den, float* dx_out, hipStream_t s)
{
    if (K == 16)
        hipLaunchKernelGGL(k_density_dx16<SDF>, dim3(blocks256((size_t)N * 16)), dim3(256), 0, s, (long long)N * 16, P, x, nbr, centers, B,
                           strengths, packed, factor, g_opac, g_den, dx_out);
    else
        hipLaunchKernelGGL(k_density_dx<SDF>, dim3(blocks256((size_t)N)), dim3(256), 0, s, N, K, P, x, nbr, centers, B, strengths, packed,
                           factor, g_opac, g_den, dx_out);
}

}  // namespace

extern "C" {

int sgr_density_field_forward(int N, int K, const float* x, const int64_t* nbr_idx, const float* centers,
                              const float* inv_scaled_rot, const float* strengths, float density_factor,
                              float* neighbor_opacities, float* density, const float* packed, void* stream)
{
    if (N <= 0) return 0;
    if (K <= 0 || !x || !nbr_idx || !centers || !inv_scaled_rot || !strengths || !density) return SGR_E_INVALID;
    launch_fwd<false>(N, K, 0, x, reinterpret_cast<const long long*>(nbr_idx), centers, inv_scaled_rot, strengths,
                      reinterpret_cast<const float4*>(packed), nullptr, density_factor, TailArgs{}, neighbor_opacities, density, nullptr,
                      nullptr, (hipStream_t)stream);
    return sgr_launch_status();
}

int sgr_sdf_field_forward(int N, int K, int P, const float* x, const int64_t* nbr_idx, const float* centers, const float* inv_scaled_rot,
                          const float* strengths, const float* min_scaling, float density_factor, float density_threshold,
                          float opacity_min_clamp, float* neighbor_opacities, float* density, float* beta, float* sdf,
                          const float* packed, void* stream)
{
    if (N <= 0) return 0;
    if (K <= 0 || P <= 0 || !x || !nbr_idx || !centers || !inv_scaled_rot || !strengths || !min_scaling || !density || !beta || !sdf ||
        !(density_threshold > 0.f) || misaligned16(packed))
        return SGR_E_INVALID;
    launch_fwd<true>(N, K, P, x, reinterpret_cast<const long long*>(nbr_idx), centers, inv_scaled_rot, strengths,
                     reinterpret_cast<const float4*>(packed), min_scaling, density_factor, tail_args(density_threshold, opacity_min_clamp),
                     neighbor_opacities, density, beta, sdf, (hipStream_t)stream);
    return sgr_launch_status();
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
    return sgr_launch_status();
}

int sgr_scaled_rotation_forward(int P, const float* quaternions, const float* scaling, int inverse_scales, float* out, void* stream)
{
    if (P <= 0) return 0;
    if (!quaternions || !scaling || !out || ((uintptr_t)quaternions & 15)) return SGR_E_INVALID;
    hipLaunchKernelGGL(k_scaled_rotation_fwd, dim3((P + 255) / 256), dim3(256), 0, (hipStream_t)stream, P, quaternions, scaling,
                       inverse_scales, out);
    return sgr_launch_status();
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
    return sgr_launch_status();
}

int sgr_view_depth_rgb(int P, const float* centers, const float* viewmatrix, float* out, void* stream)
{
    if (P <= 0) return 0;
    if (!centers || !viewmatrix || !out) return SGR_E_INVALID;
    hipLaunchKernelGGL(k_view_depth_rgb, dim3((P + 255) / 256), dim3(256), 0, (hipStream_t)stream, P, centers, viewmatrix, out);
    return sgr_launch_status();
}

int sgr_view_std(int P, const float* centers, const float* quaternions, const float* scaling, const float* cam_center, float* out,
                 void* stream)
{
    if (P <= 0) return 0;
    if (!centers || !quaternions || !scaling || !cam_center || !out || ((uintptr_t)quaternions & 15)) return SGR_E_INVALID;
    hipLaunchKernelGGL(k_view_std, dim3((P + 255) / 256), dim3(256), 0, (hipStream_t)stream, P, centers, quaternions, scaling, cam_center,
                       out);
    return sgr_launch_status();
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
    return sgr_launch_status();
}

int sgr_pack_gaussians(int P, const float* centers, const float* inv_scaled_rot, const float* strengths, float* packed, void* stream)
{
    if (P <= 0) return 0;
    if (!centers || !inv_scaled_rot || !strengths || !packed || ((uintptr_t)packed & 15)) return SGR_E_INVALID;
    hipLaunchKernelGGL(k_pack_gaussians, dim3((P + 255) / 256), dim3(256), 0, (hipStream_t)stream, P, centers, inv_scaled_rot,
                       strengths, reinterpret_cast<float4*>(packed));
    return sgr_launch_status();
}

size_t sgr_density_field_backward_scratch_bytes(int N, int K, int P)
{
    return sgr_carve_ranked(nullptr, (size_t)(N > 0 ? N : 0) * (size_t)(K > 0 ? K : 0), P).total;
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
    const size_t nk = (size_t)N * K;
    const SgrRankedScratch sc = sgr_carve_ranked(scratch, nk, P);
    const long long* nbr = reinterpret_cast<const long long*>(nbr_idx);
    const float4* pk = reinterpret_cast<const float4*>(packed);
    const uint32_t* pairs = sc.list;
    if (dL_dx && N > 0)
        launch_dx<false>(N, K, 0, x, nbr, centers, inv_scaled_rot, strengths, pk, density_factor, dL_dopacities, dL_ddensity, dL_dx, s);
    if (sgr_group_by_atomics() || N == 0) {
        if (hipMemsetAsync(sc.cnt, 0, ((size_t)P + 1) * 4, s) != hipSuccess) return SGR_E_HIP;
        if (N > 0) hipLaunchKernelGGL(k_density_bwd_rank, dim3(blocks256(nk)), dim3(256), 0, s, (long long)nk, nbr, sc.cnt, sc.rank);
        sgr_launch_scan(P, sc.cnt, sc.block_sums, sc.start, s);
        if (N > 0) hipLaunchKernelGGL(k_density_bwd_fill, dim3(blocks256(nk)), dim3(256), 0, s, (long long)nk, nbr, sc.start, sc.rank, sc.list);
    } else {
        const int rc = sgr_group_by_key((long long)nk, nbr, P, sc.group, sc.start, &pairs, s);
        if (rc < 0) return rc;
    }
    hipLaunchKernelGGL(k_density_bwd_gather<false>, dim3(blocks256((size_t)P * 16)), dim3(256), 0, s, P, K, x, centers, inv_scaled_rot,
                       strengths, pk, density_factor, dL_dopacities, dL_ddensity, (const float*)nullptr, sc.start, pairs, dL_dcenters,
                       dL_dinv_scaled_rot, dL_dstrengths, (float*)nullptr);
    return sgr_launch_status();
}

size_t sgr_sdf_field_backward_scratch_bytes(int N, int K, int P)
{
    const size_t n = (size_t)(N > 0 ? N : 0), nk = n * (size_t)(K > 0 ? K : 0), p = (size_t)(P > 0 ? P : 0);
    return sgr_align((p + 1) * 4) + 2 * sgr_align(n * 4) + sgr_group_scratch_bytes(nk);   // start | gD | gB | the grouping's buffers
}

int sgr_sdf_field_backward(int N, int K, int P, const float* x, const int64_t* nbr_idx, const float* centers, const float* inv_scaled_rot,
                           const float* strengths, float density_factor, float density_threshold, float opacity_min_clamp,
                           const float* density, const float* beta, const float* dL_dopacities, const float* dL_ddensity,
                           const float* dL_dbeta, const float* dL_dsdf, float* dL_dx, float* dL_dcenters, float* dL_dinv_scaled_rot,
                           float* dL_dstrengths, float* dL_dmin_scaling, char* scratch, const float* packed, void* stream)
{
    if (P <= 0) return 0;
    if (N < 0 || K <= 0 || (N > 0 && (!x || !nbr_idx || !density || !beta)) || !centers || !inv_scaled_rot || !strengths || !dL_dcenters ||
        !dL_dinv_scaled_rot || !dL_dstrengths || !dL_dmin_scaling || !scratch || !(density_threshold > 0.f) || misaligned16(packed) ||
        (size_t)(N > 0 ? N : 0) * K > 0xFFFFFFFFull)
        return SGR_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const TailArgs ta = tail_args(density_threshold, opacity_min_clamp);
    const size_t nk = (size_t)N * K, pa = sgr_align(((size_t)P + 1) * 4), na = sgr_align((size_t)N * 4);
    uint32_t* start = reinterpret_cast<uint32_t*>(scratch);
    float* gD = reinterpret_cast<float*>(scratch + pa);
    float* gB = reinterpret_cast<float*>(scratch + pa + na);
    const long long* nbr = reinterpret_cast<const long long*>(nbr_idx);
    const float4* pk = reinterpret_cast<const float4*>(packed);
    const uint32_t* pairs = nullptr;
    if (N > 0) {
        hipLaunchKernelGGL(k_sdf_tail_bwd, dim3(blocks256((size_t)N)), dim3(256), 0, s, N, K, density, beta, dL_ddensity, dL_dbeta, dL_dsdf,
                           ta, gD, gB);
        if (dL_dx) launch_dx<true>(N, K, P, x, nbr, centers, inv_scaled_rot, strengths, pk, density_factor, dL_dopacities, gD, dL_dx, s);
    }
    const int rc = sgr_group_by_key((long long)nk, nbr, P, scratch + pa + 2 * na, start, &pairs, s);
    if (rc < 0) return rc;
    hipLaunchKernelGGL(k_density_bwd_gather<true>, dim3(blocks256((size_t)P * 16)), dim3(256), 0, s, P, K, x, centers, inv_scaled_rot,
                       strengths, pk, density_factor, dL_dopacities, gD, gB, start, pairs, dL_dcenters, dL_dinv_scaled_rot, dL_dstrengths,
                       dL_dmin_scaling);
    return sgr_launch_status();
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
    return sgr_launch_status();
}

}  // extern "C"
