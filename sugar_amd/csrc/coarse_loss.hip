// coarse_loss.hip -- the loss arithmetic that SuGaR's two coarse trainers write inline inside the SDF regulariser
// (sugar_trainers/coarse_sdf.py:606-716, coarse_density.py:610-730), between the method calls that csrc/sdf_regulariser.hip and
// csrc/field.hip already answer, as gfx950 kernels.  Three operations:
//
//   surface band      : coarse_sdf.py:610-623 (no gradient).  One lane per Gaussian: the centre in camera space, its depth looked up in
//                       the depth map (sgr_depth_lookup.h), std = | s (.) R(q)^T normalize(cam_center - mu) | (view_std_of),
//                       close = |map_z - z| < threshold * std.
//   estimation losses : :644-686.  One lane per sample: c = [x 1] * world_to_view, z = c.z, proj = z > znear, est = map_z(c) - z, then
//                       'sdf'     | sdf - |est| | / s   or its square of the quotient, clamped to clamp_max
//                       'density' | density - exp(-est^2 / 2 / beta^2) |   or the square
//                       on-surface  |est| / s  or the square of the quotient, clamped
//                       each averaged over the projected samples only; M = their count, formed on the device.
//   better normal     : :688-716.  j = knn_idx[sample_idx[n], k]:  c = n_j sign<n_j, n_s>,  w = opac |<x - mu_j, c>| / max(ms_j, 1e-6)^2,
//                       w^ = w / max(sum_k w, 1e-6) (the sum detached),  loss_n = | n_s - sum_k w^_k c_k |^2, averaged over N.
//                       K = 16: one lane per (sample, neighbour) pair, the sixteen pairs of a sample in one DPP row; any other K: one
//                       lane per sample.
//   projection losses : coarse_density.py:651-700 with use_projection_as_estimation (sgr_projection_loss_*).  One lane per sample:
//                       g = sample_idx[n], est = <x - mu_g, n_g> (three products, summed left to right), every sample counts (the
//                       divisor is N), then the 'sdf' / 'density' / on-surface terms above with the one number s as the scale.
//   opacity entropy   : :543-551, the term the loop adds before the regulariser starts.  One lane per Gaussian:
//                       (-o) log(o + 1e-10) - (1 - o) log((1 - o) + 1e-10), averaged over the visible rows; their count is formed on
//                       the device, no visible row gives NaN.  The backward writes every row, zero where invisible.
//
// Reductions: every workgroup writes ONE float64 partial per term into the scratch, one workgroup then adds them in a fixed order and
// divides: no float atomics, the same bits every run.  Per-Gaussian gradients of the better-normal loss: every (sample, neighbour)
// pair and every sample's own Gaussian writes one row of a table, the N (K + 1) rows are grouped by Gaussian (group.hip) and sixteen
// lanes per Gaussian fold them with row rotates -- every row of the output is written, zero where nothing references the Gaussian.
// Per-Gaussian gradients of the projection losses: the per-sample pass leaves only dL/dest_n behind (4 B per sample), the samples are
// grouped by their Gaussian (group.hip, the int64 indices as they are) and ONE lane per Gaussian folds its samples in ascending sample
// order (float64 sums), re-reading x_n:  dL/dmu_g = -n_g sum dest_n,  dL/dn_g = sum dest_n (x_n - mu_g).  No row table: the draw is uniform over the
// Gaussians in view, a few samples each, and a table would write and read back 24 B per sample for what 16 B of gathers give.
// The one output that is NOT reproducible bit for bit is the depth map's gradient of the estimation backward: four float atomic adds
// per sample, as sgr_depth_lookup_backward.
//
// Kinks as torch has them: sign(0) = 0, d|x|/dx = 0 at 0, clamp(max = c) passes its gradient where x <= c, clamp(min = c) where x >= c.
// Indices wrap once when negative; a sample or a neighbour whose index is outside [-P, P) contributes nothing and is never dereferenced.
#include "../../include/sugar_raster.h"
#include "coarse_loss_layout.h"
#include "sgr_depth_lookup.h"
#include "sgr_device.h"
#include "sgr_group.h"

namespace {

enum { CL_SQUARED_EST = 1, CL_SQUARED_SURFACE = 2, CL_WITH_EST = 4, CL_WITH_SURFACE = 8 };   // SGR_CL_* of the header

__device__ __forceinline__ float sgnf(float v) { return (float)(v > 0.f) - (float)(v < 0.f); }
__device__ __forceinline__ float clamp_max(float v, float c) { return v > c ? c : v; }   // (a NaN stays a NaN, as torch.clamp)

// sum of v over the 256 threads of a workgroup in a fixed order, valid in thread 0; every thread must call it
__device__ __forceinline__ double block_sum256(double v, double* s_wave)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    __syncthreads();                                  // (s_wave may still be read from a previous call)
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = v;
    __syncthreads();
    return (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
}

// [x y z 1] * V, divided by its w (pytorch3d's Transform3d.transform_points; w = 1 for a rigid world-to-view matrix)
struct ViewPoint { float h3, x, y, z; };
__device__ __forceinline__ ViewPoint to_view(float X, float Y, float Z, const float* __restrict__ V)
{
    ViewPoint c;
    const float h0 = X * V[0] + Y * V[4] + Z * V[8] + V[12];
    const float h1 = X * V[1] + Y * V[5] + Z * V[9] + V[13];
    const float h2 = X * V[2] + Y * V[6] + Z * V[10] + V[14];
    c.h3 = X * V[3] + Y * V[7] + Z * V[11] + V[15];
    c.x = h0 / c.h3; c.y = h1 / c.h3; c.z = h2 / c.h3;
    return c;
}

// ------------------------------------------------------------------------------------------------------------- surface band
__global__ void __launch_bounds__(256) k_surface_band(int P, const float* __restrict__ points, const float* __restrict__ quats,
                                                      const float* __restrict__ scaling, const float* __restrict__ V,
                                                      const float* __restrict__ cam_center, const float* __restrict__ Pm,
                                                      const float* __restrict__ depth, long long sy, long long sx, int H, int W,
                                                      float threshold, uint8_t* __restrict__ close, float* __restrict__ std_out)
{
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= P) return;
    const ViewPoint c = to_view(points[3 * (size_t)g], points[3 * (size_t)g + 1], points[3 * (size_t)g + 2], V);
    const float map_z = lookup_value(lookup_coords(c.x, c.y, c.z, Pm, H, W), depth, sy, sx, H, W);
    const float sd = view_std_of((size_t)g, points, quats, scaling, cam_center);
    std_out[g] = sd;
    close[g] = fabsf(map_z - c.z) < threshold * sd ? 1 : 0;
}

// -------------------------------------------------------------------------------------------------------- estimation losses
struct EstArgs {
    long long N; int P, flags;
    const float *x, *field, *beta;      // samples[N,3]; sdf[N] ('sdf') or density[N] ('density'); beta[N] ('density' only)
    const long long* idx; const float* std;   // std[idx[n]] is the sample's scale when std != NULL, s_const otherwise
    float s_const, cmax;
    const float *V, *Pm, *znear;        // world_to_view[16], projection[16], znear[1]: on the device
    const float* depth; long long sy, sx; int H, W;
};

struct EstSample { bool proj; ViewPoint c; Lookup L; float est, s; };

__device__ __forceinline__ EstSample est_sample(const EstArgs& a, long long n)
{
    EstSample e;
    e.c = to_view(a.x[3 * n], a.x[3 * n + 1], a.x[3 * n + 2], a.V);
    e.proj = e.c.z > a.znear[0];
    e.s = a.s_const;
    e.est = 0.f;
    if (a.std) {
        const long long i = wrap_row(a.idx[n], a.P);
        if (i < 0 || i >= a.P) e.proj = false;        // (torch raises; here the sample is left out, never a wild read)
        else e.s = a.std[i];
    }
    if (e.proj) {
        e.L = lookup_coords(e.c.x, e.c.y, e.c.z, a.Pm, a.H, a.W);
        e.est = lookup_value(e.L, a.depth, a.sy, a.sx, a.H, a.W) - e.c.z;
    }
    return e;
}

template <bool DENSITY>
__global__ void __launch_bounds__(256) k_estimation_fwd(EstArgs a, double* __restrict__ partial, size_t n_blocks)
{
    __shared__ double s_wave[4];
    const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
    double t_est = 0.0, t_surf = 0.0, t_cnt = 0.0;
    if (n < a.N) {
        const EstSample e = est_sample(a, n);
        if (e.proj) {
            t_cnt = 1.0;
            if (a.flags & CL_WITH_EST) {
                float v;
                if constexpr (DENSITY) {
                    const float b = a.beta[n];
                    const float d = a.field[n] - expf((-0.5f * (e.est * e.est)) / (b * b));
                    v = (a.flags & CL_SQUARED_EST) ? d * d : fabsf(d);
                } else {
                    const float t = a.field[n] - fabsf(e.est);
                    if (a.flags & CL_SQUARED_EST) { const float u = t / e.s; v = u * u; } else v = fabsf(t) / e.s;
                    v = clamp_max(v, a.cmax);
                }
                t_est = (double)v;
            }
            if (a.flags & CL_WITH_SURFACE) {
                float v;
                if (a.flags & CL_SQUARED_SURFACE) { const float u = e.est / e.s; v = u * u; } else v = fabsf(e.est) / e.s;
                t_surf = (double)clamp_max(v, a.cmax);
            }
        }
    }
    t_est = block_sum256(t_est, s_wave);
    t_surf = block_sum256(t_surf, s_wave);
    t_cnt = block_sum256(t_cnt, s_wave);
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = t_est; partial[n_blocks + blockIdx.x] = t_surf; partial[2 * n_blocks + blockIdx.x] = t_cnt;
    }
}

// the ordered pass: one workgroup adds the partials (thread t takes every 256th, then the fixed tree of block_sum256) and divides.
// `count_row` >= 0: the divisor is the sum of that row of partials (written to M_out); otherwise it is `divisor`.  0 / 0 gives the
// NaN of torch's empty mean.
__global__ void __launch_bounds__(256) k_finish_means(const double* __restrict__ partial, size_t n_blocks, int rows, int count_row,
                                                      double divisor, float* __restrict__ out0, float* __restrict__ out1,
                                                      long long* __restrict__ M_out)
{
    __shared__ double s_wave[4];
    double sum[3] = {0.0, 0.0, 0.0};
    for (int r = 0; r < rows; r++) {
        double v = 0.0;
        for (size_t b = threadIdx.x; b < n_blocks; b += 256) v += partial[(size_t)r * n_blocks + b];
        sum[r] = block_sum256(v, s_wave);
    }
    if (threadIdx.x == 0) {
        if (count_row >= 0) { divisor = sum[count_row]; if (M_out) M_out[0] = (long long)divisor; }
        if (out0) out0[0] = (float)(sum[0] / divisor);
        if (out1) out1[0] = (float)(sum[1] / divisor);
    }
}

template <bool DENSITY>
__global__ void __launch_bounds__(256) k_estimation_bwd(EstArgs a, const long long* __restrict__ M, const float* __restrict__ g_est,
                                                        const float* __restrict__ g_surf, float* __restrict__ dfield,
                                                        float* __restrict__ dbeta, float* __restrict__ dx, float* __restrict__ ddepth)
{
    const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
    if (n >= a.N) return;
    const EstSample e = est_sample(a, n);
    float df = 0.f, db = 0.f, dX = 0.f, dY = 0.f, dZ = 0.f;
    if (e.proj) {
        const float Mf = (float)M[0];
        float dest = 0.f;
        if ((a.flags & CL_WITH_EST) && g_est) {
            const float gm = g_est[0] / Mf;                                     // mean
            if constexpr (DENSITY) {
                const float b = a.beta[n];
                const float num = -0.5f * (e.est * e.est), den = b * b;
                const float T = expf(num / den);
                const float d = a.field[n] - T;
                df = (a.flags & CL_SQUARED_EST) ? gm * (2.f * d) : gm * sgnf(d);
                const float da = -df * T;                                       // through exp
                dest += (da / den) * (-0.5f) * (2.f * e.est);
                db = (-da * num / (den * den)) * (2.f * b);
            } else {
                const float t = a.field[n] - fabsf(e.est);
                if (a.flags & CL_SQUARED_EST) {
                    const float u = t / e.s;
                    df = (u * u <= a.cmax) ? (gm * (2.f * u)) / e.s : 0.f;
                } else {
                    df = (fabsf(t) / e.s <= a.cmax) ? (gm / e.s) * sgnf(t) : 0.f;
                }
                dest -= df * sgnf(e.est);
            }
        }
        if ((a.flags & CL_WITH_SURFACE) && g_surf) {
            const float gm = g_surf[0] / Mf;
            if (a.flags & CL_SQUARED_SURFACE) {
                const float u = e.est / e.s;
                if (u * u <= a.cmax) dest += (gm * (2.f * u)) / e.s;
            } else if (fabsf(e.est) / e.s <= a.cmax) {
                dest += (gm / e.s) * sgnf(e.est);
            }
        }
        // est = map_z(c) - c.z
        float gix, giy, dcx, dcy, dcz;
        lookup_value_bwd(e.L, a.depth, a.sy, a.sx, a.H, a.W, dest, ddepth, gix, giy);
        lookup_coords_bwd(e.L, a.Pm, gix, giy, dcx, dcy, dcz);
        dcz -= dest;
        // c = h.xyz / h.w,  h = [x 1] * V
        const float dh0 = dcx / e.c.h3, dh1 = dcy / e.c.h3, dh2 = dcz / e.c.h3;
        const float dh3 = -(e.c.x * dcx + e.c.y * dcy + e.c.z * dcz) / e.c.h3;
        dX = a.V[0] * dh0 + a.V[1] * dh1 + a.V[2] * dh2 + a.V[3] * dh3;
        dY = a.V[4] * dh0 + a.V[5] * dh1 + a.V[6] * dh2 + a.V[7] * dh3;
        dZ = a.V[8] * dh0 + a.V[9] * dh1 + a.V[10] * dh2 + a.V[11] * dh3;
    }
    if (dfield) dfield[n] = df;
    if (DENSITY && dbeta) dbeta[n] = db;
    if (dx) { dx[3 * n] = dX; dx[3 * n + 1] = dY; dx[3 * n + 2] = dZ; }
}

// ------------------------------------------------------------------------------------------------------------ better normal
struct NormalArgs {
    long long N; int K, P;
    const float* x; const long long *idx, *knn;      // samples[N,3], sample_idx[N], knn_idx[P,K]
    const float *normals, *points, *min_scaling;     // [P,3], [P,3], [P]
    const float* opac;                               // [N,K]
};

struct Pair { bool ok; long long j; float sgn, c0, c1, c2, d0, d1, d2, proj, op, ms2, w; };

// the pair (sample n of Gaussian i, neighbour k): everything of :691-707 that belongs to it
__device__ __forceinline__ Pair pair_eval(const NormalArgs& a, long long n, long long i, int k, float X, float Y, float Z, float s0, float s1,
                                          float s2)
{
    Pair p;
    p.j = wrap_row(a.knn[i * a.K + k], a.P);
    p.ok = p.j >= 0 && p.j < a.P;
    p.sgn = p.c0 = p.c1 = p.c2 = p.d0 = p.d1 = p.d2 = p.proj = p.op = p.w = 0.f;
    p.ms2 = 1.f;
    if (!p.ok) return p;
    const size_t j = (size_t)p.j;
    const float n0 = a.normals[3 * j], n1 = a.normals[3 * j + 1], n2 = a.normals[3 * j + 2];
    p.sgn = sgnf(n0 * s0 + n1 * s1 + n2 * s2);
    p.c0 = n0 * p.sgn; p.c1 = n1 * p.sgn; p.c2 = n2 * p.sgn;
    p.d0 = X - a.points[3 * j]; p.d1 = Y - a.points[3 * j + 1]; p.d2 = Z - a.points[3 * j + 2];
    p.proj = p.d0 * p.c0 + p.d1 * p.c1 + p.d2 * p.c2;
    const float ms = fmaxf(a.min_scaling[j], 1e-6f);
    p.ms2 = ms * ms;
    p.op = a.opac[n * a.K + k];
    p.w = (p.op * fabsf(p.proj)) / p.ms2;
    return p;
}

struct SampleHead { bool ok; long long i; float X, Y, Z, s0, s1, s2; };
__device__ __forceinline__ SampleHead sample_head(const NormalArgs& a, long long n)
{
    SampleHead h;
    h.i = wrap_row(a.idx[n], a.P);
    h.ok = h.i >= 0 && h.i < a.P;
    h.X = a.x[3 * n]; h.Y = a.x[3 * n + 1]; h.Z = a.x[3 * n + 2];
    h.s0 = h.s1 = h.s2 = 0.f;
    if (h.ok) { h.s0 = a.normals[3 * h.i]; h.s1 = a.normals[3 * h.i + 1]; h.s2 = a.normals[3 * h.i + 2]; }
    return h;
}

// K = 16: lane = (sample, neighbour); 16 samples per workgroup
__global__ void __launch_bounds__(256) k_normal_fwd16(NormalArgs a, double* __restrict__ partial)
{
    __shared__ double s_wave[4];
    const long long n = (long long)blockIdx.x * 16 + (threadIdx.x >> 4);
    const int k = threadIdx.x & 15;
    double term = 0.0;
    if (n < a.N) {                                    // (whole rows take the branch together: the row rotates never cross a row)
        const SampleHead h = sample_head(a, n);
        Pair p; p.w = p.c0 = p.c1 = p.c2 = 0.f;
        if (h.ok) p = pair_eval(a, n, h.i, k, h.X, h.Y, h.Z, h.s0, h.s1, h.s2);
        const float wh = p.w / fmaxf(row_sum16(p.w), 1e-6f);
        const float r0 = h.s0 - row_sum16(wh * p.c0), r1 = h.s1 - row_sum16(wh * p.c1), r2 = h.s2 - row_sum16(wh * p.c2);
        if (k == 0 && h.ok) term = (double)(r0 * r0 + r1 * r1 + r2 * r2);
    }
    term = block_sum256(term, s_wave);
    if (threadIdx.x == 0) partial[blockIdx.x] = term;
}

// the residual r = n_s - sum_k w^_k c_k and max(sum w, 1e-6) of one sample, by one lane (any K)
__device__ __forceinline__ void sample_residual(const NormalArgs& a, long long n, const SampleHead& h, float& den, float& r0, float& r1,
                                                float& r2)
{
    float S = 0.f;
    for (int k = 0; k < a.K; k++) S += pair_eval(a, n, h.i, k, h.X, h.Y, h.Z, h.s0, h.s1, h.s2).w;
    den = fmaxf(S, 1e-6f);
    float m0 = 0.f, m1 = 0.f, m2 = 0.f;
    for (int k = 0; k < a.K; k++) {
        const Pair p = pair_eval(a, n, h.i, k, h.X, h.Y, h.Z, h.s0, h.s1, h.s2);
        const float wh = p.w / den;
        m0 += wh * p.c0; m1 += wh * p.c1; m2 += wh * p.c2;
    }
    r0 = h.s0 - m0; r1 = h.s1 - m1; r2 = h.s2 - m2;
}

__global__ void __launch_bounds__(256) k_normal_fwd(NormalArgs a, double* __restrict__ partial)
{
    __shared__ double s_wave[4];
    const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
    double term = 0.0;
    if (n < a.N) {
        const SampleHead h = sample_head(a, n);
        if (h.ok) {
            float den, r0, r1, r2;
            sample_residual(a, n, h, den, r0, r1, r2);
            term = (double)(r0 * r0 + r1 * r1 + r2 * r2);
        }
    }
    term = block_sum256(term, s_wave);
    if (threadIdx.x == 0) partial[blockIdx.x] = term;
}

// what a pair hands to its neighbour Gaussian: the row {dL/dn_j (, dL/dmu_j)} of entry n (K + 1) + k and the entry's key; returns the
// pair's share of dL/dx.  (dm0..2 = dL/d(sum_k w^_k c_k) = -dL/dr.)
template <bool ONLY>
__device__ __forceinline__ void pair_backward(const NormalArgs& a, const Pair& p, float den, float dm0, float dm1, float dm2, size_t e,
                                              long long* __restrict__ keys, float* __restrict__ rows, float& dX, float& dY, float& dZ)
{
    constexpr int WD = ONLY ? 3 : 6;
    const float wh = p.w / den;
    float dc0 = wh * dm0, dc1 = wh * dm1, dc2 = wh * dm2;
    dX = dY = dZ = 0.f;
    float dmu0 = 0.f, dmu1 = 0.f, dmu2 = 0.f;
    if constexpr (!ONLY) {
        const float dwh = p.c0 * dm0 + p.c1 * dm1 + p.c2 * dm2;
        const float dproj = (((dwh / den) / p.ms2) * p.op) * sgnf(p.proj);     // w^ = w / den (den detached), w = (op |proj|) / ms2
        dc0 += dproj * p.d0; dc1 += dproj * p.d1; dc2 += dproj * p.d2;
        dX = dproj * p.c0; dY = dproj * p.c1; dZ = dproj * p.c2;
        dmu0 = -dX; dmu1 = -dY; dmu2 = -dZ;
    }
    keys[e] = p.ok ? p.j : (long long)a.P;                                     // (a key of P is outside [-P, P): the grouping leaves it out)
    rows[e * WD] = p.sgn * dc0; rows[e * WD + 1] = p.sgn * dc1; rows[e * WD + 2] = p.sgn * dc2;
    if constexpr (!ONLY) { rows[e * WD + 3] = dmu0; rows[e * WD + 4] = dmu1; rows[e * WD + 5] = dmu2; }
}

// the sample's own entry n (K + 1) + K: dL/dn_s = dL/dr
template <bool ONLY>
__device__ __forceinline__ void self_entry(const NormalArgs& a, const SampleHead& h, float dr0, float dr1, float dr2, size_t e,
                                           long long* __restrict__ keys, float* __restrict__ rows)
{
    constexpr int WD = ONLY ? 3 : 6;
    keys[e] = h.ok ? h.i : (long long)a.P;
    rows[e * WD] = dr0; rows[e * WD + 1] = dr1; rows[e * WD + 2] = dr2;
    if constexpr (!ONLY) { rows[e * WD + 3] = 0.f; rows[e * WD + 4] = 0.f; rows[e * WD + 5] = 0.f; }
}

template <bool ONLY>
__global__ void __launch_bounds__(256) k_normal_bwd16(NormalArgs a, const float* __restrict__ g, long long* __restrict__ keys,
                                                      float* __restrict__ rows, float* __restrict__ dx)
{
    const long long n = (long long)blockIdx.x * 16 + (threadIdx.x >> 4);
    const int k = threadIdx.x & 15;
    if (n >= a.N) return;                             // (whole rows leave together)
    const SampleHead h = sample_head(a, n);
    Pair p; p.ok = false; p.j = 0; p.sgn = p.w = p.c0 = p.c1 = p.c2 = p.d0 = p.d1 = p.d2 = p.proj = p.op = 0.f; p.ms2 = 1.f;
    if (h.ok) p = pair_eval(a, n, h.i, k, h.X, h.Y, h.Z, h.s0, h.s1, h.s2);
    const float den = fmaxf(row_sum16(p.w), 1e-6f);
    const float wh = p.w / den;
    const float r0 = h.s0 - row_sum16(wh * p.c0), r1 = h.s1 - row_sum16(wh * p.c1), r2 = h.s2 - row_sum16(wh * p.c2);
    const float gm = h.ok ? g[0] / (float)a.N : 0.f;
    const float dr0 = gm * (2.f * r0), dr1 = gm * (2.f * r1), dr2 = gm * (2.f * r2);
    const size_t e = (size_t)n * 17 + k;
    float dX, dY, dZ;
    pair_backward<ONLY>(a, p, den, -dr0, -dr1, -dr2, e, keys, rows, dX, dY, dZ);
    if constexpr (!ONLY) { dX = row_sum16(dX); dY = row_sum16(dY); dZ = row_sum16(dZ); }
    if (k == 0) {
        self_entry<ONLY>(a, h, dr0, dr1, dr2, (size_t)n * 17 + 16, keys, rows);
        if (!ONLY && dx) { dx[3 * n] = dX; dx[3 * n + 1] = dY; dx[3 * n + 2] = dZ; }
    }
}

template <bool ONLY>
__global__ void __launch_bounds__(256) k_normal_bwd(NormalArgs a, const float* __restrict__ g, long long* __restrict__ keys,
                                                    float* __restrict__ rows, float* __restrict__ dx)
{
    const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
    if (n >= a.N) return;
    const SampleHead h = sample_head(a, n);
    const size_t e0 = (size_t)n * (size_t)(a.K + 1);
    float den = 1.f, r0 = 0.f, r1 = 0.f, r2 = 0.f;
    if (h.ok) sample_residual(a, n, h, den, r0, r1, r2);
    const float gm = h.ok ? g[0] / (float)a.N : 0.f;
    const float dr0 = gm * (2.f * r0), dr1 = gm * (2.f * r1), dr2 = gm * (2.f * r2);
    float sX = 0.f, sY = 0.f, sZ = 0.f;
    for (int k = 0; k < a.K; k++) {
        Pair p; p.ok = false; p.j = 0; p.sgn = p.w = p.c0 = p.c1 = p.c2 = p.d0 = p.d1 = p.d2 = p.proj = p.op = 0.f; p.ms2 = 1.f;
        if (h.ok) p = pair_eval(a, n, h.i, k, h.X, h.Y, h.Z, h.s0, h.s1, h.s2);
        float dX, dY, dZ;
        pair_backward<ONLY>(a, p, den, -dr0, -dr1, -dr2, e0 + k, keys, rows, dX, dY, dZ);
        sX += dX; sY += dY; sZ += dZ;
    }
    self_entry<ONLY>(a, h, dr0, dr1, dr2, e0 + a.K, keys, rows);
    if (!ONLY && dx) { dx[3 * n] = sX; dx[3 * n + 1] = sY; dx[3 * n + 2] = sZ; }
}

// SIXTEEN lanes per Gaussian add the rows of its entries (every sixteenth each) and fold with row rotates, as k_density_bwd_gather
template <int WD>
__global__ void __launch_bounds__(256) k_normal_rows_gather(int P, const float* __restrict__ rows, const uint32_t* __restrict__ start,
                                                            const uint32_t* __restrict__ list, float* __restrict__ dnormals,
                                                            float* __restrict__ dpoints)
{
    const int t = (int)(((size_t)blockIdx.x * 256 + threadIdx.x) >> 4);
    const uint32_t sub = threadIdx.x & 15;
    if (t >= P) return;   // (whole rows leave together)
    float acc[WD];
#pragma unroll
    for (int c = 0; c < WD; c++) acc[c] = 0.f;
    const uint32_t e0 = start[t], e1 = start[t + 1];
    for (uint32_t e = e0 + sub; e < e1; e += 16) {
        const float* r = rows + (size_t)list[e] * WD;
#pragma unroll
        for (int c = 0; c < WD; c++) acc[c] += r[c];
    }
#pragma unroll
    for (int c = 0; c < WD; c++) acc[c] = row_sum16(acc[c]);
    if (sub == 0) {
        dnormals[3 * (size_t)t] = acc[0]; dnormals[3 * (size_t)t + 1] = acc[1]; dnormals[3 * (size_t)t + 2] = acc[2];
        if constexpr (WD == 6) { dpoints[3 * (size_t)t] = acc[3]; dpoints[3 * (size_t)t + 1] = acc[4]; dpoints[3 * (size_t)t + 2] = acc[5]; }
    }
}

// -------------------------------------------------------------------------------------------------------- projection losses
struct ProjArgs {
    long long N; int P, flags;
    const float* x; const long long* idx;            // samples[N,3], sample_idx[N]
    const float *points, *normals;                   // [P,3], [P,3]
    const float *field, *beta;                       // sdf[N] ('sdf') or density[N] ('density'); beta[N] ('density' only)
    float s, cmax;
};

struct ProjSample { bool ok; float n0, n1, n2, est; };

// est = <x - mu_g, n_g> of coarse_density.py:655-656; a sample whose index is outside [-P, P) is left out, never dereferenced
__device__ __forceinline__ ProjSample proj_sample(const ProjArgs& a, long long n)
{
    ProjSample e;
    const long long i = wrap_row(a.idx[n], a.P);
    e.ok = i >= 0 && i < a.P;
    e.n0 = e.n1 = e.n2 = e.est = 0.f;
    if (e.ok) {
        e.n0 = a.normals[3 * i]; e.n1 = a.normals[3 * i + 1]; e.n2 = a.normals[3 * i + 2];
        const float d0 = a.x[3 * n] - a.points[3 * i], d1 = a.x[3 * n + 1] - a.points[3 * i + 1], d2 = a.x[3 * n + 2] - a.points[3 * i + 2];
        e.est = (d0 * e.n0 + d1 * e.n1) + d2 * e.n2;
    }
    return e;
}

template <bool DENSITY>
__global__ void __launch_bounds__(256) k_projection_fwd(ProjArgs a, double* __restrict__ partial, size_t n_blocks)
{
    __shared__ double s_wave[4];
    const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
    double t_est = 0.0, t_surf = 0.0;
    if (n < a.N) {
        const ProjSample e = proj_sample(a, n);
        if (e.ok) {
            if (a.flags & CL_WITH_EST) {
                float v;
                if constexpr (DENSITY) {
                    const float b = a.beta[n];
                    const float d = a.field[n] - expf((-0.5f * (e.est * e.est)) / (b * b));
                    v = (a.flags & CL_SQUARED_EST) ? d * d : fabsf(d);
                } else {
                    const float t = a.field[n] - fabsf(e.est);
                    if (a.flags & CL_SQUARED_EST) { const float u = t / a.s; v = u * u; } else v = fabsf(t) / a.s;
                    v = clamp_max(v, a.cmax);
                }
                t_est = (double)v;
            }
            if (a.flags & CL_WITH_SURFACE) {
                float v;
                if (a.flags & CL_SQUARED_SURFACE) { const float u = e.est / a.s; v = u * u; } else v = fabsf(e.est) / a.s;
                t_surf = (double)clamp_max(v, a.cmax);
            }
        }
    }
    t_est = block_sum256(t_est, s_wave);
    t_surf = block_sum256(t_surf, s_wave);
    if (threadIdx.x == 0) { partial[blockIdx.x] = t_est; partial[n_blocks + blockIdx.x] = t_surf; }
}

// the per-sample pass: dfield, dbeta, dsamples = dest n_g, and dest itself for the fold
template <bool DENSITY>
__global__ void __launch_bounds__(256) k_projection_bwd(ProjArgs a, const float* __restrict__ g_est, const float* __restrict__ g_surf,
                                                        float* __restrict__ dfield, float* __restrict__ dbeta, float* __restrict__ dx,
                                                        float* __restrict__ dest_out)
{
    const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
    if (n >= a.N) return;
    const ProjSample e = proj_sample(a, n);
    float df = 0.f, db = 0.f, dest = 0.f;
    if (e.ok) {
        const float Nf = (float)a.N;
        if ((a.flags & CL_WITH_EST) && g_est) {
            const float gm = g_est[0] / Nf;                                     // mean
            if constexpr (DENSITY) {
                const float b = a.beta[n];
                const float num = -0.5f * (e.est * e.est), den = b * b;
                const float T = expf(num / den);
                const float d = a.field[n] - T;
                df = (a.flags & CL_SQUARED_EST) ? gm * (2.f * d) : gm * sgnf(d);
                const float da = -df * T;                                       // through exp
                if (da != 0.f) {                                                // (a target that underflowed passes nothing: no 0 / 0 at a tiny beta)
                    dest += (da / den) * (-0.5f) * (2.f * e.est);
                    db = (-da * num / (den * den)) * (2.f * b);
                }
            } else {
                const float t = a.field[n] - fabsf(e.est);
                if (a.flags & CL_SQUARED_EST) {
                    const float u = t / a.s;
                    df = (u * u <= a.cmax) ? (gm * (2.f * u)) / a.s : 0.f;
                } else {
                    df = (fabsf(t) / a.s <= a.cmax) ? (gm / a.s) * sgnf(t) : 0.f;
                }
                dest -= df * sgnf(e.est);
            }
        }
        if ((a.flags & CL_WITH_SURFACE) && g_surf) {
            const float gm = g_surf[0] / Nf;
            if (a.flags & CL_SQUARED_SURFACE) {
                const float u = e.est / a.s;
                if (u * u <= a.cmax) dest += (gm * (2.f * u)) / a.s;
            } else if (fabsf(e.est) / a.s <= a.cmax) {
                dest += (gm / a.s) * sgnf(e.est);
            }
        }
    }
    if (dfield) dfield[n] = df;
    if (DENSITY && dbeta) dbeta[n] = db;
    if (dx) { dx[3 * n] = dest * e.n0; dx[3 * n + 1] = dest * e.n1; dx[3 * n + 2] = dest * e.n2; }
    if (dest_out) dest_out[n] = dest;
}

// ONE lane per Gaussian folds its samples in ascending sample order; every row is written
__global__ void __launch_bounds__(256) k_projection_fold(int P, const float* __restrict__ x, const float* __restrict__ points,
                                                         const float* __restrict__ normals, const float* __restrict__ dest,
                                                         const uint32_t* __restrict__ start, const uint32_t* __restrict__ list,
                                                         float* __restrict__ dpoints, float* __restrict__ dnormals)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= P) return;
    const uint32_t e0 = start[t], e1 = start[t + 1];
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, m0 = 0.f, m1 = 0.f, m2 = 0.f;
    if (e1 > e0) {
        // float64 sums: the signed dest_n of one Gaussian cancel (samples on either side of its plane), and a float32 running sum would
        // lose against the per-sample values what the cancellation amplifies; the adds are few and the pass is bound by its gathers
        const float u0 = points[3 * t], u1 = points[3 * t + 1], u2 = points[3 * t + 2];
        double S = 0.0, A0 = 0.0, A1 = 0.0, A2 = 0.0;
        for (uint32_t e = e0; e < e1; e++) {
            const size_t n = list[e];
            const double d = (double)dest[n];
            S += d;
            A0 += d * (double)(x[3 * n] - u0); A1 += d * (double)(x[3 * n + 1] - u1); A2 += d * (double)(x[3 * n + 2] - u2);
        }
        a0 = (float)A0; a1 = (float)A1; a2 = (float)A2;
        m0 = (float)(-((double)normals[3 * t] * S)); m1 = (float)(-((double)normals[3 * t + 1] * S));
        m2 = (float)(-((double)normals[3 * t + 2] * S));
    }
    if (dpoints) { dpoints[3 * t] = m0; dpoints[3 * t + 1] = m1; dpoints[3 * t + 2] = m2; }
    if (dnormals) { dnormals[3 * t] = a0; dnormals[3 * t + 1] = a1; dnormals[3 * t + 2] = a2; }
}

bool proj_args_ok(const ProjArgs& a, int mode)
{
    return a.N > 0 && (unsigned long long)a.N < 0xFFFFFFFFull && a.P > 0 && (mode == 0 || mode == 1) && a.x && a.idx && a.points &&
           a.normals && (!(a.flags & CL_WITH_EST) || (a.field && (mode == 0 || a.beta))) && (a.flags & (CL_WITH_EST | CL_WITH_SURFACE)) &&
           !(a.flags & ~15);
}

// ---------------------------------------------------------------------------------------------------------- opacity entropy
// coarse_sdf.py:548-551 for one row, in the trainer's operation order: (-o) log(o + 1e-10) - (1 - o) log((1 - o) + 1e-10)
__global__ void __launch_bounds__(256) k_entropy_fwd(int P, const float* __restrict__ opac, const uint8_t* __restrict__ visible,
                                                     double* __restrict__ partial, size_t n_blocks)
{
    __shared__ double s_wave[4];
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;   // (P up to 2^31 - 1: the last workgroup's rows do not wrap)
    double t_sum = 0.0, t_cnt = 0.0;
    if (g < P && visible[g]) {
        const float o = opac[g], b = 1.f - o;
        t_sum = (double)((-o) * logf(o + 1e-10f) - b * logf(b + 1e-10f));
        t_cnt = 1.0;
    }
    t_sum = block_sum256(t_sum, s_wave);
    t_cnt = block_sum256(t_cnt, s_wave);
    if (threadIdx.x == 0) { partial[blockIdx.x] = t_sum; partial[n_blocks + blockIdx.x] = t_cnt; }
}

// every row is written: (g / n_visible) d/do of the row's term where visible, zero elsewhere
__global__ void __launch_bounds__(256) k_entropy_bwd(int P, const float* __restrict__ opac, const uint8_t* __restrict__ visible,
                                                     const long long* __restrict__ n_visible, const float* __restrict__ g_loss,
                                                     float* __restrict__ dopac)
{
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;   // (P up to 2^31 - 1: the last workgroup's rows do not wrap)
    if (g >= P) return;
    float d = 0.f;
    if (visible[g]) {
        const float gm = g_loss[0] / (float)n_visible[0];
        const float o = opac[g], b = 1.f - o, a = o + 1e-10f, c = b + 1e-10f;
        // first term: d/do [(-o) log a] = -log a - o / a;   second: d/do [-(b log c)] = log c + b / c
        d = (-gm * logf(a) + (gm * (-o)) / a) + (gm * logf(c) + (gm * b) / c);
    }
    dopac[g] = d;
}

bool est_args_ok(const EstArgs& a, int mode)
{
    return a.N > 0 && (unsigned long long)a.N <= 0xFFFFFFFFull && (mode == 0 || mode == 1) && a.x && a.V && a.Pm && a.znear && a.depth &&
           a.H >= 1 && a.W >= 1 && a.sy >= 0 && a.sx >= 0 && (!(a.flags & CL_WITH_EST) || (a.field && (mode == 0 || a.beta))) &&
           (!a.std || (a.idx && a.P > 0)) && (a.flags & (CL_WITH_EST | CL_WITH_SURFACE)) && !(a.flags & ~15);
}

}  // namespace

extern "C" {

int sgr_surface_band(int P, const float* points, const float* quaternions, const float* scaling, const float* world_to_view,
                     const float* cam_center, const float* projection, const float* depth, long long stride_y, long long stride_x,
                     int height, int width, float threshold, uint8_t* close, float* std_out, void* stream)
{
    if (P <= 0) return 0;
    if (!points || !quaternions || !scaling || !world_to_view || !cam_center || !projection || !depth || !close || !std_out ||
        misaligned16(quaternions) || height < 1 || width < 1 || stride_y < 0 || stride_x < 0)
        return SGR_E_INVALID;
    hipLaunchKernelGGL(k_surface_band, dim3(blocks256((size_t)P)), dim3(256), 0, (hipStream_t)stream, P, points, quaternions, scaling,
                       world_to_view, cam_center, projection, depth, stride_y, stride_x, height, width, threshold, close, std_out);
    return sgr_launch_status();
}

size_t sgr_estimation_loss_scratch_bytes(long long N) { return cl_estimation_scratch_bytes(N); }

int sgr_estimation_loss_forward(long long N, int P, int mode, int flags, const float* samples, const float* field, const float* beta,
                                const int64_t* sample_idx, const float* std, float scale, float clamp_max, const float* world_to_view,
                                const float* projection, const float* znear, const float* depth, long long stride_y, long long stride_x,
                                int height, int width, float* loss_estimation, float* loss_surface, int64_t* n_projected, char* scratch,
                                void* stream)
{
    const EstArgs a{N, P, flags, samples, field, beta, reinterpret_cast<const long long*>(sample_idx), std, scale, clamp_max,
                    world_to_view, projection, znear, depth, stride_y, stride_x, height, width};
    if (!est_args_ok(a, mode) || !scratch || ((flags & CL_WITH_EST) && !loss_estimation) || ((flags & CL_WITH_SURFACE) && !loss_surface))
        return SGR_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const size_t nb = cl_estimation_blocks(N);
    double* partial = reinterpret_cast<double*>(scratch);
    if (mode == 1) hipLaunchKernelGGL(k_estimation_fwd<true>, dim3((unsigned)nb), dim3(256), 0, s, a, partial, nb);
    else hipLaunchKernelGGL(k_estimation_fwd<false>, dim3((unsigned)nb), dim3(256), 0, s, a, partial, nb);
    hipLaunchKernelGGL(k_finish_means, dim3(1), dim3(256), 0, s, partial, nb, 3, 2, 0.0, (flags & CL_WITH_EST) ? loss_estimation : nullptr,
                       (flags & CL_WITH_SURFACE) ? loss_surface : nullptr, reinterpret_cast<long long*>(n_projected));
    return sgr_launch_status();
}

int sgr_estimation_loss_backward(long long N, int P, int mode, int flags, const float* samples, const float* field, const float* beta,
                                 const int64_t* sample_idx, const float* std, float scale, float clamp_max, const float* world_to_view,
                                 const float* projection, const float* znear, const float* depth, long long stride_y, long long stride_x,
                                 int height, int width, const int64_t* n_projected, const float* dL_dloss_estimation,
                                 const float* dL_dloss_surface, float* dL_dfield, float* dL_dbeta, float* dL_dsamples, float* dL_ddepth,
                                 void* stream)
{
    const EstArgs a{N, P, flags, samples, field, beta, reinterpret_cast<const long long*>(sample_idx), std, scale, clamp_max,
                    world_to_view, projection, znear, depth, stride_y, stride_x, height, width};
    if (!est_args_ok(a, mode) || !n_projected) return SGR_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    if (dL_ddepth && hipMemsetAsync(dL_ddepth, 0, (size_t)height * width * 4, s) != hipSuccess) return SGR_E_HIP;
    const long long* M = reinterpret_cast<const long long*>(n_projected);
    if (mode == 1)
        hipLaunchKernelGGL(k_estimation_bwd<true>, dim3(blocks256((size_t)N)), dim3(256), 0, s, a, M, dL_dloss_estimation, dL_dloss_surface,
                           dL_dfield, dL_dbeta, dL_dsamples, dL_ddepth);
    else
        hipLaunchKernelGGL(k_estimation_bwd<false>, dim3(blocks256((size_t)N)), dim3(256), 0, s, a, M, dL_dloss_estimation, dL_dloss_surface,
                           dL_dfield, dL_dbeta, dL_dsamples, dL_ddepth);
    return sgr_launch_status();
}

size_t sgr_projection_loss_scratch_bytes(long long N) { return cl_projection_fwd_scratch_bytes(N); }

int sgr_projection_loss_forward(long long N, int P, int mode, int flags, const float* samples, const int64_t* sample_idx, const float* points,
                                const float* normals, const float* field, const float* beta, float scale, float clamp_max,
                                float* loss_estimation, float* loss_surface, char* scratch, void* stream)
{
    const ProjArgs a{N, P, flags, samples, reinterpret_cast<const long long*>(sample_idx), points, normals, field, beta, scale, clamp_max};
    if (!proj_args_ok(a, mode) || !scratch || ((flags & CL_WITH_EST) && !loss_estimation) || ((flags & CL_WITH_SURFACE) && !loss_surface))
        return SGR_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const size_t nb = cl_estimation_blocks(N);
    double* partial = reinterpret_cast<double*>(scratch);
    if (mode == 1) hipLaunchKernelGGL(k_projection_fwd<true>, dim3((unsigned)nb), dim3(256), 0, s, a, partial, nb);
    else hipLaunchKernelGGL(k_projection_fwd<false>, dim3((unsigned)nb), dim3(256), 0, s, a, partial, nb);
    hipLaunchKernelGGL(k_finish_means, dim3(1), dim3(256), 0, s, partial, nb, 2, -1, (double)N, (flags & CL_WITH_EST) ? loss_estimation : nullptr,
                       (flags & CL_WITH_SURFACE) ? loss_surface : nullptr, nullptr);
    return sgr_launch_status();
}

size_t sgr_projection_loss_backward_scratch_bytes(long long N, int P)
{
    if (N <= 0 || (unsigned long long)N >= 0xFFFFFFFFull) return 0;
    return cl_projection_bwd_layout((size_t)N, P, sgr_group_scratch_bytes((size_t)N)).total;
}

int sgr_projection_loss_backward(long long N, int P, int mode, int flags, const float* samples, const int64_t* sample_idx, const float* points,
                                 const float* normals, const float* field, const float* beta, float scale, float clamp_max,
                                 const float* dL_dloss_estimation, const float* dL_dloss_surface, float* dL_dfield, float* dL_dbeta,
                                 float* dL_dsamples, float* dL_dpoints, float* dL_dnormals, char* scratch, void* stream)
{
    const ProjArgs a{N, P, flags, samples, reinterpret_cast<const long long*>(sample_idx), points, normals, field, beta, scale, clamp_max};
    if (!proj_args_ok(a, mode) || !scratch) return SGR_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const ClProjectionBwdLayout L = cl_projection_bwd_layout((size_t)N, P, sgr_group_scratch_bytes((size_t)N));
    const bool fold = dL_dpoints || dL_dnormals;
    float* dest = fold ? reinterpret_cast<float*>(scratch + L.dest) : nullptr;
    if (mode == 1)
        hipLaunchKernelGGL(k_projection_bwd<true>, dim3(blocks256((size_t)N)), dim3(256), 0, s, a, dL_dloss_estimation, dL_dloss_surface,
                           dL_dfield, dL_dbeta, dL_dsamples, dest);
    else
        hipLaunchKernelGGL(k_projection_bwd<false>, dim3(blocks256((size_t)N)), dim3(256), 0, s, a, dL_dloss_estimation, dL_dloss_surface,
                           dL_dfield, dL_dbeta, dL_dsamples, dest);
    if (fold) {
        uint32_t* start = reinterpret_cast<uint32_t*>(scratch + L.start);
        const uint32_t* list = nullptr;
        const int rc = sgr_group_by_key(N, a.idx, P, scratch + L.group, start, &list, s);
        if (rc < 0) return rc;
        hipLaunchKernelGGL(k_projection_fold, dim3(blocks256((size_t)P)), dim3(256), 0, s, P, samples, points, normals, dest, start, list,
                           dL_dpoints, dL_dnormals);
    }
    return sgr_launch_status();
}

size_t sgr_opacity_entropy_scratch_bytes(int P) { return cl_entropy_scratch_bytes(P); }

int sgr_opacity_entropy_forward(int P, const float* opacities, const uint8_t* visible, float* loss, int64_t* n_visible, char* scratch,
                                void* stream)
{
    if (P <= 0 || !opacities || !visible || !loss || !n_visible || !scratch) return SGR_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const size_t nb = cl_blocks((size_t)P, 256);
    double* partial = reinterpret_cast<double*>(scratch);
    hipLaunchKernelGGL(k_entropy_fwd, dim3((unsigned)nb), dim3(256), 0, s, P, opacities, visible, partial, nb);
    hipLaunchKernelGGL(k_finish_means, dim3(1), dim3(256), 0, s, partial, nb, 2, 1, 0.0, loss, nullptr, reinterpret_cast<long long*>(n_visible));
    return sgr_launch_status();
}

int sgr_opacity_entropy_backward(int P, const float* opacities, const uint8_t* visible, const int64_t* n_visible, const float* dL_dloss,
                                 float* dL_dopacities, void* stream)
{
    if (P <= 0 || !opacities || !visible || !n_visible || !dL_dloss || !dL_dopacities) return SGR_E_INVALID;
    hipLaunchKernelGGL(k_entropy_bwd, dim3(blocks256((size_t)P)), dim3(256), 0, (hipStream_t)stream, P, opacities, visible,
                       reinterpret_cast<const long long*>(n_visible), dL_dloss, dL_dopacities);
    return sgr_launch_status();
}

size_t sgr_better_normal_forward_scratch_bytes(long long N, int K) { return cl_normal_fwd_scratch_bytes(N, K); }

static bool normal_args_ok(const NormalArgs& a)
{
    size_t entries;
    return a.N > 0 && a.K >= 1 && a.P > 0 && cl_normal_entries(a.N, a.K, &entries) && a.x && a.idx && a.knn && a.normals && a.points &&
           a.min_scaling && a.opac;
}

int sgr_better_normal_forward(long long N, int K, int P, const float* samples, const int64_t* sample_idx, const int64_t* knn_idx,
                              const float* normals, const float* points, const float* min_scaling, const float* opacities, float* loss,
                              char* scratch, void* stream)
{
    const NormalArgs a{N, K, P, samples, reinterpret_cast<const long long*>(sample_idx), reinterpret_cast<const long long*>(knn_idx),
                       normals, points, min_scaling, opacities};
    if (!normal_args_ok(a) || !loss || !scratch) return SGR_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const size_t nb = cl_normal_blocks(N, K);
    double* partial = reinterpret_cast<double*>(scratch);
    if (K == 16) hipLaunchKernelGGL(k_normal_fwd16, dim3((unsigned)nb), dim3(256), 0, s, a, partial);
    else hipLaunchKernelGGL(k_normal_fwd, dim3((unsigned)nb), dim3(256), 0, s, a, partial);
    hipLaunchKernelGGL(k_finish_means, dim3(1), dim3(256), 0, s, partial, nb, 1, -1, (double)N, loss, nullptr, nullptr);
    return sgr_launch_status();
}

size_t sgr_better_normal_backward_scratch_bytes(long long N, int K, int P, int through_normal_only)
{
    size_t entries;
    if (!cl_normal_entries(N, K, &entries)) return 0;
    return cl_normal_bwd_layout(entries, P, through_normal_only ? 3 : 6, sgr_group_scratch_bytes(entries)).total;
}

int sgr_better_normal_backward(long long N, int K, int P, const float* samples, const int64_t* sample_idx, const int64_t* knn_idx,
                               const float* normals, const float* points, const float* min_scaling, const float* opacities,
                               int through_normal_only, const float* dL_dloss, float* dL_dnormals, float* dL_dpoints, float* dL_dsamples,
                               char* scratch, void* stream)
{
    const NormalArgs a{N, K, P, samples, reinterpret_cast<const long long*>(sample_idx), reinterpret_cast<const long long*>(knn_idx),
                       normals, points, min_scaling, opacities};
    if (!normal_args_ok(a) || !dL_dloss || !dL_dnormals || !scratch || (!through_normal_only && !dL_dpoints)) return SGR_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    size_t entries = 0;
    cl_normal_entries(N, K, &entries);
    const ClNormalBwdLayout L = cl_normal_bwd_layout(entries, P, through_normal_only ? 3 : 6, sgr_group_scratch_bytes(entries));
    long long* keys = reinterpret_cast<long long*>(scratch + L.keys);
    uint32_t* start = reinterpret_cast<uint32_t*>(scratch + L.start);
    float* rows = reinterpret_cast<float*>(scratch + L.rows);
    const unsigned nb = (unsigned)cl_normal_blocks(N, K);
    if (K == 16) {
        if (through_normal_only) hipLaunchKernelGGL(k_normal_bwd16<true>, dim3(nb), dim3(256), 0, s, a, dL_dloss, keys, rows, dL_dsamples);
        else hipLaunchKernelGGL(k_normal_bwd16<false>, dim3(nb), dim3(256), 0, s, a, dL_dloss, keys, rows, dL_dsamples);
    } else {
        if (through_normal_only) hipLaunchKernelGGL(k_normal_bwd<true>, dim3(nb), dim3(256), 0, s, a, dL_dloss, keys, rows, dL_dsamples);
        else hipLaunchKernelGGL(k_normal_bwd<false>, dim3(nb), dim3(256), 0, s, a, dL_dloss, keys, rows, dL_dsamples);
    }
    const uint32_t* list = nullptr;
    const int rc = sgr_group_by_key((long long)entries, keys, P, scratch + L.group, start, &list, s);
    if (rc < 0) return rc;
    if (through_normal_only)
        hipLaunchKernelGGL(k_normal_rows_gather<3>, dim3(blocks256((size_t)P * 16)), dim3(256), 0, s, P, rows, start, list, dL_dnormals, dL_dpoints);
    else
        hipLaunchKernelGGL(k_normal_rows_gather<6>, dim3(blocks256((size_t)P * 16)), dim3(256), 0, s, P, rows, start, list, dL_dnormals, dL_dpoints);
    return sgr_launch_status();
}

}  // extern "C"
