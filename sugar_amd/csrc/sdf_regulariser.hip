// sdf_regulariser.hip -- the tensor code of SuGaR's coarse-stage SDF regulariser (sugar_trainers/coarse_sdf.py:566-716) that runs
// inside methods of the `SuGaR` class, as gfx950 kernels.  Three operations, each a forward and a backward (the fourth, the SDF field,
// is the SDF = true half of the density kernel family in csrc/field.hip):
//
//   sample transform : sugar_scene/sugar_model.py:924-926    x_n = mu_i + rot(q_i, f * s_i (.) eps_n),  i = idx[n]
//                      rot(q, v) = vector part of q (x) (0, v) (x) conj(q), q NOT normalised (pytorch3d's quaternion_apply).
//                      Backward: the samples are grouped by Gaussian (sgr_group.h), sixteen lanes per Gaussian sum its samples.
//   smallest axis    : :930-944     n_p = column j of R(q_p), j = argmin_j s_p[j] (lowest j on ties), R = pytorch3d's quaternion_to_matrix
//                      (two_s = 2 / |q|^2).  Backward to the quaternions only.
//   depth lookup     : :1318-1333   projection (row vectors, divide by w), g = -min(H,W)/(W,H) * ndc, then grid_sample: bilinear,
//                      padding 'border', align_corners False.  The depth map is read through its strides.  Backward: the points through
//                      the bilinear derivatives and the projection; the depth map by float atomic adds (as torch's own
//                      grid_sampler_2d_backward: the one output here that is not bit-reproducible).
//
// Every per-Gaussian gradient row is WRITTEN (zero where nothing references the Gaussian) and summed in a fixed order, without float
// atomics: bit-identical from run to run.
#include "../../include/sugar_raster.h"
#include "sgr_device.h"
#include "sgr_group.h"
#include "sgr_depth_lookup.h"

namespace {

struct Q4 { float w, x, y, z; };

__device__ __forceinline__ Q4 qmul(const Q4 a, const Q4 b)  // Hamilton product, pytorch3d's quaternion_raw_multiply
{
    Q4 o;
    o.w = a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z;
    o.x = a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y;
    o.y = a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x;
    o.z = a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w;
    return o;
}
__device__ __forceinline__ Q4 qconj(const Q4 a) { return Q4{a.w, -a.x, -a.y, -a.z}; }

// ---------------------------------------------------------------------------------------------------------- sample transform
__global__ void __launch_bounds__(256) k_sample_fwd(long long N, int P, const long long* __restrict__ idx, const float* __restrict__ points,
                                                    const float* __restrict__ quats, const float* __restrict__ scaling,
                                                    const float* __restrict__ noise, float factor, float* __restrict__ out)
{
    const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const long long i = wrap_row(idx[n], P);
    if (i < 0 || i >= P) { out[3 * n] = 0.f; out[3 * n + 1] = 0.f; out[3 * n + 2] = 0.f; return; }  // (torch raises; never a wild read)
    const float4 qq = reinterpret_cast<const float4*>(quats)[i];
    const Q4 q{qq.x, qq.y, qq.z, qq.w};
    const Q4 v{0.f, factor * scaling[3 * i] * noise[3 * n], factor * scaling[3 * i + 1] * noise[3 * n + 1],
               factor * scaling[3 * i + 2] * noise[3 * n + 2]};
    const Q4 o = qmul(qmul(q, v), qconj(q));
    out[3 * n] = points[3 * i] + o.x; out[3 * n + 1] = points[3 * i + 1] + o.y; out[3 * n + 2] = points[3 * i + 2] + o.z;
}

// out = (q (x) V) (x) conj(q) with cotangent G = (0, g): for c = a (x) b, <G, c> = <G (x) conj(b), a> = <conj(a) (x) G, b>.
__global__ void __launch_bounds__(256) k_sample_bwd_gather(int P, const float* __restrict__ quats, const float* __restrict__ scaling,
                                                           const float* __restrict__ noise, const float* __restrict__ g, float factor,
                                                           const uint32_t* __restrict__ start, const uint32_t* __restrict__ list,
                                                           float* __restrict__ dpoints, float* __restrict__ dquats,
                                                           float* __restrict__ dscaling)
{
    const int t = (int)(((size_t)blockIdx.x * 256 + threadIdx.x) >> 4);
    const uint32_t sub = threadIdx.x & 15;
    if (t >= P) return;   // (whole rows leave together: the row rotates never cross a row)
    const float4 qq = reinterpret_cast<const float4*>(quats)[t];
    const Q4 q{qq.x, qq.y, qq.z, qq.w};
    const float s0 = scaling[3 * (size_t)t], s1 = scaling[3 * (size_t)t + 1], s2 = scaling[3 * (size_t)t + 2];
    float dp0 = 0.f, dp1 = 0.f, dp2 = 0.f, dqw = 0.f, dqx = 0.f, dqy = 0.f, dqz = 0.f, ds0 = 0.f, ds1 = 0.f, ds2 = 0.f;
    const uint32_t e0 = start[t], e1 = start[t + 1];
    for (uint32_t e = e0 + sub; e < e1; e += 16) {
        const size_t n = list[e];
        const float e0n = noise[3 * n], e1n = noise[3 * n + 1], e2n = noise[3 * n + 2];
        const Q4 G{0.f, g[3 * n], g[3 * n + 1], g[3 * n + 2]};
        const Q4 V{0.f, factor * s0 * e0n, factor * s1 * e1n, factor * s2 * e2n};
        const Q4 a = qmul(q, V);
        const Q4 da = qmul(G, q);                         // G (x) conj(conj(q))
        const Q4 dq1 = qconj(qmul(qconj(a), G));          // through b = conj(q)
        const Q4 dq2 = qmul(da, qconj(V));                // through a = q (x) V
        const Q4 dV = qmul(qconj(q), da);
        dp0 += G.x; dp1 += G.y; dp2 += G.z;
        dqw += dq1.w + dq2.w; dqx += dq1.x + dq2.x; dqy += dq1.y + dq2.y; dqz += dq1.z + dq2.z;
        ds0 += factor * e0n * dV.x; ds1 += factor * e1n * dV.y; ds2 += factor * e2n * dV.z;
    }
    dp0 = row_sum16(dp0); dp1 = row_sum16(dp1); dp2 = row_sum16(dp2);
    dqw = row_sum16(dqw); dqx = row_sum16(dqx); dqy = row_sum16(dqy); dqz = row_sum16(dqz);
    ds0 = row_sum16(ds0); ds1 = row_sum16(ds1); ds2 = row_sum16(ds2);
    if (sub == 0) {
        dpoints[3 * (size_t)t] = dp0; dpoints[3 * (size_t)t + 1] = dp1; dpoints[3 * (size_t)t + 2] = dp2;
        reinterpret_cast<float4*>(dquats)[t] = make_float4(dqw, dqx, dqy, dqz);
        dscaling[3 * (size_t)t] = ds0; dscaling[3 * (size_t)t + 1] = ds1; dscaling[3 * (size_t)t + 2] = ds2;
    }
}

// ------------------------------------------------------------------------------------------------------------- smallest axis
__device__ __forceinline__ int smallest_of3(const float* __restrict__ s)  // the lowest index wins on ties
{
    int j = 0;
    float m = s[0];
    if (s[1] < m) { j = 1; m = s[1]; }
    if (s[2] < m) j = 2;
    return j;
}

__global__ void __launch_bounds__(256) k_smallest_axis_fwd(int P, const float* __restrict__ quats, const float* __restrict__ scaling,
                                                           float* __restrict__ axis, long long* __restrict__ axis_idx)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const float4 q = reinterpret_cast<const float4*>(quats)[p];
    const int j = smallest_of3(scaling + 3 * (size_t)p);
    const float t = 2.0f / (q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
    float M[9];
    quat_M(q.x, q.y, q.z, q.w, M);
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float m = j == 0 ? M[3 * a] : (j == 1 ? M[3 * a + 1] : M[3 * a + 2]);
        axis[3 * (size_t)p + a] = (a == j ? 1.0f : 0.0f) + t * m;
    }
    if (axis_idx) axis_idx[p] = j;
}

__global__ void __launch_bounds__(256) k_smallest_axis_bwd(int P, const float* __restrict__ quats, const float* __restrict__ scaling,
                                                           const float* __restrict__ g_axis, float* __restrict__ d_quats)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const float4 q = reinterpret_cast<const float4*>(quats)[p];
    const float r = q.x, i = q.y, j = q.z, k = q.w;
    const int col = smallest_of3(scaling + 3 * (size_t)p);
    const float t = 2.0f / (r * r + i * i + j * j + k * k);
    float M[9], G[9];
    quat_M(r, i, j, k, M);
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) G[3 * a + b] = (b == col) ? g_axis[3 * (size_t)p + a] : 0.f;   // dL/dR
    float GM = 0.f;
#pragma unroll
    for (int e = 0; e < 9; e++) GM += G[e] * M[e];
    // dL/dq = t * sum G : dM/dq  +  (G : M) * dt/dq,   dt/dq = -t^2 q   (as k_scaled_rotation_bwd of field.hip)
    const float dr = t * (-k * G[1] + j * G[2] + k * G[3] - i * G[5] - j * G[6] + i * G[7]) - GM * t * t * r;
    const float di = t * (j * G[1] + k * G[2] + j * G[3] - 2.f * i * G[4] - r * G[5] + k * G[6] + r * G[7] - 2.f * i * G[8]) - GM * t * t * i;
    const float dj = t * (-2.f * j * G[0] + i * G[1] + r * G[2] + i * G[3] + k * G[5] - r * G[6] + k * G[7] - 2.f * j * G[8]) - GM * t * t * j;
    const float dk = t * (-2.f * k * G[0] - r * G[1] + i * G[2] + r * G[3] - 2.f * k * G[4] + j * G[5] + i * G[6] + j * G[7]) - GM * t * t * k;
    reinterpret_cast<float4*>(d_quats)[p] = make_float4(dr, di, dj, dk);
}

// -------------------------------------------------------------------------------------------------------------- depth lookup
// (the per-point arithmetic is sgr_depth_lookup.h: coarse_loss.hip evaluates the same lookup inside its loss kernels)
__global__ void __launch_bounds__(256) k_depth_lookup_fwd(long long M, const float* __restrict__ pts, const float* __restrict__ Pm,
                                                          const float* __restrict__ depth, long long sy, long long sx, int H, int W,
                                                          float* __restrict__ out)
{
    const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
    if (n >= M) return;
    const Lookup L = lookup_coords(pts[3 * n], pts[3 * n + 1], pts[3 * n + 2], Pm, H, W);
    out[n] = lookup_value(L, depth, sy, sx, H, W);
}

__global__ void __launch_bounds__(256) k_depth_lookup_bwd(long long M, const float* __restrict__ pts, const float* __restrict__ Pm,
                                                          const float* __restrict__ depth, long long sy, long long sx, int H, int W,
                                                          const float* __restrict__ g_out, float* __restrict__ dpts,
                                                          float* __restrict__ ddepth)
{
    const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
    if (n >= M) return;
    const Lookup L = lookup_coords(pts[3 * n], pts[3 * n + 1], pts[3 * n + 2], Pm, H, W);
    float gix, giy;
    lookup_value_bwd(L, depth, sy, sx, H, W, g_out[n], ddepth, gix, giy);
    if (dpts) lookup_coords_bwd(L, Pm, gix, giy, dpts[3 * n], dpts[3 * n + 1], dpts[3 * n + 2]);
}

}  // namespace

extern "C" {

int sgr_sample_transform_forward(long long N, int P, const int64_t* idx, const float* points, const float* quaternions,
                                 const float* scaling, const float* noise, float factor, float* out, void* stream)
{
    if (N <= 0) return 0;
    if (P <= 0 || !idx || !points || !quaternions || !scaling || !noise || !out || misaligned16(quaternions) ||
        (unsigned long long)N > 0xFFFFFFFFull)
        return SGR_E_INVALID;
    hipLaunchKernelGGL(k_sample_fwd, dim3(blocks256((size_t)N)), dim3(256), 0, (hipStream_t)stream, N, P,
                       reinterpret_cast<const long long*>(idx), points, quaternions, scaling, noise, factor, out);
    return sgr_launch_status();
}

size_t sgr_sample_transform_backward_scratch_bytes(long long N, int P)
{
    const size_t n = (size_t)(N > 0 ? N : 0), p = (size_t)(P > 0 ? P : 0);
    return sgr_align((p + 1) * 4) + sgr_group_scratch_bytes(n);   // start | the radix grouping's buffers
}

int sgr_sample_transform_backward(long long N, int P, const int64_t* idx, const float* quaternions, const float* scaling,
                                  const float* noise, float factor, const float* dL_dout, float* dL_dpoints, float* dL_dquaternions,
                                  float* dL_dscaling, char* scratch, void* stream)
{
    if (P <= 0) return 0;
    if (N < 0 || (N > 0 && (!idx || !noise || !dL_dout)) || !quaternions || !scaling || !dL_dpoints || !dL_dquaternions ||
        !dL_dscaling || !scratch || misaligned16(quaternions) || misaligned16(dL_dquaternions) || (unsigned long long)N > 0xFFFFFFFFull)
        return SGR_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    uint32_t* start = reinterpret_cast<uint32_t*>(scratch);
    const uint32_t* list = nullptr;
    const int rc = sgr_group_by_key(N, reinterpret_cast<const long long*>(idx), P, scratch + sgr_align(((size_t)P + 1) * 4), start, &list, s);
    if (rc < 0) return rc;
    hipLaunchKernelGGL(k_sample_bwd_gather, dim3(blocks256((size_t)P * 16)), dim3(256), 0, s, P, quaternions, scaling, noise, dL_dout,
                       factor, start, list, dL_dpoints, dL_dquaternions, dL_dscaling);
    return sgr_launch_status();
}

int sgr_smallest_axis_forward(int P, const float* quaternions, const float* scaling, float* axis, int64_t* axis_idx, void* stream)
{
    if (P <= 0) return 0;
    if (!quaternions || !scaling || !axis || misaligned16(quaternions)) return SGR_E_INVALID;
    hipLaunchKernelGGL(k_smallest_axis_fwd, dim3(blocks256((size_t)P)), dim3(256), 0, (hipStream_t)stream, P, quaternions, scaling, axis,
                       reinterpret_cast<long long*>(axis_idx));
    return sgr_launch_status();
}

int sgr_smallest_axis_backward(int P, const float* quaternions, const float* scaling, const float* dL_daxis, float* dL_dquaternions,
                               void* stream)
{
    if (P <= 0) return 0;
    if (!quaternions || !scaling || !dL_daxis || !dL_dquaternions || misaligned16(quaternions) || misaligned16(dL_dquaternions))
        return SGR_E_INVALID;
    hipLaunchKernelGGL(k_smallest_axis_bwd, dim3(blocks256((size_t)P)), dim3(256), 0, (hipStream_t)stream, P, quaternions, scaling,
                       dL_daxis, dL_dquaternions);
    return sgr_launch_status();
}

int sgr_depth_lookup_forward(long long M, const float* points_cam, const float* projection, const float* depth, long long stride_y,
                             long long stride_x, int height, int width, float* out, void* stream)
{
    if (M <= 0) return 0;
    if (!points_cam || !projection || !depth || !out || height < 1 || width < 1 || stride_y < 0 || stride_x < 0 ||
        (unsigned long long)M > 0xFFFFFFFFull)
        return SGR_E_INVALID;
    hipLaunchKernelGGL(k_depth_lookup_fwd, dim3(blocks256((size_t)M)), dim3(256), 0, (hipStream_t)stream, M, points_cam, projection, depth,
                       stride_y, stride_x, height, width, out);
    return sgr_launch_status();
}

int sgr_depth_lookup_backward(long long M, const float* points_cam, const float* projection, const float* depth, long long stride_y,
                              long long stride_x, int height, int width, const float* dL_dout, float* dL_dpoints_cam, float* dL_ddepth,
                              void* stream)
{
    if (height < 1 || width < 1 || M < 0 || (unsigned long long)M > 0xFFFFFFFFull) return SGR_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    if (dL_ddepth && hipMemsetAsync(dL_ddepth, 0, (size_t)height * width * 4, s) != hipSuccess) return SGR_E_HIP;
    if (M == 0) return 0;
    if (!points_cam || !projection || !depth || !dL_dout || (!dL_dpoints_cam && !dL_ddepth) || stride_y < 0 || stride_x < 0)
        return SGR_E_INVALID;
    hipLaunchKernelGGL(k_depth_lookup_bwd, dim3(blocks256((size_t)M)), dim3(256), 0, s, M, points_cam, projection, depth, stride_y,
                       stride_x, height, width, dL_dout, dL_dpoints_cam, dL_ddepth);
    return sgr_launch_status();
}

}  // extern "C"
