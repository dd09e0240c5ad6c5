// sgr_device.h -- device helpers shared by the translation units: the tile rectangle of preprocess.hip and binning.hip, and the
// wave and workgroup prefix sums of every kernel that forms one (binning, k-NN grid, field scatter, pixel pick, marching cubes),
// and the DPP row sum, quaternion matrix and index wrap of the field, regulariser and grouping kernels.
#pragma once
#include "sgr_common.h"

// inclusive scan over the 64 lanes of a wave
__device__ __forceinline__ uint32_t sgr_wave_incl_scan(uint32_t v)
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up((int)v, d);
        if (lane >= d) v += y;
    }
    return v;
}

// sum of x over the WAVES * 64 threads of a workgroup, returned to every thread; `excl` = the sum over the threads before this one.
// Every thread of the workgroup must call it (two barriers; s_wave[WAVES] may be reused after it returns).
template <int WAVES>
__device__ __forceinline__ uint32_t sgr_block_scan(uint32_t x, uint32_t* s_wave, uint32_t& excl)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t incl = sgr_wave_incl_scan(x);
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < WAVES; w++) {
        const uint32_t t = s_wave[w];
        if (w < wave) before += t;
        total += t;
    }
    excl = before + incl - x;
    __syncthreads();
    return total;
}

// ---- shared by field.hip, sdf_regulariser.hip and group.hip ---------------------------------------------------------
// sum over the 16 lanes of a DPP row, returned to every lane of the row (row_ror:8 / 4 / 2 / 1 fold into the adds)
__device__ __forceinline__ float row_sum16(float x)
{
    x += __uint_as_float((uint32_t)__builtin_amdgcn_update_dpp(0, (int)__float_as_uint(x), 0x128, 0xF, 0xF, false));
    x += __uint_as_float((uint32_t)__builtin_amdgcn_update_dpp(0, (int)__float_as_uint(x), 0x124, 0xF, 0xF, false));
    x += __uint_as_float((uint32_t)__builtin_amdgcn_update_dpp(0, (int)__float_as_uint(x), 0x122, 0xF, 0xF, false));
    x += __uint_as_float((uint32_t)__builtin_amdgcn_update_dpp(0, (int)__float_as_uint(x), 0x121, 0xF, 0xF, false));
    return x;
}

// R = I + two_s * M, two_s = 2 / |q|^2 (pytorch3d's quaternion_to_matrix, real part first)
__device__ __forceinline__ void quat_M(float r, float i, float j, float k, float M[9])
{
    M[0] = -(j * j + k * k); M[1] = i * j - k * r;     M[2] = i * k + j * r;
    M[3] = i * j + k * r;    M[4] = -(i * i + k * k);  M[5] = j * k - i * r;
    M[6] = i * k - j * r;    M[7] = j * k + i * r;     M[8] = -(i * i + j * j);
}

// gaussian_std of sugar_model.py:1971-1972 (and coarse_sdf.py:612-620) for Gaussian g: | scales (.) R(q)^T normalize(cam_center - centre) |
// with the unit quaternions the model hands out (`quaternion_apply(quaternion_invert(q), v)`; F.normalize: v / max(|v|, 1e-12)).
// Shared by k_view_std of field.hip and the surface band of coarse_loss.hip.
__device__ __forceinline__ float view_std_of(size_t g, const float* __restrict__ centers, const float* __restrict__ quats,
                                             const float* __restrict__ scaling, const float* __restrict__ cam_center)
{
    const float4 q = reinterpret_cast<const float4*>(quats)[g];
    const float r = q.x, x = q.y, y = q.z, z = q.w;
    float vx = cam_center[0] - centers[3 * g], vy = cam_center[1] - centers[3 * g + 1],
          vz = cam_center[2] - centers[3 * g + 2];
    const float inv = 1.0f / fmaxf(sqrtf(vx * vx + vy * vy + vz * vz), 1e-12f);
    vx *= inv; vy *= inv; vz *= inv;
    // rows of R^T = columns of R
    const float ox = (1 - 2 * (y * y + z * z)) * vx + 2 * (x * y + r * z) * vy + 2 * (x * z - r * y) * vz;
    const float oy = 2 * (x * y - r * z) * vx + (1 - 2 * (x * x + z * z)) * vy + 2 * (y * z + r * x) * vz;
    const float oz = 2 * (x * z + r * y) * vx + 2 * (y * z - r * x) * vy + (1 - 2 * (x * x + y * y)) * vz;
    const float sx = scaling[3 * g] * ox, sy = scaling[3 * g + 1] * oy, sz = scaling[3 * g + 2] * oz;
    return sqrtf(sx * sx + sy * sy + sz * sz);
}

// a row index as Python reads it: negative values wrap once (the caller checks 0 <= result < P)
__device__ __forceinline__ long long wrap_row(long long i, int P) { return i < 0 ? i + P : i; }

static inline bool misaligned16(const void* p) { return ((uintptr_t)p & 15) != 0; }
static inline unsigned blocks256(size_t n) { return (unsigned)((n + 255) / 256); }

__device__ __forceinline__ int sgr_f2i_sat(float v)
{
    if (v != v) return 0;
    if (v >= 2147483648.0f) return 2147483647;
    if (v <= -2147483648.0f) return (-2147483647 - 1);
    return (int)v;
}

// getRect, DGR/cuda_rasterizer/auxiliary.h:46-56: float divide, truncation toward zero, clamp to the grid.
// Must stay bit-identical between the counting pass (preprocess) and the scatter pass (binning): both
// translation units are built with -ffp-contract=off.
__device__ __forceinline__ void sgr_get_rect(float px, float py, int max_radius, int gx, int gy,
                                             int& minx, int& miny, int& maxx, int& maxy)
{
    const float r = (float)max_radius;
    minx = min(gx, max(0, sgr_f2i_sat((px - r) / (float)SGR_TILE_X)));
    miny = min(gy, max(0, sgr_f2i_sat((py - r) / (float)SGR_TILE_Y)));
    maxx = min(gx, max(0, sgr_f2i_sat((px + r + (float)SGR_TILE_X - 1.0f) / (float)SGR_TILE_X)));
    maxy = min(gy, max(0, sgr_f2i_sat((py + r + (float)SGR_TILE_Y - 1.0f) / (float)SGR_TILE_Y)));
}
