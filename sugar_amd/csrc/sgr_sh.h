// sgr_sh.h -- spherical-harmonics constants and evaluation (device code shared by preprocess.hip, sh_adam.hip and sh_rgb.hip).
//
// Restates computeColorFromSH and its backward (DGR/cuda_rasterizer/forward.cu:20-71, backward.cu:47-139).  The three units that
// include it are built with -ffp-contract=off: every float op is an individually rounded IEEE operation in the order written.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

__device__ __constant__ const float SH_C0 = 0.28209479177387814f;
__device__ __constant__ const float SH_C1 = 0.4886025119029199f;
__device__ __constant__ const float SH_C2[5] = {1.0925484305920792f, -1.0925484305920792f, 0.31539156525252005f,
                                                 -1.0925484305920792f, 0.5462742152960396f};
__device__ __constant__ const float SH_C3[7] = {-0.5900435899266435f, 2.890611442640554f, -0.4570457994644658f,
                                                 0.3731763325901154f, -0.4570457994644658f, 1.445305721320277f,
                                                 -0.5900435899266435f};

__device__ __forceinline__ float fmin_(float a, float b) { return a < b ? a : b; }
__device__ __forceinline__ float fmax_(float a, float b) { return a > b ? a : b; }

// SH -> RGB for channel c; sh points at this Gaussian's [M][3] coefficient block
__device__ __forceinline__ float sh_channel(int deg, const float* sh, int c, float x, float y, float z)
{
#define SH(k) sh[3 * (k) + c]
    float r = SH_C0 * SH(0);
    if (deg > 0) {
        r = r - SH_C1 * y * SH(1) + SH_C1 * z * SH(2) - SH_C1 * x * SH(3);
        if (deg > 1) {
            float xx = x * x, yy = y * y, zz = z * z;
            float xy = x * y, yz = y * z, xz = x * z;
            r = r + SH_C2[0] * xy * SH(4) + SH_C2[1] * yz * SH(5) + SH_C2[2] * (2.0f * zz - xx - yy) * SH(6) +
                SH_C2[3] * xz * SH(7) + SH_C2[4] * (xx - yy) * SH(8);
            if (deg > 2) {
                r = r + SH_C3[0] * y * (3.0f * xx - yy) * SH(9) + SH_C3[1] * xy * z * SH(10) +
                    SH_C3[2] * y * (4.0f * zz - xx - yy) * SH(11) +
                    SH_C3[3] * z * (2.0f * zz - 3.0f * xx - 3.0f * yy) * SH(12) +
                    SH_C3[4] * x * (4.0f * zz - xx - yy) * SH(13) + SH_C3[5] * z * (xx - yy) * SH(14) +
                    SH_C3[6] * x * (xx - 3.0f * yy) * SH(15);
            }
        }
    }
#undef SH
    return r + 0.5f;
}

// Load this Gaussian's SH block into registers.  The [P,M,3] layout gives each lane 12*M contiguous
// bytes; with M == 16 and a 16-B aligned base (FAST: decided by the launcher, so the kernel holds ONE load path and the
// loaded values need not meet another path's at a join, which would make the compiler wait for them on the spot) that is
// twelve dwordx4 loads per lane.
template <int MAXC, bool FAST = false>
__device__ __forceinline__ void load_sh(const float* shs, size_t idx, int M, float* sh)
{
    const float* src = shs + idx * (size_t)M * 3;
    const int n = M * 3;
    if (FAST) {
        const float4* s4 = reinterpret_cast<const float4*>(shs) + idx * 12;
#pragma unroll
        for (int i = 0; i < 12; i++) {
            float4 v = s4[i];
            sh[4 * i] = v.x; sh[4 * i + 1] = v.y; sh[4 * i + 2] = v.z; sh[4 * i + 3] = v.w;
        }
    } else if (MAXC == 48 && n == 48 && ((uintptr_t)src & 15) == 0) {
        const float4* s4 = reinterpret_cast<const float4*>(src);
#pragma unroll
        for (int i = 0; i < 12; i++) {
            float4 v = s4[i];
            sh[4 * i] = v.x; sh[4 * i + 1] = v.y; sh[4 * i + 2] = v.z; sh[4 * i + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < MAXC; i++) sh[i] = (i < n) ? src[i] : 0.0f;
    }
}
__host__ __device__ __forceinline__ bool sh_fast_layout(const float* shs, int M) { return shs && M == 16 && ((uintptr_t)shs & 15) == 0; }

// d RGB_c / d(view direction) for one colour channel from its 16 coefficients h[k] (backward.cu:99-131): the derivative half
// of computeColorFromSH's backward, shared by the backward preprocess kernel and the SH-Adam kernel.
__device__ __forceinline__ void sh_dir_channel(const int deg, const float* h, const float x, const float y, const float z,
                                               float& dRGBdx, float& dRGBdy, float& dRGBdz)
{
    dRGBdx = 0; dRGBdy = 0; dRGBdz = 0;
    if (deg > 0) {
        dRGBdx = -SH_C1 * h[3]; dRGBdy = -SH_C1 * h[1]; dRGBdz = SH_C1 * h[2];
        if (deg > 1) {
            float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
            dRGBdx += SH_C2[0] * y * h[4] + SH_C2[2] * 2.f * -x * h[6] + SH_C2[3] * z * h[7] + SH_C2[4] * 2.f * x * h[8];
            dRGBdy += SH_C2[0] * x * h[4] + SH_C2[1] * z * h[5] + SH_C2[2] * 2.f * -y * h[6] + SH_C2[4] * 2.f * -y * h[8];
            dRGBdz += SH_C2[1] * y * h[5] + SH_C2[2] * 2.f * 2.f * z * h[6] + SH_C2[3] * x * h[7];
            if (deg > 2) {
                dRGBdx += (SH_C3[0] * h[9] * 3.f * 2.f * xy + SH_C3[1] * h[10] * yz + SH_C3[2] * h[11] * -2.f * xy +
                           SH_C3[3] * h[12] * -3.f * 2.f * xz + SH_C3[4] * h[13] * (-3.f * xx + 4.f * zz - yy) +
                           SH_C3[5] * h[14] * 2.f * xz + SH_C3[6] * h[15] * 3.f * (xx - yy));
                dRGBdy += (SH_C3[0] * h[9] * 3.f * (xx - yy) + SH_C3[1] * h[10] * xz +
                           SH_C3[2] * h[11] * (-3.f * yy + 4.f * zz - xx) + SH_C3[3] * h[12] * -3.f * 2.f * yz +
                           SH_C3[4] * h[13] * -2.f * xy + SH_C3[5] * h[14] * -2.f * yz + SH_C3[6] * h[15] * -3.f * 2.f * xy);
                dRGBdz += (SH_C3[1] * h[10] * xy + SH_C3[2] * h[11] * 4.f * 2.f * yz +
                           SH_C3[3] * h[12] * 3.f * (2.f * zz - xx - yy) + SH_C3[4] * h[13] * 4.f * 2.f * xz +
                           SH_C3[5] * h[14] * (xx - yy));
            }
        }
    }
}

// The 16 SH basis values of computeColorFromSH's backward (backward.cu:47-97: dRGBdsh0 ... dRGBdsh15), zero beyond the active
// degree; the very expressions sh_backward multiplies by dL/dRGB, so basis[k] * dL_dRGB[c] is bit-identical to its DSH(k).
__device__ __forceinline__ void sh_basis16(const int deg, const float x, const float y, const float z, float* b)
{
#pragma unroll
    for (int k = 0; k < 16; k++) b[k] = 0.0f;
    b[0] = SH_C0;
    if (deg > 0) {
        b[1] = -SH_C1 * y; b[2] = SH_C1 * z; b[3] = -SH_C1 * x;
        if (deg > 1) {
            float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
            b[4] = SH_C2[0] * xy; b[5] = SH_C2[1] * yz; b[6] = SH_C2[2] * (2.f * zz - xx - yy); b[7] = SH_C2[3] * xz;
            b[8] = SH_C2[4] * (xx - yy);
            if (deg > 2) {
                b[9] = SH_C3[0] * y * (3.f * xx - yy); b[10] = SH_C3[1] * xy * z; b[11] = SH_C3[2] * y * (4.f * zz - xx - yy);
                b[12] = SH_C3[3] * z * (2.f * zz - 3.f * xx - 3.f * yy); b[13] = SH_C3[4] * x * (4.f * zz - xx - yy);
                b[14] = SH_C3[5] * z * (xx - yy); b[15] = SH_C3[6] * x * (xx - 3.f * yy);
            }
        }
    }
}

// computeColorFromSH backward for one Gaussian (backward.cu:47-137): dsh[k][c] = basis_k(dir) * masked dL/dRGB[c] and the
// gradient w.r.t. the (normalised) view direction.  `clamped` bit c set = channel c was clamped to 0 by the forward.
__device__ __forceinline__ void sh_backward(const int deg, const float* sh, const float* dcol, const uint32_t clamped,
                                            const float x, const float y, const float z, float* dsh, float* dL_ddir)
{
#pragma unroll
    for (int c = 0; c < 3; c++) {
#define DSH(k) dsh[3 * (k) + c]
        float dL_dRGB = dcol[c] * (((clamped >> c) & 1u) ? 0.0f : 1.0f);
        DSH(0) = SH_C0 * dL_dRGB;
        if (deg > 0) {
            DSH(1) = (-SH_C1 * y) * dL_dRGB; DSH(2) = (SH_C1 * z) * dL_dRGB; DSH(3) = (-SH_C1 * x) * dL_dRGB;
            if (deg > 1) {
                float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
                DSH(4) = (SH_C2[0] * xy) * dL_dRGB; DSH(5) = (SH_C2[1] * yz) * dL_dRGB;
                DSH(6) = (SH_C2[2] * (2.f * zz - xx - yy)) * dL_dRGB; DSH(7) = (SH_C2[3] * xz) * dL_dRGB;
                DSH(8) = (SH_C2[4] * (xx - yy)) * dL_dRGB;
                if (deg > 2) {
                    DSH(9) = (SH_C3[0] * y * (3.f * xx - yy)) * dL_dRGB; DSH(10) = (SH_C3[1] * xy * z) * dL_dRGB;
                    DSH(11) = (SH_C3[2] * y * (4.f * zz - xx - yy)) * dL_dRGB;
                    DSH(12) = (SH_C3[3] * z * (2.f * zz - 3.f * xx - 3.f * yy)) * dL_dRGB;
                    DSH(13) = (SH_C3[4] * x * (4.f * zz - xx - yy)) * dL_dRGB;
                    DSH(14) = (SH_C3[5] * z * (xx - yy)) * dL_dRGB; DSH(15) = (SH_C3[6] * x * (xx - 3.f * yy)) * dL_dRGB;
                }
            }
        }
#undef DSH
        float h[16];
#pragma unroll
        for (int k = 0; k < 16; k++) h[k] = sh[3 * k + c];
        float dRGBdx, dRGBdy, dRGBdz;
        sh_dir_channel(deg, h, x, y, z, dRGBdx, dRGBdy, dRGBdz);
        dL_ddir[0] += dRGBdx * dL_dRGB; dL_ddir[1] += dRGBdy * dL_dRGB; dL_ddir[2] += dRGBdz * dL_dRGB;
    }
}

}  // namespace
