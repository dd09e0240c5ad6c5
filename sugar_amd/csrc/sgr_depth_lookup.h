// sgr_depth_lookup.h -- the arithmetic of SuGaR.get_points_depth_in_depth_map (sugar_scene/sugar_model.py:1318-1333) for one point,
// shared by the kernels of sdf_regulariser.hip (sgr_depth_lookup_*) and coarse_loss.hip: projection (row vectors, divide by w),
// g = -min(H,W)/(W,H) * ndc, then grid_sample: bilinear, padding 'border', align_corners False.  The depth map is read through its
// strides (in elements).
#pragma once
#include <hip/hip_runtime.h>

struct Lookup {
    float c3, ndc_x, ndc_y;   // w of the projection, and x / w, y / w
    float ix, iy;             // pixel coordinates after the clamp to the image
    float mx, my;             // d(ix) / d(ndc_x), d(iy) / d(ndc_y): 0 where the clamp is active
    bool finite;
};

__device__ __forceinline__ Lookup lookup_coords(float x, float y, float z, const float* __restrict__ Pm, int H, int W)
{
    Lookup L;
    const float c0 = x * Pm[0] + y * Pm[4] + z * Pm[8] + Pm[12];
    const float c1 = x * Pm[1] + y * Pm[5] + z * Pm[9] + Pm[13];
    L.c3 = x * Pm[3] + y * Pm[7] + z * Pm[11] + Pm[15];
    L.ndc_x = c0 / L.c3; L.ndc_y = c1 / L.c3;
    const float m = (float)(H < W ? H : W);
    const float fx = -1.0f * m / (float)W, fy = -1.0f * m / (float)H;
    const float gx = fx * L.ndc_x, gy = fy * L.ndc_y;
    float ix = ((gx + 1.0f) * (float)W - 1.0f) / 2.0f, iy = ((gy + 1.0f) * (float)H - 1.0f) / 2.0f;
    L.mx = fx * ((float)W / 2.0f); L.my = fy * ((float)H / 2.0f);
    if (ix <= 0.f) { ix = 0.f; L.mx = 0.f; } else if (ix >= (float)(W - 1)) { ix = (float)(W - 1); L.mx = 0.f; }
    if (iy <= 0.f) { iy = 0.f; L.my = 0.f; } else if (iy >= (float)(H - 1)) { iy = (float)(H - 1); L.my = 0.f; }
    L.finite = (ix == ix) && (iy == iy);   // NaN coordinates reach no tap (grid_sample: every tap out of bounds)
    L.ix = ix; L.iy = iy;
    return L;
}

// the bilinear value at L: up to four taps, every one inside [0, W-1] x [0, H-1]
__device__ __forceinline__ float lookup_value(const Lookup& L, const float* __restrict__ depth, long long sy, long long sx, int H, int W)
{
    float v = 0.f;
    if (L.finite) {
        const int x0 = (int)floorf(L.ix), y0 = (int)floorf(L.iy), x1 = x0 + 1, y1 = y0 + 1;   // in [0, W-1] x [0, H-1] after the clamp
        const float wx1 = L.ix - (float)x0, wx0 = (float)x1 - L.ix, wy1 = L.iy - (float)y0, wy0 = (float)y1 - L.iy;
        const bool bx1 = x1 < W, by1 = y1 < H;
        v += depth[y0 * sy + x0 * sx] * (wx0 * wy0);
        if (bx1) v += depth[y0 * sy + x1 * sx] * (wx1 * wy0);
        if (by1) v += depth[y1 * sy + x0 * sx] * (wx0 * wy1);
        if (bx1 && by1) v += depth[y1 * sy + x1 * sx] * (wx1 * wy1);
    }
    return v;
}

// backward of lookup_value under the cotangent g: (gix, giy) = dL/d(ix, iy); the four taps are ADDED into ddepth[H * W] (contiguous;
// may be NULL) with float atomics
__device__ __forceinline__ void lookup_value_bwd(const Lookup& L, const float* __restrict__ depth, long long sy, long long sx, int H, int W,
                                                 float g, float* __restrict__ ddepth, float& gix, float& giy)
{
    gix = 0.f; giy = 0.f;
    if (L.finite) {
        const int x0 = (int)floorf(L.ix), y0 = (int)floorf(L.iy), x1 = x0 + 1, y1 = y0 + 1;
        const float wx1 = L.ix - (float)x0, wx0 = (float)x1 - L.ix, wy1 = L.iy - (float)y0, wy0 = (float)y1 - L.iy;
        const bool bx1 = x1 < W, by1 = y1 < H;
        const float v00 = depth[y0 * sy + x0 * sx];
        gix -= v00 * wy0 * g; giy -= v00 * wx0 * g;
        if (ddepth) atomicAdd(&ddepth[(size_t)y0 * W + x0], wx0 * wy0 * g);
        if (bx1) {
            const float v = depth[y0 * sy + x1 * sx];
            gix += v * wy0 * g; giy -= v * wx1 * g;
            if (ddepth) atomicAdd(&ddepth[(size_t)y0 * W + x1], wx1 * wy0 * g);
        }
        if (by1) {
            const float v = depth[y1 * sy + x0 * sx];
            gix -= v * wy1 * g; giy += v * wx0 * g;
            if (ddepth) atomicAdd(&ddepth[(size_t)y1 * W + x0], wx0 * wy1 * g);
        }
        if (bx1 && by1) {
            const float v = depth[y1 * sy + x1 * sx];
            gix += v * wy1 * g; giy += v * wx1 * g;
            if (ddepth) atomicAdd(&ddepth[(size_t)y1 * W + x1], wx1 * wy1 * g);
        }
    }
}

// (gix, giy) carried on through the clamp and the projection: dL/d(x, y, z) of the point handed to lookup_coords
__device__ __forceinline__ void lookup_coords_bwd(const Lookup& L, const float* __restrict__ Pm, float gix, float giy, float& dx, float& dy,
                                                  float& dz)
{
    const float dnx = L.mx * gix, dny = L.my * giy;          // dL/d ndc
    const float dc0 = dnx / L.c3, dc1 = dny / L.c3;
    const float dc3 = -(L.ndc_x * dnx + L.ndc_y * dny) / L.c3;
    dx = Pm[0] * dc0 + Pm[1] * dc1 + Pm[3] * dc3;
    dy = Pm[4] * dc0 + Pm[5] * dc1 + Pm[7] * dc3;
    dz = Pm[8] * dc0 + Pm[9] * dc1 + Pm[11] * dc3;
}
