// mesh_shade.hip -- shading of a UV-textured mesh from its hard fragments: pytorch3d 0.7.4's
//   SoftPhongShader(AmbientLights, default Materials) over a TexturesUV, i.e. TexturesUV.sample_textures (interpolate_face_attributes,
//   F.grid_sample of the y-flipped map, 'nearest' or 'bilinear', padding_mode 'border'), colour = ambient x texel, softmax_rgb_blend --
//   what metrics.py:260-300, 370-372 renders the refined mesh's .obj with.  One kernel, one lane per pixel in row-major order.
//
// The torch formulation gathers [H,W,K,3,2] UVs, copies the whole flipped map and runs grid_sample and ~15 element-wise launches.  Here a
// lane reads its K fragments (coalesced), per covered face the three UV rows and the one (nearest) or four (bilinear) texels, read in
// place at row TH-1-iy of the map as stored, and keeps the softmax in registers: two passes over the K slots (the largest inverse depth
// first, then the weights), no LDS, no atomics, no arrays.
//
// Compiled with -ffp-contract=off: every float operation is the individually rounded operation of the stand-in's tensor code
// (sugar_amd/shims/pytorch3d/renderer/mesh/shader.py, blending.py), in its order.  exp goes through the device libm, which may differ
// from the host's vectorised exp in the last place.
#include "../../include/sugar_raster.h"
#include "sgr_common.h"

#include <cmath>

namespace {

#define MS_EPS 1e-10f        // softmax_rgb_blend's eps
#define MS_MAX_K 16          // MAX_FACES_PER_PIXEL of the mesh rasterizer

struct ShadeParams {
    int64_t n_pix;
    int K;
    int64_t face_base, F, n_uv;
    int TH, TW, bilinear, align_corners;
    float ambient[3], background[3];
    float sigma, gamma, znear, zfar;
};

// grid_sampler_unnormalize + clip_coordinates (padding_mode 'border') of one coordinate; a NaN comes out as 0 (fmaxf), in bounds
__device__ __forceinline__ float unnormalize(float g, int size, int align_corners)
{
    const float x = align_corners ? ((g + 1.f) / 2.f) * (float)(size - 1) : ((g + 1.f) * (float)size - 1.f) / 2.f;
    return fminf((float)(size - 1), fmaxf(x, 0.f));
}

// texel (iy, ix) of the y-flipped map = row TH-1-iy of the map as stored; (iy, ix) must be in bounds
__device__ __forceinline__ const float* texel_ptr(const float* __restrict__ tex, int TH, int TW, int iy, int ix)
{
    return tex + ((int64_t)(TH - 1 - iy) * TW + ix) * 3;
}

// the colour of face slot (texel only, before the ambient factor); false = a face or UV index out of range
__device__ __forceinline__ bool sample_face(const ShadeParams& P, int64_t f, float b0, float b1, float b2,
                                            const int64_t* __restrict__ faces_uvs, const float* __restrict__ verts_uvs,
                                            const float* __restrict__ tex, float c[3])
{
    if (f < 0 || f >= P.F) return false;
    const int64_t i0 = faces_uvs[3 * f], i1 = faces_uvs[3 * f + 1], i2 = faces_uvs[3 * f + 2];
    if (i0 < 0 || i0 >= P.n_uv || i1 < 0 || i1 >= P.n_uv || i2 < 0 || i2 >= P.n_uv) return false;
    // interpolate_face_attributes: sum over the three corners, in order
    float u = b0 * verts_uvs[2 * i0];
    u = u + b1 * verts_uvs[2 * i1];
    u = u + b2 * verts_uvs[2 * i2];
    float v = b0 * verts_uvs[2 * i0 + 1];
    v = v + b1 * verts_uvs[2 * i1 + 1];
    v = v + b2 * verts_uvs[2 * i2 + 1];
    const float x = unnormalize(u * 2.f - 1.f, P.TW, P.align_corners);
    const float y = unnormalize(v * 2.f - 1.f, P.TH, P.align_corners);
    if (!P.bilinear) {
        const int ix = (int)nearbyintf(x), iy = (int)nearbyintf(y);       // half to even; inside [0, size-1] after the clamp
        const float* t = texel_ptr(tex, P.TH, P.TW, iy, ix);
        c[0] = t[0]; c[1] = t[1]; c[2] = t[2];
        return true;
    }
    // grid_sample 'bilinear': corners nw, ne, sw, se with the weights of the opposite corner's rectangle; a corner outside adds 0
    const float x0 = floorf(x), y0 = floorf(y);
    const float x1 = x0 + 1.f, y1 = y0 + 1.f;
    const float w_nw = (x1 - x) * (y1 - y), w_ne = (x - x0) * (y1 - y), w_sw = (x1 - x) * (y - y0), w_se = (x - x0) * (y - y0);
    const int ix0 = (int)x0, iy0 = (int)y0;                                // in [0, size-1]
    const bool in_x1 = ix0 + 1 < P.TW, in_y1 = iy0 + 1 < P.TH;
    // (all four reads are issued unconditionally, a corner outside the map from its in-bounds neighbour's address, and dropped by a
    // select: no divergent branch sits between the loads)
    const float* t_nw = texel_ptr(tex, P.TH, P.TW, iy0, ix0);
    const float* t_ne = t_nw + (in_x1 ? 3 : 0);
    const float* t_sw = t_nw - (in_y1 ? (int64_t)3 * P.TW : 0);            // one row down in the flipped map = one row up as stored
    const float* t_se = t_sw + (in_x1 ? 3 : 0);
    for (int ch = 0; ch < 3; ++ch) {
        float a = t_nw[ch] * w_nw;
        const float a_ne = a + t_ne[ch] * w_ne;
        a = in_x1 ? a_ne : a;
        const float a_sw = a + t_sw[ch] * w_sw;
        a = in_y1 ? a_sw : a;
        const float a_se = a + t_se[ch] * w_se;
        a = (in_x1 && in_y1) ? a_se : a;
        c[ch] = a;
    }
    return true;
}

// KT > 0: K known at compile time (the loops unroll); KT = 0: K = P.K at run time
template <int KT>
__global__ void __launch_bounds__(256) k_shade_texture_uv(ShadeParams P, const int64_t* __restrict__ p2f, const float* __restrict__ bary,
                                                          const float* __restrict__ zbuf, const float* __restrict__ dists,
                                                          const int64_t* __restrict__ faces_uvs, const float* __restrict__ verts_uvs,
                                                          const float* __restrict__ tex, float* __restrict__ rgba)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P.n_pix) return;
    const int K = KT > 0 ? KT : P.K;
    const int64_t s0 = p * K;
    const float zrange = P.zfar - P.znear;
    // pass 1: alpha = prod(1 - prob), z_inv_max = max(z_inv) over all K slots (an empty slot has z_inv = 0)
    float alpha = 1.f, zmax = -INFINITY;
    for (int k = 0; k < K; ++k) {
        const bool covered = p2f[s0 + k] >= 0;
        const float prob = covered ? 1.f / (1.f + expf(-((-dists[s0 + k]) / P.sigma))) : 0.f;
        alpha = alpha * (1.f - prob);
        const float zi = covered ? (P.zfar - zbuf[s0 + k]) / zrange : 0.f;
        zmax = fmaxf(zmax, zi);
    }
    zmax = fmaxf(zmax, MS_EPS);
    // pass 2: the weights and the weighted colours
    float wsum = 0.f, c0 = 0.f, c1 = 0.f, c2 = 0.f;
    bool bad = false;
    for (int k = 0; k < K; ++k) {
        const int64_t pf = p2f[s0 + k];
        if (pf < 0) continue;                                              // prob = 0: weight 0, the slot adds nothing
        const float prob = 1.f / (1.f + expf(-((-dists[s0 + k]) / P.sigma)));
        const float zi = (P.zfar - zbuf[s0 + k]) / zrange;
        const float w = prob * expf((zi - zmax) / P.gamma);
        const float* b = bary + 3 * (s0 + k);
        float t[3];
        if (!sample_face(P, pf - P.face_base, b[0], b[1], b[2], faces_uvs, verts_uvs, tex, t)) {
            bad = true;
            continue;
        }
        wsum = wsum + w;
        c0 = c0 + w * (P.ambient[0] * t[0]);
        c1 = c1 + w * (P.ambient[1] * t[1]);
        c2 = c2 + w * (P.ambient[2] * t[2]);
    }
    const float delta = fmaxf(expf((MS_EPS - zmax) / P.gamma), MS_EPS);
    const float den = wsum + delta;
    float4 out;
    out.x = (c0 + delta * P.background[0]) / den;
    out.y = (c1 + delta * P.background[1]) / den;
    out.z = (c2 + delta * P.background[2]) / den;
    out.w = 1.f - alpha;
    if (bad) out.x = out.y = out.z = out.w = NAN;                          // a malformed index: visible, never an out-of-bounds read
    reinterpret_cast<float4*>(rgba)[p] = out;
}

}  // namespace

extern "C" {

int sgr_shade_texture_uv(int width, int height, int K, int64_t face_index_base, const int64_t* pix_to_face, const float* bary,
                         const float* zbuf, const float* dists, int64_t F, const int64_t* faces_uvs, int64_t n_uv,
                         const float* verts_uvs, const float* texture, int TH, int TW, int bilinear, int align_corners,
                         const float* ambient3, const float* background3, float sigma, float gamma, float znear, float zfar,
                         float* rgba, void* stream)
{
    if (width <= 0 || height <= 0) return sgr_fail(SGR_E_INVALID, "shade_texture_uv: width and height must be positive");
    if (K < 1 || K > MS_MAX_K) return sgr_fail(SGR_E_INVALID, "shade_texture_uv: K must be in 1..16");
    if (F <= 0 || n_uv <= 0 || TH <= 0 || TW <= 0) return sgr_fail(SGR_E_INVALID, "shade_texture_uv: F, n_uv, TH, TW must be positive");
    if (!pix_to_face || !bary || !zbuf || !dists || !faces_uvs || !verts_uvs || !texture || !ambient3 || !background3 || !rgba)
        return sgr_fail(SGR_E_INVALID, "shade_texture_uv: null pointer");
    if ((reinterpret_cast<uintptr_t>(rgba) & 15) != 0) return sgr_fail(SGR_E_INVALID, "shade_texture_uv: rgba must be 16-byte aligned");
    ShadeParams P;
    P.n_pix = (int64_t)width * height;
    if (P.n_pix > (int64_t)0x7FFFFFFF * 256) return sgr_fail(SGR_E_INVALID, "shade_texture_uv: too many pixels");
    P.K = K;
    P.face_base = face_index_base;
    P.F = F;
    P.n_uv = n_uv;
    P.TH = TH;
    P.TW = TW;
    P.bilinear = bilinear != 0;
    P.align_corners = align_corners != 0;
    for (int c = 0; c < 3; ++c) {
        P.ambient[c] = ambient3[c];
        P.background[c] = background3[c];
    }
    P.sigma = sigma;
    P.gamma = gamma;
    P.znear = znear;
    P.zfar = zfar;
    const dim3 grid((unsigned)((P.n_pix + 255) / 256));
    if (K == 1)
        hipLaunchKernelGGL(k_shade_texture_uv<1>, grid, dim3(256), 0, (hipStream_t)stream, P, pix_to_face, bary, zbuf, dists, faces_uvs,
                           verts_uvs, texture, rgba);
    else
        hipLaunchKernelGGL(k_shade_texture_uv<0>, grid, dim3(256), 0, (hipStream_t)stream, P, pix_to_face, bary, zbuf, dists, faces_uvs,
                           verts_uvs, texture, rgba);
    return hipGetLastError() == hipSuccess ? 0 : sgr_fail(SGR_E_HIP, "shade_texture_uv: launch failed");
}

}  // extern "C"
