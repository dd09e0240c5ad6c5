// texture.hip -- the UV texture of SuGaR's refined mesh: `extract_texture_image_and_uv_from_gaussians`
//   sugar_scene/sugar_model.py:2464-2677 (called by sugar_extractors/refined_mesh.py:191-219 with n_sh = 1), the atlas
//   initialisation (:2538-2605) and the per-view baking loop (:2607-2675).
//
// The reference builds T x s(s-1)/2 x n x 3 intermediates for the atlas and, per camera, shades the whole mesh through
// pytorch3d's SoftPhongShader over an index texture, then does three boolean-mask index_put_ rounds.  Here:
//   * k_texture_atlas: one lane per texel of the finished S x S image.  The lane finds the triangle that owns it (if any), its
//     barycentrics, evaluates the triangle's n Gaussian densities and writes SH2RGB of the first densest Gaussian's DC feature
//     straight to its transposed / flipped position (unowned texels: SH2RGB(0) = 0.5).  It also zeroes counter[] and winner[].
//   * k_texture_claim: one lane per pixel of a view restates the nearest-texel lookup (pytorch3d 0.7.4's TexturesUV.sample_textures
//     with sampling_mode 'nearest', AmbientLights shading = colour x 1, softmax_rgb_blend at K = 1) and claims the texel with
//     atomicMax of ((view + 1) << 32 | pixel): the largest row-major pixel of the view wins a texel several pixels map to, which is
//     the element a serial CPU index_put_ keeps.  The view tag makes winner[] monotone: it is never cleared between views.
//   * k_texture_apply: the winning lane, and only it, does `tex = (counter ? tex : 0) + rgb; counter += 1` -- the reference's three
//     index_put_ rounds for that texel in its order, with no float atomics: bit-identical and run-to-run deterministic.
//   * k_texture_finalize: tex / max(counter, 1).
//
// Compiled with -ffp-contract=off: every float operation below is the individually rounded operation of the reference's tensor code,
// in its order (the CPU matmul of 3 x 3 by 3 x 1 accumulates from 0 over k = 0, 1, 2; sums over a dimension of 3 run in index
// order).  exp / sigmoid go through the device libm, which may differ from the host's vectorised exp in the last place.
#include "../../include/sugar_raster.h"
#include "sgr_common.h"

#include <cmath>

namespace {

#define TX_SH_C0 0.28209479177387814f   // SH2RGB, sugar_utils/spherical_harmonics.py
#define TX_SIGMA 1e-4f                  // BlendParams() defaults (sigma, gamma), pytorch3d/renderer/blending.py
#define TX_GAMMA 1e-4f
#define TX_EPS 1e-10f                   // softmax_rgb_blend's eps

// One lane per texel (r, c) of the final image.  Before the reference's transpose + flip(0) that texel was (i, j) = (c, S-1-r);
// (i, j) lies in square (i / s, j / s) -- row-major over the P x P grid of squares -- at offset (di, dj).  Triangle 2q + 0 owns
// di <= s-2, dj <= di of square q, triangle 2q + 1 owns dj >= di + 1; row di = s-1 and squares past T/2 belong to nobody.
__global__ void __launch_bounds__(256) k_texture_atlas(int T, int n, int s, int P, int S, int V, const float* __restrict__ verts,
                                                       const int64_t* __restrict__ faces, const float* __restrict__ points,
                                                       const float* __restrict__ M, const float* __restrict__ feat, int feat_stride,
                                                       float* __restrict__ tex, float* __restrict__ counter,
                                                       unsigned long long* __restrict__ winner)
{
    const int64_t texel = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t SS = (int64_t)S * S;
    if (texel >= SS) return;
    counter[texel] = 0.f;
    winner[texel] = 0ull;
    const int r = (int)(texel / S), c = (int)(texel - (int64_t)r * S);
    const int i = c, j = S - 1 - r;
    const int sq_r = i / s, sq_c = j / s;
    const int di = i - sq_r * s, dj = j - sq_c * s;
    const int64_t sq = (int64_t)sq_r * P + sq_c;
    int half = -1;
    if (di <= s - 2 && dj <= di) half = 0;
    else if (dj >= di + 1) half = 1;
    const int64_t t = 2 * sq + half;
    float f0 = 0.f, f1 = 0.f, f2 = 0.f;
    if (half >= 0 && t < T) {
        // barycentrics, :2561-2577: ((s-2-di), (dj-1)) / (s-3) for the bottom half, ((di-1), (s-1-dj)) / (s-3) for the top half
        const float den = (float)(s - 3);
        float b1, b2;
        if (half == 0) {
            b1 = (-((float)di - (float)(s - 2)) + 0.f) / den;
            b2 = (((float)dj - 1.f) + 0.f) / den;
        } else {
            b1 = (((float)di - 1.f) + 0.f) / den;
            b2 = (-((float)dj - (float)(s - 1)) + 0.f) / den;
        }
        const float b0 = 1.f - (b1 + b2);
        const int64_t v0 = faces[3 * t], v1 = faces[3 * t + 1], v2 = faces[3 * t + 2];
        if (v0 < 0 || v0 >= V || v1 < 0 || v1 >= V || v2 < 0 || v2 >= V) {   // a malformed face: visible, never an out-of-bounds read
            f0 = f1 = f2 = NAN;
        } else {
            float x[3];
            for (int k = 0; k < 3; ++k) {                                   // :2585: sum over the three corners, in order
                float a = b0 * verts[3 * v0 + k];
                a = a + b1 * verts[3 * v1 + k];
                a = a + b2 * verts[3 * v2 + k];
                x[k] = a;
            }
            int best = 0;
            float best_d = 0.f;
            for (int g = 0; g < n; ++g) {                                   // :2587-2596
                const int64_t gi = t * n + g;
                const float* mu = points + 3 * gi;
                const float* m = M + 9 * gi;                                // M[k][i] = m[3k + i]; warped = M^T (x - mu)
                const float sh0 = x[0] - mu[0], sh1 = x[1] - mu[1], sh2 = x[2] - mu[2];
                float q = 0.f;
                for (int ii = 0; ii < 3; ++ii) {
                    float w = 0.f;
                    w = w + m[ii] * sh0;
                    w = w + m[3 + ii] * sh1;
                    w = w + m[6 + ii] * sh2;
                    q = q + w * w;
                }
                q = fminf(fmaxf(q, 0.f), 1e8f);
                const float d = expf(-0.5f * q);
                if (g == 0 || d > best_d) { best = g; best_d = d; }        // strict '>': the first maximum, as torch.argmax
            }
            const float* fp = feat + (t * n + best) * (int64_t)feat_stride;
            f0 = fp[0]; f1 = fp[1]; f2 = fp[2];
        }
    }
    float* o = tex + 3 * texel;
    o[0] = f0 * TX_SH_C0 + 0.5f;
    o[1] = f1 * TX_SH_C0 + 0.5f;
    o[2] = f2 * TX_SH_C0 + 0.5f;
}

// The texel a covered pixel lands on (flat index a * S + b into the final image), or -1: :2656-2661 restated --
//   uv = sum_k bary_k uv_k (interpolate_face_attributes); grid_sample(nearest, align_corners, border) of the y-flipped index map
//   (x = (u*2-1 + 1) * (S-1)/2, clamped to [0, S-1], rounded half to even); colour = (S-1-row, col, 0) x ambient 1;
//   softmax_rgb_blend at K = 1, background 0; then round() of channels 0 and 1.
__device__ __forceinline__ int64_t texel_of_pixel(int64_t p, int T, int S, const int64_t* __restrict__ p2f, const float* __restrict__ bary,
                                                  const float* __restrict__ zbuf, const float* __restrict__ dists, float znear,
                                                  float zfar, const float* __restrict__ verts_uv)
{
    const float z = zbuf[p];
    if (!(z > 0.f)) return -1;                                              // update_mask = zbuf > 0
    const int64_t f = p2f[p];
    if (f < 0 || f >= T) return -1;
    const float b0 = bary[3 * p], b1 = bary[3 * p + 1], b2 = bary[3 * p + 2];
    const float* uv = verts_uv + 6 * f;                                     // faces_uv[f] = (3f, 3f+1, 3f+2)
    float u = b0 * uv[0];
    u = u + b1 * uv[2];
    u = u + b2 * uv[4];
    float v = b0 * uv[1];
    v = v + b1 * uv[3];
    v = v + b2 * uv[5];
    const float gx = u * 2.f - 1.f, gy = v * 2.f - 1.f;
    const float mx = (float)(S - 1), hs = (float)(S - 1) / 2.f;
    const float ix = fminf(mx, fmaxf((gx + 1.f) * hs, 0.f));
    const float iy = fminf(mx, fmaxf((gy + 1.f) * hs, 0.f));
    if (!(ix == ix) || !(iy == iy)) return -1;
    const float col = rintf(ix), row = rintf(iy);
    const float c0 = mx - row, c1 = col;                                    // flipped map: texel_idx[S-1-row, col] = (S-1-row, col, 0)
    // softmax_rgb_blend (pytorch3d/renderer/blending.py), K = 1, covered pixel (mask = 1)
    const float prob = 1.f / (1.f + expf(-((-dists[p]) / TX_SIGMA)));
    const float zi = (zfar - z) / (zfar - znear);
    const float zmax = fmaxf(zi, TX_EPS);
    const float w = prob * expf((zi - zmax) / TX_GAMMA);
    const float delta = fmaxf(expf((TX_EPS - zmax) / TX_GAMMA), TX_EPS);
    const float den = w + delta;
    const float a = rintf((w * c0) / den), b = rintf((w * c1) / den);
    if (!(a >= 0.f && a <= mx && b >= 0.f && b <= mx)) return -1;
    return (int64_t)a * S + (int64_t)b;
}

__global__ void __launch_bounds__(256) k_texture_claim(int64_t n_pix, unsigned long long tag_hi, int T, int S,
                                                       const int64_t* __restrict__ p2f, const float* __restrict__ bary,
                                                       const float* __restrict__ zbuf, const float* __restrict__ dists, float znear,
                                                       float zfar, const float* __restrict__ verts_uv, unsigned long long* winner)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pix) return;
    const int64_t t = texel_of_pixel(p, T, S, p2f, bary, zbuf, dists, znear, zfar, verts_uv);
    if (t >= 0) atomicMax(winner + t, tag_hi | (unsigned long long)p);
}

__global__ void __launch_bounds__(256) k_texture_apply(int64_t n_pix, int width, unsigned long long tag_hi, int T, int S,
                                                       const int64_t* __restrict__ p2f, const float* __restrict__ bary,
                                                       const float* __restrict__ zbuf, const float* __restrict__ dists, float znear,
                                                       float zfar, const float* __restrict__ verts_uv, const float* __restrict__ rgb,
                                                       int64_t sh, int64_t sw, int64_t sc, const unsigned long long* __restrict__ winner,
                                                       float* __restrict__ tex, float* __restrict__ counter)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pix) return;
    const int64_t t = texel_of_pixel(p, T, S, p2f, bary, zbuf, dists, znear, zfar, verts_uv);
    if (t < 0 || winner[t] != (tag_hi | (unsigned long long)p)) return;
    const int64_t y = p / width, x = p - y * width;
    const float* src = rgb + y * sh + x * sw;
    float* o = tex + 3 * t;
    const float cnt = counter[t];
    const bool keep = cnt != 0.f;                                           // :2666-2667: the init colour goes on the first visit
    o[0] = (keep ? o[0] : 0.f) + src[0];
    o[1] = (keep ? o[1] : 0.f) + src[sc];
    o[2] = (keep ? o[2] : 0.f) + src[2 * sc];
    counter[t] = cnt + 1.f;
}

__global__ void __launch_bounds__(256) k_texture_finalize(int64_t SS, const float* __restrict__ tex, const float* __restrict__ counter,
                                                          float* __restrict__ out)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= SS) return;
    const float d = fmaxf(counter[t], 1.f);                                 // texture_counter.clamp(min=1)
    out[3 * t] = tex[3 * t] / d;
    out[3 * t + 1] = tex[3 * t + 1] / d;
    out[3 * t + 2] = tex[3 * t + 2] / d;
}

// P = int(sqrt(T // 2 + 1) + 1), :2487-2488
int squares_per_axis(int T) { return (int)(std::sqrt((double)(T / 2 + 1)) + 1.0); }

const int64_t kMaxTexels = (int64_t)1 << 31;

}  // namespace

extern "C" {

int sgr_texture_size(int T, int square_size)
{
    if (T <= 0 || square_size < 3) return SGR_E_INVALID;
    const int64_t S = (int64_t)square_size * squares_per_axis(T);
    return (S * S >= kMaxTexels) ? SGR_E_INVALID : (int)S;
}

int sgr_texture_atlas(int T, int n, int square_size, int V, const float* verts, const int64_t* faces, const float* points,
                      const float* inv_scaled_rot, const float* features_dc, int feat_stride, int S, float* texture, float* counter,
                      uint64_t* winner_u64, void* stream)
{
    unsigned long long* winner = reinterpret_cast<unsigned long long*>(winner_u64);
    if (T <= 0 || n <= 0 || V <= 0 || square_size < 3 || feat_stride < 3)
        return sgr_fail(SGR_E_INVALID, "texture_atlas: T, n, V must be positive, square_size >= 3, feat_stride >= 3");
    if (!verts || !faces || !points || !inv_scaled_rot || !features_dc || !texture || !counter || !winner)
        return sgr_fail(SGR_E_INVALID, "texture_atlas: null pointer");
    if (sgr_texture_size(T, square_size) != S)
        return sgr_fail(SGR_E_INVALID, "texture_atlas: S must be square_size * int(sqrt(T // 2 + 1) + 1) (and S^2 < 2^31)");
    if ((int64_t)T * n >= kMaxTexels) return sgr_fail(SGR_E_INVALID, "texture_atlas: too many Gaussians");
    const int64_t SS = (int64_t)S * S;
    hipLaunchKernelGGL(k_texture_atlas, dim3((unsigned)((SS + 255) / 256)), dim3(256), 0, (hipStream_t)stream, T, n, square_size,
                       S / square_size, S, V, verts, faces, points, inv_scaled_rot, features_dc, feat_stride, texture, counter, winner);
    return hipGetLastError() == hipSuccess ? 0 : sgr_fail(SGR_E_HIP, "texture_atlas: launch failed");
}

int sgr_texture_bake_view(int width, int height, int view, const int64_t* pix_to_face, const float* bary, const float* zbuf,
                          const float* dists, float znear, float zfar, int T, const float* verts_uv, const float* rgb,
                          int64_t rgb_stride_h, int64_t rgb_stride_w, int64_t rgb_stride_c, int S, uint64_t* winner_u64,
                          float* texture, float* counter, void* stream)
{
    unsigned long long* winner = reinterpret_cast<unsigned long long*>(winner_u64);
    if (width <= 0 || height <= 0 || T <= 0 || view < 0 || view >= 0x7FFFFFFF)
        return sgr_fail(SGR_E_INVALID, "texture_bake_view: width, height, T must be positive, 0 <= view < 2^31 - 1");
    const int64_t n_pix = (int64_t)width * height;
    if (n_pix > 0xFFFFFFFFll) return sgr_fail(SGR_E_INVALID, "texture_bake_view: more than 2^32 - 1 pixels");
    if (S <= 0 || (int64_t)S * S >= kMaxTexels) return sgr_fail(SGR_E_INVALID, "texture_bake_view: bad texture size");
    if (!pix_to_face || !bary || !zbuf || !dists || !verts_uv || !rgb || !winner || !texture || !counter)
        return sgr_fail(SGR_E_INVALID, "texture_bake_view: null pointer");
    if (rgb_stride_h < 0 || rgb_stride_w < 0 || rgb_stride_c < 0) return sgr_fail(SGR_E_INVALID, "texture_bake_view: negative rgb stride");
    const unsigned long long tag_hi = (unsigned long long)(view + 1) << 32;
    const dim3 grid((unsigned)((n_pix + 255) / 256));
    hipLaunchKernelGGL(k_texture_claim, grid, dim3(256), 0, (hipStream_t)stream, n_pix, tag_hi, T, S, pix_to_face, bary, zbuf, dists,
                       znear, zfar, verts_uv, winner);
    hipLaunchKernelGGL(k_texture_apply, grid, dim3(256), 0, (hipStream_t)stream, n_pix, width, tag_hi, T, S, pix_to_face, bary, zbuf,
                       dists, znear, zfar, verts_uv, rgb, rgb_stride_h, rgb_stride_w, rgb_stride_c, winner, texture, counter);
    return hipGetLastError() == hipSuccess ? 0 : sgr_fail(SGR_E_HIP, "texture_bake_view: launch failed");
}

int sgr_texture_finalize(int S, const float* texture, const float* counter, float* out, void* stream)
{
    if (S <= 0 || (int64_t)S * S >= kMaxTexels || !texture || !counter || !out)
        return sgr_fail(SGR_E_INVALID, "texture_finalize: bad size or null pointer");
    const int64_t SS = (int64_t)S * S;
    hipLaunchKernelGGL(k_texture_finalize, dim3((unsigned)((SS + 255) / 256)), dim3(256), 0, (hipStream_t)stream, SS, texture, counter, out);
    return hipGetLastError() == hipSuccess ? 0 : sgr_fail(SGR_E_HIP, "texture_finalize: launch failed");
}

}  // extern "C"
