// sh_adam.hip -- the SH half of the optimiser for gfx950: the SH gradient summed over the views, Adam on the SH block straight from
// the per-view colour gradients (dense, with the view-direction term, or masked by reach flag), the zero-gradient half of the split
// as launches of their own, and their C entry points (include/sugar_raster.h: sgr_sh_grad_from_views, sgr_sh_adam_*).
//
// Arithmetic contract: this translation unit is compiled with -ffp-contract=off, as preprocess.hip is, whose backward these kernels
// restate: every float op is an individually rounded IEEE operation in the order written.  The dense and the masked kernel and the
// zero-gradient waves therefore leave the same bits, and all of them update a coefficient with the one function sh_adam_update
// (sh_adam_update.h) that blend.hip carries for the ride-along in the blend backward's launch.
//
// The host's description of a step is SgrShAdamHyper (sgr_common.h): the entry points here and sgr_trainer_step fill it through
// sgr_sh_adam_hyper, and the kernels' ShAdamArgs / SgrShAdamJob are copies of it.
#include "../../include/sugar_raster.h"
#include "sgr_common.h"
#include "sgr_sh.h"
#include "sh_adam_update.h"

#include <string>

namespace {

// dL/dmean3D through the view direction, summed over the views (the tail of the backward preprocess kernel,
// backward.cu:99-139 + dnormvdv, moved next to the only other reader of the SH coefficients; `row` = this Gaussian's 48
// coefficients in LDS).  Same arithmetic, operation for operation, as k_preprocess_bwd (sh_backward).  One colour channel at
// a time, its 16 coefficients fetched from the LDS row: with all 48 in registers next to the expanded polynomial the kernel
// needed 190 VGPRs, two waves per SIMD, and lost in bandwidth what the backward preprocess kernel saved.
__device__ __forceinline__ void sh_dir_sum_over_views(int idx, size_t P, int V, int D, const float* __restrict__ means3D,
                                                      const float* __restrict__ campos, const float* __restrict__ dcolor,
                                                      const float* row, float* dm)
{
    const size_t i3 = 3 * (size_t)idx;
    const float mx = means3D[i3], my = means3D[i3 + 1], mz = means3D[i3 + 2];
    dm[0] = 0.f; dm[1] = 0.f; dm[2] = 0.f;
    for (int v = 0; v < V; v++) {
        const float* g = dcolor + ((size_t)v * P + idx) * 3;
        const float g0 = g[0], g1 = g[1], g2 = g[2];
        if (g0 == 0.f && g1 == 0.f && g2 == 0.f) continue;  // culled or fully clamped in this view
        const float dx = mx - campos[3 * v], dy = my - campos[3 * v + 1], dz = mz - campos[3 * v + 2];
        const float len = sqrtf(dx * dx + dy * dy + dz * dz);
        const float x = dx / len, y = dy / len, z = dz / len;
        float dL_ddir[3] = {0.f, 0.f, 0.f};
#pragma unroll 1
        for (int c = 0; c < 3; c++) {
            float h[16];
#pragma unroll
            for (int k = 0; k < 16; k++) h[k] = row[3 * k + c];
            const float dL_dRGB = (c == 0 ? g0 : (c == 1 ? g1 : g2)) * 1.0f;  // (sh_backward's mask factor: the colours arrive masked)
            float dRGBdx, dRGBdy, dRGBdz;
            sh_dir_channel(D, h, x, y, z, dRGBdx, dRGBdy, dRGBdz);
            dL_ddir[0] += dRGBdx * dL_dRGB; dL_ddir[1] += dRGBdy * dL_dRGB; dL_ddir[2] += dRGBdz * dL_dRGB;
        }
        // dnormvdv, auxiliary.h:107-117
        const float sum2 = dx * dx + dy * dy + dz * dz;
        const float invsum32 = 1.0f / sqrtf(sum2 * sum2 * sum2);
        dm[0] += ((+sum2 - dx * dx) * dL_ddir[0] - dy * dx * dL_ddir[1] - dz * dx * dL_ddir[2]) * invsum32;
        dm[1] += (-dx * dy * dL_ddir[0] + (sum2 - dy * dy) * dL_ddir[1] - dz * dy * dL_ddir[2]) * invsum32;
        dm[2] += (-dx * dz * dL_ddir[0] - dy * dz * dL_ddir[1] + (sum2 - dz * dz) * dL_ddir[2]) * invsum32;
    }
}

// dL/dsh[k][c] = sum over views v of  basis_k(dir_v) * g_v[c]   with dir_v = normalize(mean - campos_v) and g_v the
// clamp-masked dL/dRGB of view v -- exactly the per-view SH backward (backward.cu:47-97) summed over views, but the views
// exchange 3 floats per Gaussian instead of 3*M.  dirs use the same arithmetic as the forward (glm::length, division).
// The basis values are spelled out here a third time, next to sh_basis16 and sh_backward (sgr_sh.h), on purpose: a call to
// sh_basis16 zero-initialises b[] first, and that changes the instructions of k_sh_grad_from_views and of all three
// k_sh_adam_from_views instances.  Keep the body as it is.
__device__ __forceinline__ void sh_grad_sum_over_views(int idx, size_t P, int V, int D, const float* __restrict__ means3D,
                                                       const float* __restrict__ campos, const float* __restrict__ dcolor,
                                                       float* acc)
{
    const size_t i3 = 3 * (size_t)idx;
    const float mx = means3D[i3], my = means3D[i3 + 1], mz = means3D[i3 + 2];
#pragma unroll
    for (int k = 0; k < 48; k++) acc[k] = 0.f;
    for (int v = 0; v < V; v++) {
        const float* g = dcolor + ((size_t)v * P + idx) * 3;
        const float g0 = g[0], g1 = g[1], g2 = g[2];
        if (g0 == 0.f && g1 == 0.f && g2 == 0.f) continue;  // culled or fully clamped in this view
        float dx = mx - campos[3 * v], dy = my - campos[3 * v + 1], dz = mz - campos[3 * v + 2];
        const float len = sqrtf(dx * dx + dy * dy + dz * dz);
        const float x = dx / len, y = dy / len, z = dz / len;
        float b[16];
        b[0] = SH_C0;
        if (D > 0) {
            b[1] = -SH_C1 * y; b[2] = SH_C1 * z; b[3] = -SH_C1 * x;
            if (D > 1) {
                const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
                b[4] = SH_C2[0] * xy; b[5] = SH_C2[1] * yz; b[6] = SH_C2[2] * (2.f * zz - xx - yy);
                b[7] = SH_C2[3] * xz; b[8] = SH_C2[4] * (xx - yy);
                if (D > 2) {
                    b[9] = SH_C3[0] * y * (3.f * xx - yy); b[10] = SH_C3[1] * xy * z;
                    b[11] = SH_C3[2] * y * (4.f * zz - xx - yy); b[12] = SH_C3[3] * z * (2.f * zz - 3.f * xx - 3.f * yy);
                    b[13] = SH_C3[4] * x * (4.f * zz - xx - yy); b[14] = SH_C3[5] * z * (xx - yy);
                    b[15] = SH_C3[6] * x * (xx - 3.f * yy);
                }
            }
        }
        const int nb = (D + 1) * (D + 1);
#pragma unroll
        for (int k = 0; k < 16; k++) {
            if (k < nb) { acc[3 * k] += b[k] * g0; acc[3 * k + 1] += b[k] * g1; acc[3 * k + 2] += b[k] * g2; }
        }
    }
}

__global__ void __launch_bounds__(256) k_sh_grad_from_views(int P, int V, int D, int M, size_t vstride,
                                                            const float* __restrict__ means3D,
                                                            const float* __restrict__ campos, const float* __restrict__ dcolor,
                                                            float* __restrict__ dL_dsh)
{
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= P) return;
    float acc[48];
    sh_grad_sum_over_views(idx, vstride, V, D, means3D, campos, dcolor, acc);
    const int n_sh = 3 * M;
    float* dst = dL_dsh + (size_t)idx * n_sh;
    if (n_sh == 48 && ((uintptr_t)dst & 15) == 0) {
        float4* d4 = reinterpret_cast<float4*>(dst);
#pragma unroll
        for (int i = 0; i < 12; i++) { float4 o = {acc[4 * i], acc[4 * i + 1], acc[4 * i + 2], acc[4 * i + 3]}; d4[i] = o; }
    } else {
#pragma unroll
        for (int i = 0; i < 48; i++) if (i < n_sh) dst[i] = acc[i];
    }
}

// The same sum, consumed on the spot: Adam on the Gaussian's SH coefficients (adam.hip's update, lr_dc for the three DC
// values and lr_rest for the others: gaussian_model.py:157-158) without ever writing the 48-float gradient to memory.
struct ShAdamArgs {
    float lr_dc, lr_rest, b1, b2, omb1, omb2, eps, bc1, bc2_sqrt, grad_scale;
    const uint32_t* guard; uint32_t guard_cap;  // forward header + list capacity: the step is a no-op if that forward was invalid (NULL: no check)
    uint8_t* reach;  // MASKED: the reach flags (sh_adam_update.h)
};

// One wave per 64 Gaussians.  Phase 1: lane = Gaussian, the 48 sums in registers, dropped into an LDS panel (row stride 52
// floats: conflict-free for 16-byte accesses).  Phase 2: the wave walks the 64 x 48 floats of parameters and moments as
// one contiguous stream, one float4 per lane and step (a lane-per-Gaussian walk touches 64 cache lines per instruction
// and ran at 2 TB/s).
#define SHA_STRIDE 52
// DIR (dmean_extra != NULL, M == 16): phase 1 also loads the Gaussian's 48 coefficients (the wave's 12 KB block, which
// phase 2 then streams out of the cache) and writes the view-direction part of dL/dmean3D, summed over the views, to
// dmean_extra[P][3]; the flat Adam kernel adds it to the position gradient (sgr_adam_step_ex).
// MASKED (M == 16, aligned buffers, no DIR): only the rows whose reach flag is set are updated -- the others got their zero-gradient
// step from sgr_sh_adam_zero_wave --, and the wave puts its 64 flags back to 0 (it is their last reader, as k_preprocess_bwd is the
// accumulator table's).  Unflagged rows run no phase 1 and load no colour, and phase 2 walks the flagged rows only: their lane
// numbers are compacted into an LDS list, and the stream is n_flagged x 12 float4 instead of 64 x 12 (a fifth of the steps on the
// metric scene; clamped addresses as below, not lane-predicated loads).
template <bool DIR, bool MASKED = false>
__global__ void __launch_bounds__(64) k_sh_adam_from_views(int P, int V, int D, int M, size_t vstride,
                                                           const float* __restrict__ means3D,
                                                           const float* __restrict__ campos, const float* __restrict__ dcolor,
                                                           float* __restrict__ sh, float* __restrict__ exp_avg,
                                                           float* __restrict__ exp_avg_sq, ShAdamArgs a,
                                                           float* __restrict__ dmean_extra)
{
    __shared__ __attribute__((aligned(16))) float s_g[64 * SHA_STRIDE];
    if (a.guard && SGR_FORWARD_INVALID(a.guard, a.guard_cap)) return;
    const int lane = threadIdx.x;
    const int g0 = blockIdx.x * 64;
    const int idx = g0 + lane;
    unsigned long long flagged = ~0ull;  // MASKED: bit g <=> row g0 + g is updated here
    if (MASKED) {
        flagged = __ballot(idx < P && a.reach[min(idx, P - 1)] != 0);
        if (flagged == 0ull) return;
    }
    float4 pkeep[12];  // DIR: the wave's 64 x 48 coefficients in the streaming layout of phase 2 (read from memory once)
    if (DIR) {
        // coalesced into the panel (row = Gaussian) for the direction term, and kept in registers for the Adam update
        // (12 loads at a 192-byte lane stride straight from memory cost this streaming kernel 25 us; re-reading the block in
        // phase 2 gives back what the backward preprocess kernel saved)
        const float4* p4 = reinterpret_cast<const float4*>(sh + (size_t)g0 * 48);
        const int n4 = min(64, P - g0) * 12;
#pragma unroll
        for (int st = 0; st < 12; st++) pkeep[st] = p4[min(st * 64 + lane, n4 - 1)];
#pragma unroll
        for (int st = 0; st < 12; st++) {
            const int e4 = st * 64 + lane;
            if (e4 < n4) { const int g = e4 / 12; *reinterpret_cast<float4*>(s_g + g * SHA_STRIDE + 4 * (e4 - g * 12)) = pkeep[st]; }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    if (DIR && idx < P) {
        float dm[3];
        sh_dir_sum_over_views(idx, vstride, V, D, means3D, campos, dcolor, s_g + lane * SHA_STRIDE, dm);
        dmean_extra[3 * (size_t)idx] = dm[0]; dmean_extra[3 * (size_t)idx + 1] = dm[1]; dmean_extra[3 * (size_t)idx + 2] = dm[2];
    }
    if (DIR) {  // every lane is done with its coefficients before any lane overwrites a row with gradient sums
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    {
        float acc[48];
        if (idx < P && ((flagged >> lane) & 1ull)) {
            sh_grad_sum_over_views(idx, vstride, V, D, means3D, campos, dcolor, acc);
        } else {
#pragma unroll
            for (int k = 0; k < 48; k++) acc[k] = 0.f;
        }
        float4* row = reinterpret_cast<float4*>(s_g + lane * SHA_STRIDE);
#pragma unroll
        for (int i = 0; i < 12; i++) row[i] = make_float4(acc[4 * i], acc[4 * i + 1], acc[4 * i + 2], acc[4 * i + 3]);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const int n_sh = 3 * M;
    const int live = min(64, P - g0);
    auto upd = [&](int c, float g, float& p, float& m, float& v) {
        sh_adam_update(g, p, m, v, c < 3 ? a.lr_dc : a.lr_rest, a.grad_scale, a.b1, a.b2, a.omb1, a.omb2, a.eps, a.bc1, a.bc2_sqrt);
    };
    const size_t base = (size_t)g0 * n_sh;
    if (MASKED) {  // (n_sh == 48 and aligned buffers: the launcher's callers have checked)
        typedef float f4 __attribute__((ext_vector_type(4)));
        __shared__ int s_row[64];  // the flagged rows of the wave, in order
        const int n4f = 12 * __popcll(flagged);
        if ((flagged >> lane) & 1ull)
            s_row[__builtin_amdgcn_mbcnt_hi((uint32_t)(flagged >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)flagged, 0u))] = lane;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        f4* p4 = reinterpret_cast<f4*>(sh + base);
        f4* m4 = reinterpret_cast<f4*>(exp_avg + base);
        f4* v4 = reinterpret_cast<f4*>(exp_avg_sq + base);
        constexpr int NB = 4;
#pragma clang loop unroll(disable)
        for (int st0 = 0; st0 * 64 < n4f; st0 += NB) {
            f4 pv[NB], mv[NB], vv[NB];
            int ee[NB];
#pragma unroll
            for (int u = 0; u < NB; u++) {
                const int j = min((st0 + u) * 64 + lane, n4f - 1);  // float4 index inside the compacted stream
                const int r = j / 12;
                ee[u] = s_row[r] * 12 + (j - r * 12);                // ... and inside the wave's 64 x 48 block
                pv[u] = p4[ee[u]];
                mv[u] = __builtin_nontemporal_load(&m4[ee[u]]); vv[u] = __builtin_nontemporal_load(&v4[ee[u]]);
            }
#pragma unroll
            for (int u = 0; u < NB; u++) {
                if ((st0 + u) * 64 + lane < n4f) {
                    const int e4 = ee[u], g = e4 / 12, c4 = e4 - g * 12;
                    const float4 gr = *reinterpret_cast<const float4*>(s_g + g * SHA_STRIDE + 4 * c4);
                    float p[4] = {pv[u].x, pv[u].y, pv[u].z, pv[u].w}, m[4] = {mv[u].x, mv[u].y, mv[u].z, mv[u].w};
                    float v[4] = {vv[u].x, vv[u].y, vv[u].z, vv[u].w};
                    const float gq[4] = {gr.x, gr.y, gr.z, gr.w};
#pragma unroll
                    for (int k = 0; k < 4; k++) upd(4 * c4 + k, gq[k], p[k], m[k], v[k]);
                    const f4 po = {p[0], p[1], p[2], p[3]}, mo = {m[0], m[1], m[2], m[3]}, vo = {v[0], v[1], v[2], v[3]};
                    p4[e4] = po;
                    __builtin_nontemporal_store(mo, &m4[e4]);
                    __builtin_nontemporal_store(vo, &v4[e4]);
                }
            }
        }
    } else if (n_sh == 48 && ((((uintptr_t)sh | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) == 0)) {
        typedef float f4 __attribute__((ext_vector_type(4)));
        f4* p4 = reinterpret_cast<f4*>(sh + base);
        f4* m4 = reinterpret_cast<f4*>(exp_avg + base);
        f4* v4 = reinterpret_cast<f4*>(exp_avg_sq + base);
        const int n4 = live * 12;
        // four steps at a time: their twelve loads go out together (one at a time -- loads under the lane predicate, every
        // step waiting for its own -- a wave made twelve serial round trips; addresses are clamped instead)
        constexpr int NB = DIR ? 2 : 4;  // (DIR holds the parameters in registers already: smaller batches keep it at 3 waves per SIMD)
#pragma unroll
        for (int st0 = 0; st0 < 12; st0 += NB) {
            f4 pv[NB], mv[NB], vv[NB];
#pragma unroll
            for (int u = 0; u < NB; u++) {
                const int e4 = min((st0 + u) * 64 + lane, n4 - 1);  // float4 index inside the wave's 64 x 48 block
                // the moments are touched once per step: stream them past the caches, the parameters are read again by
                // the next forward and should stay in the last-level cache
                if (DIR) { const float4 k = pkeep[st0 + u]; pv[u] = (f4){k.x, k.y, k.z, k.w}; }
                else pv[u] = p4[e4];
                mv[u] = __builtin_nontemporal_load(&m4[e4]); vv[u] = __builtin_nontemporal_load(&v4[e4]);
            }
#pragma unroll
            for (int u = 0; u < NB; u++) {
                const int e4 = (st0 + u) * 64 + lane;
                if (e4 < n4) {
                    const int g = e4 / 12, c4 = e4 - g * 12;
                    const float4 gr = *reinterpret_cast<const float4*>(s_g + g * SHA_STRIDE + 4 * c4);
                    float p[4] = {pv[u].x, pv[u].y, pv[u].z, pv[u].w}, m[4] = {mv[u].x, mv[u].y, mv[u].z, mv[u].w};
                    float v[4] = {vv[u].x, vv[u].y, vv[u].z, vv[u].w};
                    const float gq[4] = {gr.x, gr.y, gr.z, gr.w};
#pragma unroll
                    for (int k = 0; k < 4; k++) upd(4 * c4 + k, gq[k], p[k], m[k], v[k]);
                    const f4 po = {p[0], p[1], p[2], p[3]}, mo = {m[0], m[1], m[2], m[3]}, vo = {v[0], v[1], v[2], v[3]};
                    p4[e4] = po;
                    __builtin_nontemporal_store(mo, &m4[e4]);
                    __builtin_nontemporal_store(vo, &v4[e4]);
                }
            }
        }
    } else {
        const int n = live * n_sh;
        for (int e = lane; e < n; e += 64) {
            const int g = e / n_sh, c = e - g * n_sh;
            float p = sh[base + e], m = exp_avg[base + e], v = exp_avg_sq[base + e];
            upd(c, s_g[g * SHA_STRIDE + c], p, m, v);
            sh[base + e] = p; exp_avg[base + e] = m; exp_avg_sq[base + e] = v;
        }
    }
    if (MASKED && idx < P) a.reach[idx] = 0;
}

// the zero-gradient half as a launch of its own, one wave per 64 Gaussians: for a step with no blend backward to ride in
__global__ void __launch_bounds__(64) k_sh_adam_zero(SgrShAdamJob job) { sgr_sh_adam_zero_wave<4>(job, (int)blockIdx.x * 64); }
// ... and the persistent form the blend backward carries, as a launch of its own: job.n_adam waves, each over every n_adam-th block
__global__ void __launch_bounds__(64) k_sh_adam_zero_persistent(SgrShAdamJob job) { sgr_sh_adam_zero_persistent(job, (int)blockIdx.x, job.n_adam); }

}  // namespace

void sgr_launch_sh_adam_from_views(int P, int V, int D, int M, size_t vstride, const float* means3D, const float* campos,
                                   const float* dcolor, float* sh, float* exp_avg, float* exp_avg_sq, const SgrShAdamHyper& h,
                                   float* dmean_extra, uint8_t* reach, hipStream_t s)
{
    ShAdamArgs a = {h.lr_dc, h.lr_rest, h.beta1, h.beta2, h.omb1, h.omb2, h.eps, h.bc1, h.bc2_sqrt, h.grad_scale, h.guard, h.guard_cap, reach};
    if (reach)  // (the callers have checked: M == 16, aligned buffers, no dmean_extra)
        hipLaunchKernelGGL((k_sh_adam_from_views<false, true>), dim3((P + 63) / 64), dim3(64), 0, s, P, V, D, M, vstride, means3D, campos,
                           dcolor, sh, exp_avg, exp_avg_sq, a, dmean_extra);
    else if (dmean_extra)
        hipLaunchKernelGGL(k_sh_adam_from_views<true>, dim3((P + 63) / 64), dim3(64), 0, s, P, V, D, M, vstride, means3D, campos, dcolor,
                           sh, exp_avg, exp_avg_sq, a, dmean_extra);
    else
        hipLaunchKernelGGL(k_sh_adam_from_views<false>, dim3((P + 63) / 64), dim3(64), 0, s, P, V, D, M, vstride, means3D, campos, dcolor,
                           sh, exp_avg, exp_avg_sq, a, dmean_extra);
}

void sgr_launch_sh_adam_zero(const SgrShAdamJob& job, hipStream_t s)
{
    if (job.P <= 0) return;
    hipLaunchKernelGGL(k_sh_adam_zero, dim3((job.P + 63) / 64), dim3(64), 0, s, job);
}

void sgr_launch_sh_adam_zero_persistent(const SgrShAdamJob& job, hipStream_t s)
{
    if (job.P <= 0 || job.n_adam <= 0) return;
    hipLaunchKernelGGL(k_sh_adam_zero_persistent, dim3(job.n_adam), dim3(64), 0, s, job);
}

void sgr_launch_sh_grad_from_views(int P, int V, int D, int M, size_t vstride, const float* means3D, const float* campos,
                                   const float* dcolor, float* dL_dsh, hipStream_t s)
{
    hipLaunchKernelGGL(k_sh_grad_from_views, dim3((P + 255) / 256), dim3(256), 0, s, P, V, D, M, vstride, means3D, campos, dcolor,
                       dL_dsh);
}

// ---- the C entry points --------------------------------------------------------------------------------------------------
// what an entry point returns after its launch: 0, or SGR_E_HIP with the runtime's message behind `what`
static int sh_launch_status(const char* what)
{
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : sgr_fail(SGR_E_HIP, (std::string(what) + ": " + hipGetErrorString(e)).c_str());
}

// the two halves of SH-Adam split by reach flag (sh_adam_update.h)
static bool sh_split_ok(int M, const float* sh, const float* m, const float* v)
{
    return M == 16 && ((((uintptr_t)sh | (uintptr_t)m | (uintptr_t)v) & 15) == 0);
}

// (n_adam == 0: one wave per 64 Gaussians; otherwise that many persistent waves)
static int sh_adam_zero_grad(int P, int M, float* sh_params, float* exp_avg, float* exp_avg_sq, const uint8_t* reach, float lr_dc,
                             float lr_rest, float beta1, float beta2, float eps, int step, float grad_scale, const uint32_t* guard_header,
                             uint32_t guard_capacity, int n_adam, void* stream)
{
    if (P <= 0) return 0;
    if (step < 1 || !sh_params || !exp_avg || !exp_avg_sq || !reach) return sgr_fail(SGR_E_INVALID, "sgr_sh_adam_zero_grad: bad argument");
    if (!sh_split_ok(M, sh_params, exp_avg, exp_avg_sq))
        return sgr_fail(SGR_E_INVALID, "sgr_sh_adam_zero_grad: needs M == 16 and 16-byte aligned buffers");
    const SgrShAdamHyper h = sgr_sh_adam_hyper(lr_dc, lr_rest, beta1, beta2, eps, step, grad_scale, guard_header, guard_capacity);
    const SgrShAdamJob job = sgr_sh_adam_job(h, P, n_adam, sh_params, exp_avg, exp_avg_sq, reach);
    if (n_adam > 0) sgr_launch_sh_adam_zero_persistent(job, (hipStream_t)stream);
    else sgr_launch_sh_adam_zero(job, (hipStream_t)stream);
    return sh_launch_status("sh_adam_zero_grad");
}

extern "C" {

int sgr_sh_grad_from_views(int P, int n_views, int D, int M, const float* means3D, const float* campos_all,
                           const float* dcolor_all, int64_t view_stride, float* dL_dsh, void* stream)
{
    if (P <= 0) return 0;
    if (n_views <= 0 || D < 0 || D > 3 || M < (D + 1) * (D + 1) || M > 16 || !means3D || !campos_all || !dcolor_all || !dL_dsh)
        return sgr_fail(SGR_E_INVALID, "sgr_sh_grad_from_views: bad arguments");
    if (view_stride != 0 && view_stride < P) return sgr_fail(SGR_E_INVALID, "sgr_sh_grad_from_views: view_stride < P");
    sgr_launch_sh_grad_from_views(P, n_views, D, M, (size_t)(view_stride ? view_stride : P), means3D, campos_all, dcolor_all, dL_dsh,
                                  (hipStream_t)stream);
    return sh_launch_status("sh_grad_from_views");
}

int sgr_sh_adam_from_views_ex(int P, int n_views, int D, int M, const float* means3D, const float* campos_all,
                              const float* dcolor_all, int64_t view_stride, float* sh_params, float* exp_avg, float* exp_avg_sq, float lr_dc,
                              float lr_rest, float beta1, float beta2, float eps, int step, float grad_scale, float* dmean_extra,
                              void* stream)
{
    if (P <= 0) return 0;
    if (n_views <= 0 || D < 0 || D > 3 || M < (D + 1) * (D + 1) || M > 16 || step < 1 || !means3D || !campos_all || !dcolor_all ||
        !sh_params || !exp_avg || !exp_avg_sq)
        return sgr_fail(SGR_E_INVALID, "sgr_sh_adam_from_views: bad argument");
    if (view_stride != 0 && view_stride < P) return sgr_fail(SGR_E_INVALID, "sgr_sh_adam_from_views: view_stride < P");
    if (dmean_extra && (M != 16 || ((uintptr_t)sh_params & 15)))
        return sgr_fail(SGR_E_INVALID, "sgr_sh_adam_from_views_ex: dmean_extra needs M == 16 and 16-byte aligned sh_params");
    sgr_launch_sh_adam_from_views(P, n_views, D, M, (size_t)(view_stride ? view_stride : P), means3D, campos_all, dcolor_all, sh_params,
                                  exp_avg, exp_avg_sq, sgr_sh_adam_hyper(lr_dc, lr_rest, beta1, beta2, eps, step, grad_scale), dmean_extra,
                                  nullptr, (hipStream_t)stream);
    return sh_launch_status("sh_adam_from_views");
}

int sgr_sh_adam_zero_grad(int P, int M, float* sh_params, float* exp_avg, float* exp_avg_sq, const uint8_t* reach, float lr_dc,
                          float lr_rest, float beta1, float beta2, float eps, int step, float grad_scale, const uint32_t* guard_header,
                          uint32_t guard_capacity, void* stream)
{
    return sh_adam_zero_grad(P, M, sh_params, exp_avg, exp_avg_sq, reach, lr_dc, lr_rest, beta1, beta2, eps, step, grad_scale, guard_header,
                             guard_capacity, 0, stream);
}

int sgr_sh_adam_zero_grad_persistent(int P, int M, float* sh_params, float* exp_avg, float* exp_avg_sq, const uint8_t* reach, float lr_dc,
                                     float lr_rest, float beta1, float beta2, float eps, int step, float grad_scale,
                                     const uint32_t* guard_header, uint32_t guard_capacity, int n_adam, void* stream)
{
    if (n_adam < 8 || (n_adam & 7) || n_adam > 65536)
        return sgr_fail(SGR_E_INVALID, "sgr_sh_adam_zero_grad_persistent: n_adam must be a multiple of 8 in [8, 65536]");
    return sh_adam_zero_grad(P, M, sh_params, exp_avg, exp_avg_sq, reach, lr_dc, lr_rest, beta1, beta2, eps, step, grad_scale, guard_header,
                             guard_capacity, n_adam, stream);
}

int sgr_sh_adam_from_views_masked(int P, int n_views, int D, int M, const float* means3D, const float* campos_all,
                                  const float* dcolor_all, int64_t view_stride, float* sh_params, float* exp_avg, float* exp_avg_sq,
                                  float lr_dc, float lr_rest, float beta1, float beta2, float eps, int step, float grad_scale,
                                  uint8_t* reach, const uint32_t* guard_header, uint32_t guard_capacity, void* stream)
{
    if (P <= 0) return 0;
    if (n_views <= 0 || D < 0 || D > 3 || M < (D + 1) * (D + 1) || step < 1 || !means3D || !campos_all || !dcolor_all || !sh_params ||
        !exp_avg || !exp_avg_sq || !reach)
        return sgr_fail(SGR_E_INVALID, "sgr_sh_adam_from_views_masked: bad argument");
    if (view_stride != 0 && view_stride < P) return sgr_fail(SGR_E_INVALID, "sgr_sh_adam_from_views_masked: view_stride < P");
    if (!sh_split_ok(M, sh_params, exp_avg, exp_avg_sq))
        return sgr_fail(SGR_E_INVALID, "sgr_sh_adam_from_views_masked: needs M == 16 and 16-byte aligned buffers");
    sgr_launch_sh_adam_from_views(P, n_views, D, M, (size_t)(view_stride ? view_stride : P), means3D, campos_all, dcolor_all, sh_params,
                                  exp_avg, exp_avg_sq,
                                  sgr_sh_adam_hyper(lr_dc, lr_rest, beta1, beta2, eps, step, grad_scale, guard_header, guard_capacity), nullptr,
                                  reach, (hipStream_t)stream);
    return sh_launch_status("sh_adam_from_views_masked");
}

int sgr_sh_adam_from_views(int P, int n_views, int D, int M, const float* means3D, const float* campos_all,
                           const float* dcolor_all, int64_t view_stride, float* sh_params, float* exp_avg, float* exp_avg_sq, float lr_dc,
                           float lr_rest, float beta1, float beta2, float eps, int step, float grad_scale, void* stream)
{
    return sgr_sh_adam_from_views_ex(P, n_views, D, M, means3D, campos_all, dcolor_all, view_stride, sh_params, exp_avg, exp_avg_sq, lr_dc,
                                     lr_rest, beta1, beta2, eps, step, grad_scale, nullptr, stream);
}

}  // extern "C"
