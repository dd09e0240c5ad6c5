// sh_adam_update.h -- Adam on the SH block, split by reach flag (device code shared by preprocess.hip and blend.hip).
//
// The forward blend sets one byte per Gaussian that gets a survivor bit in any block (blend.hip).  The blend backward walks exactly
// those bits, so a Gaussian whose flag is 0 receives no atomic: its nine accumulator sums stay zero, the backward preprocess takes
// its zero-row exit, its colour gradient is +0 and its 48-float SH gradient is +0 in every view.  Its Adam step therefore depends
// on nothing the backward computes (flag superset of reached => zero row), and runs as soon as the forward is done:
//   sgr_sh_adam_zero_wave   flag == 0 rows, gradient zero -- as extra workgroups of the blend backward, or a launch of its own;
//   k_sh_adam_from_views    masked mode: flag != 0 rows from the colour gradients, then the wave's 64 flags back to 0.
// Together they leave the bits of one dense k_sh_adam_from_views launch.
#pragma once
#include "sgr_common.h"

// The update of one SH coefficient.  Every operation is rounded on its own, in the order k_sh_adam_from_views has always had
// (preprocess.hip is built without contraction: v_mul, v_mul, v_add per moment, IEEE sqrt and divides); the pragma keeps it so in a
// translation unit that contracts.
__device__ __forceinline__ void sh_adam_update(float g, float& p, float& m, float& v, float lr, float grad_scale, float b1, float b2,
                                               float omb1, float omb2, float eps, float bc1, float bc2_sqrt)
{
#pragma clang fp contract(off)
    g *= grad_scale;
    m = b1 * m + omb1 * g;
    v = b2 * v + omb2 * g * g;
    const float denom = sqrtf(v) / bc2_sqrt + eps;
    p -= (lr / bc1) * (m / denom);
}

// One wave, 64 Gaussians from g0 on: the 64 x 48 floats of parameters and moments as one contiguous stream, one float4 per lane and
// step (phase 2 of k_sh_adam_from_views), rows with a flag left alone.  A flagged row's loads are redirected to the same column of
// the wave's first unflagged row -- an address the wave reads anyway -- instead of being predicated (see k_sh_adam_from_views).
// NB: float4 steps whose loads go out together.
template <int NB>
__device__ __forceinline__ void sgr_sh_adam_zero_wave(const SgrShAdamJob& a, int g0)
{
    typedef float f4 __attribute__((ext_vector_type(4)));
    if (a.guard && SGR_FORWARD_INVALID(a.guard, a.guard_cap)) return;  // the host repeats that step
    const int lane = threadIdx.x & 63;
    const int live = min(64, a.P - g0);
    if (live <= 0) return;
    const unsigned long long rows = live == 64 ? ~0ull : ((1ull << live) - 1ull);
    const unsigned long long todo = __ballot(a.reach[g0 + min(lane, live - 1)] == 0) & rows;  // bit g: row g0 + g is updated here
    if (todo == 0ull) return;
    const int gfree = (int)__builtin_ctzll(todo);
    const size_t base = (size_t)g0 * 48;
    f4* p4 = reinterpret_cast<f4*>(a.sh + base);
    f4* m4 = reinterpret_cast<f4*>(a.exp_avg + base);
    f4* v4 = reinterpret_cast<f4*>(a.exp_avg_sq + base);
    const int n4 = live * 12;
#pragma unroll
    for (int st0 = 0; st0 < 12; st0 += NB) {
        f4 pv[NB], mv[NB], vv[NB];
        int col[NB];
        bool mine[NB];
#pragma unroll
        for (int u = 0; u < NB; u++) {
            const int e4 = (st0 + u) * 64 + lane;
            const int ec = min(e4, n4 - 1);
            const int g = ec / 12;
            col[u] = ec - g * 12;
            const bool upd = (todo >> g) & 1ull;
            mine[u] = upd && e4 < n4;
            const int ea = upd ? ec : gfree * 12 + col[u];
            pv[u] = p4[ea];
            mv[u] = __builtin_nontemporal_load(&m4[ea]); vv[u] = __builtin_nontemporal_load(&v4[ea]);
        }
#pragma unroll
        for (int u = 0; u < NB; u++) {
            if (mine[u]) {
                const int e4 = (st0 + u) * 64 + lane;
                float p[4] = {pv[u].x, pv[u].y, pv[u].z, pv[u].w}, m[4] = {mv[u].x, mv[u].y, mv[u].z, mv[u].w};
                float v[4] = {vv[u].x, vv[u].y, vv[u].z, vv[u].w};
#pragma unroll
                for (int k = 0; k < 4; k++)
                    sh_adam_update(a.zero, p[k], m[k], v[k], 4 * col[u] + k < 3 ? a.lr_dc : a.lr_rest, a.grad_scale, a.b1, a.b2, a.omb1,
                                   a.omb2, a.eps, a.bc1, a.bc2_sqrt);
                const f4 po = {p[0], p[1], p[2], p[3]}, mo = {m[0], m[1], m[2], m[3]}, vo = {v[0], v[1], v[2], v[3]};
                p4[e4] = po;
                __builtin_nontemporal_store(mo, &m4[e4]);
                __builtin_nontemporal_store(vo, &v4[e4]);
            }
        }
    }
}
