// sh_adam_update.h -- Adam on the SH block, split by reach flag (device code shared by sh_adam.hip and blend.hip).
//
// The forward blend sets one byte per Gaussian that gets a survivor bit in any block (blend.hip).  The blend backward walks exactly
// those bits, so a Gaussian whose flag is 0 receives no atomic: its nine accumulator sums stay zero, the backward preprocess takes
// its zero-row exit, its colour gradient is +0 and its 48-float SH gradient is +0 in every view.  Its Adam step therefore depends
// on nothing the backward computes (flag superset of reached => zero row), and runs as soon as the forward is done:
//   sgr_sh_adam_zero_persistent  flag == 0 rows, gradient zero -- persistent waves in front of the blend backward's workgroups
//                                (sgr_sh_adam_zero_wave: one wave per 64 Gaussians, the launch of its own where there is no blend);
//   k_sh_adam_from_views         masked mode: flag != 0 rows from the colour gradients, then the wave's 64 flags back to 0.
// Together they leave the bits of one dense k_sh_adam_from_views launch.
#pragma once
#include "sgr_common.h"

// The update of one SH coefficient.  Every operation is rounded on its own, in the order k_sh_adam_from_views has always had
// (sh_adam.hip is built without contraction: v_mul, v_mul, v_add per moment, IEEE sqrt and divides); the pragma keeps it so in a
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

// The same update with the quotient lr / bc1 formed by the caller.  Both operands are wave-uniform and lr is one of two values, so a
// caller forms the two correctly rounded quotients once and selects per coefficient: the operation sh_adam_update does per coefficient
// (11 of its 62 VALU instructions), on the same inputs, with the same result.
__device__ __forceinline__ void sh_adam_update_q(float g, float& p, float& m, float& v, float lr_over_bc1, float grad_scale, float b1,
                                                 float b2, float omb1, float omb2, float eps, float bc2_sqrt)
{
#pragma clang fp contract(off)
    g *= grad_scale;
    m = b1 * m + omb1 * g;
    v = b2 * v + omb2 * g * g;
    const float denom = sqrtf(v) / bc2_sqrt + eps;
    p -= lr_over_bc1 * (m / denom);
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

// The same rows, by n_w persistent waves: wave w takes the 64-Gaussian blocks w, w + n_w, w + 2 n_w, ... -- a static split, no wave
// waits for or signals another -- and keeps loads in flight while it computes.  A block is six rounds of two float4 steps; the loads of
// the next round (of the next block with work, behind a block's last round) go out before the arithmetic and the stores of the current
// one, into the other of two register buffers, and the flag bytes of the block after next are requested two blocks ahead.  Per row the
// arithmetic, its inputs and the redirect of a flagged row's loads are those of sgr_sh_adam_zero_wave.
struct SgrShAdamBlock { int g0, n4, gfree; unsigned long long todo; };  // wave-uniform: first row, float4s, first unflagged row, rows to update
typedef float sgr_f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void sgr_sh_adam_zero_issue(const SgrShAdamJob& a, const SgrShAdamBlock& b, int round, int lane, sgr_f4 (&pv)[2],
                                                       sgr_f4 (&mv)[2], sgr_f4 (&vv)[2])
{
    const size_t base = (size_t)b.g0 * 48;
    const sgr_f4* p4 = reinterpret_cast<const sgr_f4*>(a.sh + base);
    const sgr_f4* m4 = reinterpret_cast<const sgr_f4*>(a.exp_avg + base);
    const sgr_f4* v4 = reinterpret_cast<const sgr_f4*>(a.exp_avg_sq + base);
#pragma unroll
    for (int u = 0; u < 2; u++) {
        const int k0 = (2 * round + u) * 64;               // (float4 k0 + lane of the block, clamped: min against a scalar, so that no
        const int ec = min(lane, b.n4 - 1 - k0) + k0;      // per-step lane constant stays live across the loop)
        const int g = ec / 12;
        const int ea = ((b.todo >> g) & 1ull) ? ec : b.gfree * 12 + (ec - g * 12);
        pv[u] = p4[ea];
        mv[u] = __builtin_nontemporal_load(&m4[ea]); vv[u] = __builtin_nontemporal_load(&v4[ea]);
    }
}

__device__ __forceinline__ void sgr_sh_adam_zero_consume(const SgrShAdamJob& a, const SgrShAdamBlock& b, int round, int lane,
                                                         const sgr_f4 (&pv)[2], const sgr_f4 (&mv)[2], const sgr_f4 (&vv)[2], float q_dc,
                                                         float q_rest)
{
    const size_t base = (size_t)b.g0 * 48;
    sgr_f4* p4 = reinterpret_cast<sgr_f4*>(a.sh + base);
    sgr_f4* m4 = reinterpret_cast<sgr_f4*>(a.exp_avg + base);
    sgr_f4* v4 = reinterpret_cast<sgr_f4*>(a.exp_avg_sq + base);
#pragma unroll
    for (int u = 0; u < 2; u++) {
        const int k0 = (2 * round + u) * 64, e4 = k0 + lane;
        const int ec = min(lane, b.n4 - 1 - k0) + k0;
        const int g = ec / 12, col = ec - g * 12;
        if (((b.todo >> g) & 1ull) && lane < b.n4 - k0) {
            float p[4] = {pv[u].x, pv[u].y, pv[u].z, pv[u].w}, m[4] = {mv[u].x, mv[u].y, mv[u].z, mv[u].w};
            float v[4] = {vv[u].x, vv[u].y, vv[u].z, vv[u].w};
#pragma unroll
            for (int k = 0; k < 4; k++)
                sh_adam_update_q(a.zero, p[k], m[k], v[k], 4 * col + k < 3 ? q_dc : q_rest, a.grad_scale, a.b1, a.b2, a.omb1, a.omb2, a.eps,
                                 a.bc2_sqrt);
            const sgr_f4 po = {p[0], p[1], p[2], p[3]}, mo = {m[0], m[1], m[2], m[3]}, vo = {v[0], v[1], v[2], v[3]};
            p4[e4] = po;
            __builtin_nontemporal_store(mo, &m4[e4]);
            __builtin_nontemporal_store(vo, &v4[e4]);
        }
    }
}

__device__ __forceinline__ void sgr_sh_adam_zero_persistent(const SgrShAdamJob& a, int w, int n_w)
{
    if (a.guard && SGR_FORWARD_INVALID(a.guard, a.guard_cap)) return;  // the host repeats that step
    const int lane = threadIdx.x & 63;
    const int nblk = (a.P + 63) >> 6;
    if (w >= nblk) return;
    const int nb = (nblk - w + n_w - 1) / n_w;  // this wave's blocks: ordinal i is block w + i * n_w
    // the flag bytes of ordinal i (behind the last one: flagged, which is "no work")
    auto flags = [&](int i) -> uint32_t {
        if (i >= nb) return 1u;
        const int g0 = (w + i * n_w) * 64;
        return a.reach[g0 + min(lane, min(64, a.P - g0) - 1)];
    };
    int i = -1;
    uint32_t f1 = flags(0), f2 = flags(1);
    SgrShAdamBlock cur;
    // on to this wave's next block with an unflagged row (a block whose 64 rows are all flagged costs its flag read only)
    auto advance = [&]() -> bool {
        for (;;) {
            if (++i >= nb) return false;
            const int g0 = (w + i * n_w) * 64, live = min(64, a.P - g0);
            const unsigned long long rows = live == 64 ? ~0ull : ((1ull << live) - 1ull);
            const unsigned long long todo = __ballot(f1 == 0u) & rows;
            f1 = f2; f2 = flags(i + 2);
            if (todo != 0ull) {
                cur.g0 = g0; cur.n4 = live * 12; cur.gfree = (int)__builtin_ctzll(todo); cur.todo = todo;
                return true;
            }
        }
    };
    if (!advance()) return;
    // (sh_adam_update_q; kept in scalar registers -- as vector registers the two cost the blend kernels their fifth wave per SIMD)
    const float q_dc = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, a.lr_dc / a.bc1)));
    const float q_rest = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, a.lr_rest / a.bc1)));
    sgr_f4 pa[2], ma[2], va[2], pb[2], mb[2], vb[2];
    sgr_sh_adam_zero_issue(a, cur, 0, lane, pa, ma, va);
    for (;;) {
        sgr_sh_adam_zero_issue(a, cur, 1, lane, pb, mb, vb); sgr_sh_adam_zero_consume(a, cur, 0, lane, pa, ma, va, q_dc, q_rest);
        sgr_sh_adam_zero_issue(a, cur, 2, lane, pa, ma, va); sgr_sh_adam_zero_consume(a, cur, 1, lane, pb, mb, vb, q_dc, q_rest);
        sgr_sh_adam_zero_issue(a, cur, 3, lane, pb, mb, vb); sgr_sh_adam_zero_consume(a, cur, 2, lane, pa, ma, va, q_dc, q_rest);
        sgr_sh_adam_zero_issue(a, cur, 4, lane, pa, ma, va); sgr_sh_adam_zero_consume(a, cur, 3, lane, pb, mb, vb, q_dc, q_rest);
        sgr_sh_adam_zero_issue(a, cur, 5, lane, pb, mb, vb); sgr_sh_adam_zero_consume(a, cur, 4, lane, pa, ma, va, q_dc, q_rest);
        const SgrShAdamBlock last = cur;
        const bool more = advance();
        if (more) sgr_sh_adam_zero_issue(a, cur, 0, lane, pa, ma, va);
        sgr_sh_adam_zero_consume(a, last, 5, lane, pb, mb, vb, q_dc, q_rest);
        if (!more) return;
    }
}
