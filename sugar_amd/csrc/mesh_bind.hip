// mesh_bind.hip -- the refine stage's mesh binding and its normal-consistency regulariser.
//
//   * SuGaR.points / .scaling / .quaternions of a model bound to a surface mesh (sugar_scene/sugar_model.py:383-479, the
//     `not editable` branch): Gaussian g = f * n + k sits on face f at barycentric coordinates bary[k]; it is flat (thickness along
//     the face normal, exp(_scales) in the plane) and its rotation is the face frame turned in the plane by a learned complex number.
//   * pytorch3d.loss.mesh_normal_consistency as the stand-in of sugar_amd/shims/pytorch3d/loss defines it, over a pair list that is
//     built once per topology (sugar_amd/mesh_bind.py): 1 - cos(n0, n1) averaged over the pairs of faces that share an edge.
//
// The reference spreads each of these over dozens of small tensor operations per iteration and walks them back with autograd.  Here:
//   k_bind_forward      one lane per Gaussian: vertex gather, barycentric sum, exp, face frame, matrix_to_quaternion, normalise.
//   k_bind_backward     one lane per face: the n Gaussians of the face in order; writes dL/d_scales, dL/d_quaternions and the nine
//                       floats dL/d(corner c of face f) to contrib[3f + c].
//   k_nc_forward/_sum   one lane per pair (grid-stride, fixed grid), per-block partial sums in double, one block adds the partials.
//   k_nc_backward       one lane per pair: twelve floats dL/d(slot s of pair p) to contrib[4p + s].
//   k_gather_vertex     one lane per vertex adds its contributions in the order of a CSR list (ascending item index).  No float atomics
//                       anywhere: the vertex gradient is the same bits on every run.
//
// Compiled with -ffp-contract=off: the forward restates the reference's individually rounded tensor arithmetic in its order (sums over a
// dimension of 3 run in index order; torch's norm() may order its three squares differently, which stays inside the rounding of one
// f32 evaluation).  Indices are validated in the kernels: a vertex index outside [0, V) gives NaN outputs for that element and no
// out-of-bounds access; a CSR item outside its range is skipped.
#include "../../include/sugar_raster.h"
#include "sgr_common.h"

#include <cmath>

namespace {

#define MB_EPS_NORMALIZE 1e-12f   // torch.nn.functional.normalize
#define MB_EPS_FACE_NORMAL 1e-6f  // the stand-in Meshes.faces_normals_list: n / max(|n|, 1e-6)
#define MB_QUAT_FLOOR 0.1f        // matrix_to_quaternion: 2 * max(q_abs, 0.1)
#define MB_EPS_COSINE 1e-8f       // torch.cosine_similarity
#define NC_BLOCKS 1024            // fixed shape of the two-stage reduction
#define NC_THREADS 256

struct V3 {
    float x, y, z;
};

__device__ __forceinline__ V3 v3(float x, float y, float z) { return V3{x, y, z}; }
__device__ __forceinline__ V3 ld3(const float* p) { return V3{p[0], p[1], p[2]}; }
__device__ __forceinline__ void st3(float* p, V3 a) { p[0] = a.x; p[1] = a.y; p[2] = a.z; }
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return V3{a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 operator-(V3 a) { return V3{-a.x, -a.y, -a.z}; }
__device__ __forceinline__ V3 operator*(float s, V3 a) { return V3{s * a.x, s * a.y, s * a.z}; }
__device__ __forceinline__ V3 operator/(V3 a, float s) { return V3{a.x / s, a.y / s, a.z / s}; }
__device__ __forceinline__ float dot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ float norm(V3 a) { return sqrtf(dot(a, a)); }
// torch.cross / torch.linalg.cross
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }

// y = x / max(|x|, eps) (F.normalize, and the stand-in's face normal with eps = 1e-6); `len` is |x|
__device__ __forceinline__ V3 normalize(V3 x, float eps, float& len)
{
    len = norm(x);
    return x / fmaxf(len, eps);
}

// the backward of y = x / max(|x|, eps) as autograd composes it: through the division and, where the clamp is inactive (|x| >= eps),
// through the norm; where it is active the divisor is a constant.
__device__ __forceinline__ V3 normalize_bwd(V3 y, float len, float eps, V3 dy)
{
    if (len >= eps) return (dy - dot(y, dy) * y) / len;
    return dy / eps;
}

// the backward of x / max(|x|, eps) inside torch.cosine_similarity: there the clamp is applied in place outside the graph, so the
// divisor D = max(|x|, eps) keeps the derivative of |x| even where the clamp is active (and none at x = 0)
__device__ __forceinline__ V3 cosine_normalize_bwd(V3 y, float len, float eps, V3 dy)
{
    const float D = fmaxf(len, eps);
    const float r = len >= eps ? 1.0f : (len > 0.f ? D / len : 0.f);
    return (dy - (r * dot(y, dy)) * y) / D;
}

struct FaceFrame {
    V3 e1, e2, m, a, R0, b, B1, c, B2;
    float Lm, La, Lb, Lc;
};

__device__ __forceinline__ void face_frame(V3 p0, V3 p1, V3 p2, FaceFrame& f)
{
    f.e1 = p1 - p0;
    f.e2 = p2 - p0;
    f.m = cross(f.e1, f.e2);
    f.a = normalize(f.m, MB_EPS_FACE_NORMAL, f.Lm);   // Meshes.faces_normals_list
    f.R0 = normalize(f.a, MB_EPS_NORMALIZE, f.La);    // :451
    f.b = p0 - p1;
    f.B1 = normalize(f.b, MB_EPS_NORMALIZE, f.Lb);    // :455
    f.c = cross(f.R0, f.B1);
    f.B2 = normalize(f.c, MB_EPS_NORMALIZE, f.Lc);    // :458
}

// matrix_to_quaternion of R = [R0 | R1 | R2] (columns), sugar_amd/shims/pytorch3d/transforms: q_abs = sqrt of the positive part of the four
// traces, the first arg-max picks the row of candidates, divided by 2 max(q_abs, 0.1).  Rows, with A = (m21-m12, m02-m20, m10-m01) and
// S = (m12+m21, m02+m20, m10+m01):  0: (q0^2, Ax, Ay, Az)  1: (Ax, q1^2, Sz, Sy)  2: (Ay, Sz, q2^2, Sx)  3: (Az, Sy, Sx, q3^2).
struct QuatPick {
    int best;
    float qa, t, s;    // q_abs[best], its trace term, the divisor 2 max(qa, 0.1)
    float row[4];      // the chosen candidate before the division
    float q[4];        // after it
};

__device__ __forceinline__ void matrix_to_quaternion(V3 R0, V3 R1, V3 R2, QuatPick& o)
{
    const float m00 = R0.x, m10 = R0.y, m20 = R0.z, m01 = R1.x, m11 = R1.y, m21 = R1.z, m02 = R2.x, m12 = R2.y, m22 = R2.z;
    float t[4];
    t[0] = 1.0f + m00 + m11 + m22;
    t[1] = 1.0f + m00 - m11 - m22;
    t[2] = 1.0f - m00 + m11 - m22;
    t[3] = 1.0f - m00 - m11 + m22;
    float qa[4];
    int best = 0;
    float best_qa = 0.f, best_t = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        qa[i] = t[i] > 0.f ? sqrtf(t[i]) : 0.f;
        if (i == 0 || qa[i] > best_qa) { best = i; best_qa = qa[i]; best_t = t[i]; }   // strict '>': the first maximum, as torch.argmax
    }
    const float Ax = m21 - m12, Ay = m02 - m20, Az = m10 - m01;
    const float Sx = m12 + m21, Sy = m02 + m20, Sz = m10 + m01;
    const float d0 = qa[0] * qa[0], d1 = qa[1] * qa[1], d2 = qa[2] * qa[2], d3 = qa[3] * qa[3];
    float r0, r1, r2, r3;
    if (best == 0) { r0 = d0; r1 = Ax; r2 = Ay; r3 = Az; }
    else if (best == 1) { r0 = Ax; r1 = d1; r2 = Sz; r3 = Sy; }
    else if (best == 2) { r0 = Ay; r1 = Sz; r2 = d2; r3 = Sx; }
    else { r0 = Az; r1 = Sy; r2 = Sx; r3 = d3; }
    o.best = best;
    o.qa = best_qa;
    o.t = best_t;
    o.s = 2.0f * fmaxf(o.qa, MB_QUAT_FLOOR);
    o.row[0] = r0; o.row[1] = r1; o.row[2] = r2; o.row[3] = r3;
    o.q[0] = r0 / o.s; o.q[1] = r1 / o.s; o.q[2] = r2 / o.s; o.q[3] = r3 / o.s;
}

__device__ __forceinline__ bool face_ok(int i0, int i1, int i2, int V)
{
    return i0 >= 0 && i0 < V && i1 >= 0 && i1 < V && i2 >= 0 && i2 < V;
}

// One lane per Gaussian g = f * n + k.  A null output pointer skips that output (uniform branch).
__global__ void __launch_bounds__(256) k_bind_forward(int F, int n, int V, const float* __restrict__ verts, const int* __restrict__ faces,
                                                      const float* __restrict__ bary, const float* __restrict__ scales,
                                                      const float* __restrict__ cplx, const float* __restrict__ thickness,
                                                      float* __restrict__ points, float* __restrict__ scaling, float* __restrict__ quats)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (int64_t)F * n) return;
    if (scaling) {                                                          // :420, :438-441
        float* o = scaling + 3 * g;
        o[0] = thickness[0] * 1.0f;
        o[1] = expf(scales[2 * g]);
        o[2] = expf(scales[2 * g + 1]);
    }
    if (!points && !quats) return;
    const int f = (int)(g / n), k = (int)(g - (int64_t)f * n);
    const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    if (!face_ok(i0, i1, i2, V)) {                                          // a malformed face: visible, never an out-of-bounds read
        if (points) st3(points + 3 * g, v3(NAN, NAN, NAN));
        if (quats) { float* q = quats + 4 * g; q[0] = q[1] = q[2] = q[3] = NAN; }
        return;
    }
    const V3 p0 = ld3(verts + 3 * (int64_t)i0), p1 = ld3(verts + 3 * (int64_t)i1), p2 = ld3(verts + 3 * (int64_t)i2);
    if (points) {                                                           // :392-398: sum over the three corners, in order
        const float b0 = bary[3 * k], b1 = bary[3 * k + 1], b2 = bary[3 * k + 2];
        st3(points + 3 * g, (b0 * p0 + b1 * p1) + b2 * p2);
    }
    if (quats) {                                                            // :449-479
        FaceFrame ff;
        face_frame(p0, p1, p2, ff);
        float Lz;
        const float zx = cplx[2 * g], zy = cplx[2 * g + 1];
        Lz = sqrtf(zx * zx + zy * zy);
        const float dz = fmaxf(Lz, MB_EPS_NORMALIZE);
        const float c0 = zx / dz, c1 = zy / dz;
        const V3 R1 = c0 * ff.B1 + c1 * ff.B2;
        const V3 R2 = (-c1) * ff.B1 + c0 * ff.B2;
        QuatPick qp;
        matrix_to_quaternion(ff.R0, R1, R2, qp);
        const float Lq = sqrtf(((qp.q[0] * qp.q[0] + qp.q[1] * qp.q[1]) + qp.q[2] * qp.q[2]) + qp.q[3] * qp.q[3]);
        const float dq = fmaxf(Lq, MB_EPS_NORMALIZE);
        float* q = quats + 4 * g;
        q[0] = qp.q[0] / dq; q[1] = qp.q[1] / dq; q[2] = qp.q[2] / dq; q[3] = qp.q[3] / dq;
    }
}

// One lane per face.  contrib[3f + c] (three floats) = dL/d(corner c of face f) from the requested cotangents; d_scales / d_cplx rows of the
// face's n Gaussians.  Null cotangent pointers are skipped (uniform branches).
__global__ void __launch_bounds__(256) k_bind_backward(int F, int n, int V, const float* __restrict__ verts, const int* __restrict__ faces,
                                                       const float* __restrict__ bary, const float* __restrict__ scales,
                                                       const float* __restrict__ cplx, const float* __restrict__ g_points,
                                                       const float* __restrict__ g_scaling, const float* __restrict__ g_quats,
                                                       float* __restrict__ contrib, float* __restrict__ d_scales, float* __restrict__ d_cplx)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    const int64_t g0 = (int64_t)f * n;
    if (g_scaling) {                                                        // d exp(s) = exp(s); the thickness column has no parameter
        for (int k = 0; k < n; ++k) {
            const int64_t g = g0 + k;
            d_scales[2 * g] = g_scaling[3 * g + 1] * expf(scales[2 * g]);
            d_scales[2 * g + 1] = g_scaling[3 * g + 2] * expf(scales[2 * g + 1]);
        }
    }
    if (!g_points && !g_quats) return;
    V3 d0 = v3(0, 0, 0), d1 = v3(0, 0, 0), d2 = v3(0, 0, 0);
    const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    const bool ok = face_ok(i0, i1, i2, V);
    if (ok && g_points) {
        for (int k = 0; k < n; ++k) {
            const V3 gp = ld3(g_points + 3 * (g0 + k));
            d0 = d0 + bary[3 * k] * gp;
            d1 = d1 + bary[3 * k + 1] * gp;
            d2 = d2 + bary[3 * k + 2] * gp;
        }
    }
    if (g_quats && !ok) {
        for (int k = 0; k < n; ++k) d_cplx[2 * (g0 + k)] = d_cplx[2 * (g0 + k) + 1] = NAN;
    }
    if (ok && g_quats) {
        const V3 p0 = ld3(verts + 3 * (int64_t)i0), p1 = ld3(verts + 3 * (int64_t)i1), p2 = ld3(verts + 3 * (int64_t)i2);
        FaceFrame ff;
        face_frame(p0, p1, p2, ff);
        V3 dR0 = v3(0, 0, 0), dB1 = v3(0, 0, 0), dB2 = v3(0, 0, 0);
        for (int k = 0; k < n; ++k) {
            const int64_t g = g0 + k;
            const float zx = cplx[2 * g], zy = cplx[2 * g + 1];
            const float Lz = sqrtf(zx * zx + zy * zy);
            const float dzn = fmaxf(Lz, MB_EPS_NORMALIZE);
            const float c0 = zx / dzn, c1 = zy / dzn;
            const V3 R1 = c0 * ff.B1 + c1 * ff.B2;
            const V3 R2 = (-c1) * ff.B1 + c0 * ff.B2;
            QuatPick qp;
            matrix_to_quaternion(ff.R0, R1, R2, qp);
            // the last normalise (:479)
            const float Lq = sqrtf(((qp.q[0] * qp.q[0] + qp.q[1] * qp.q[1]) + qp.q[2] * qp.q[2]) + qp.q[3] * qp.q[3]);
            const float dqn = fmaxf(Lq, MB_EPS_NORMALIZE);
            const float go0 = g_quats[4 * g], go1 = g_quats[4 * g + 1], go2 = g_quats[4 * g + 2], go3 = g_quats[4 * g + 3];
            float dq[4];
            if (Lq >= MB_EPS_NORMALIZE) {
                const float y0 = qp.q[0] / dqn, y1 = qp.q[1] / dqn, y2 = qp.q[2] / dqn, y3 = qp.q[3] / dqn;
                const float yd = ((y0 * go0 + y1 * go1) + y2 * go2) + y3 * go3;
                dq[0] = (go0 - yd * y0) / Lq; dq[1] = (go1 - yd * y1) / Lq; dq[2] = (go2 - yd * y2) / Lq; dq[3] = (go3 - yd * y3) / Lq;
            } else {
                dq[0] = go0 / MB_EPS_NORMALIZE; dq[1] = go1 / MB_EPS_NORMALIZE; dq[2] = go2 / MB_EPS_NORMALIZE; dq[3] = go3 / MB_EPS_NORMALIZE;
            }
            // q = row / s, s = 2 max(qa, 0.1)
            float drow[4];
            float ds = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                drow[j] = dq[j] / qp.s;
                ds = ds - dq[j] * qp.row[j] / (qp.s * qp.s);
            }
            float dqa = qp.qa > MB_QUAT_FLOOR ? 2.0f * ds : 0.f;
            // the chosen row back to A, S and the diagonal q_abs^2
            float dAx = 0.f, dAy = 0.f, dAz = 0.f, dSx = 0.f, dSy = 0.f, dSz = 0.f;
            float sg0, sg1, sg2;                                            // signs of (m00, m11, m22) in the chosen trace term
            if (qp.best == 0) { dqa += 2.0f * qp.qa * drow[0]; dAx = drow[1]; dAy = drow[2]; dAz = drow[3]; sg0 = 1.f; sg1 = 1.f; sg2 = 1.f; }
            else if (qp.best == 1) { dAx = drow[0]; dqa += 2.0f * qp.qa * drow[1]; dSz = drow[2]; dSy = drow[3]; sg0 = 1.f; sg1 = -1.f; sg2 = -1.f; }
            else if (qp.best == 2) { dAy = drow[0]; dSz = drow[1]; dqa += 2.0f * qp.qa * drow[2]; dSx = drow[3]; sg0 = -1.f; sg1 = 1.f; sg2 = -1.f; }
            else { dAz = drow[0]; dSy = drow[1]; dSx = drow[2]; dqa += 2.0f * qp.qa * drow[3]; sg0 = -1.f; sg1 = -1.f; sg2 = 1.f; }
            const float dt = qp.t > 0.f ? dqa / (2.0f * qp.qa) : 0.f;      // _sqrt_positive_part: zero subgradient at 0
            // m_rc = R_c[r]:  A = (m21-m12, m02-m20, m10-m01), S = (m12+m21, m02+m20, m10+m01)
            const V3 gR0 = v3(sg0 * dt, dAz + dSz, dSy - dAy);             // (m00, m10, m20)
            const V3 gR1 = v3(dSz - dAz, sg1 * dt, dAx + dSx);             // (m01, m11, m21)
            const V3 gR2 = v3(dAy + dSy, dSx - dAx, sg2 * dt);             // (m02, m12, m22)
            dR0 = dR0 + gR0;
            // R1 = c0 B1 + c1 B2, R2 = -c1 B1 + c0 B2
            const float dc0 = dot(gR1, ff.B1) + dot(gR2, ff.B2);
            const float dc1 = dot(gR1, ff.B2) - dot(gR2, ff.B1);
            dB1 = dB1 + (c0 * gR1 - c1 * gR2);
            dB2 = dB2 + (c1 * gR1 + c0 * gR2);
            float dzx, dzy;
            if (Lz >= MB_EPS_NORMALIZE) {
                const float yd = c0 * dc0 + c1 * dc1;
                dzx = (dc0 - yd * c0) / Lz;
                dzy = (dc1 - yd * c1) / Lz;
            } else {
                dzx = dc0 / MB_EPS_NORMALIZE;
                dzy = dc1 / MB_EPS_NORMALIZE;
            }
            d_cplx[2 * g] = dzx;
            d_cplx[2 * g + 1] = dzy;
        }
        // the face frame back to the three corners
        const V3 dc = normalize_bwd(ff.B2, ff.Lc, MB_EPS_NORMALIZE, dB2);
        dR0 = dR0 + cross(ff.B1, dc);                                       // c = R0 x B1
        dB1 = dB1 + cross(dc, ff.R0);
        const V3 db = normalize_bwd(ff.B1, ff.Lb, MB_EPS_NORMALIZE, dB1);   // b = p0 - p1
        const V3 da = normalize_bwd(ff.R0, ff.La, MB_EPS_NORMALIZE, dR0);
        const V3 dm = normalize_bwd(ff.a, ff.Lm, MB_EPS_FACE_NORMAL, da);
        const V3 de1 = cross(ff.e2, dm), de2 = cross(dm, ff.e1);            // m = e1 x e2
        d0 = d0 + (db - (de1 + de2));
        d1 = d1 + (de1 - db);
        d2 = d2 + de2;
    }
    if (!ok) d0 = d1 = d2 = v3(NAN, NAN, NAN);
    float* o = contrib + 9 * (int64_t)f;
    st3(o, d0);
    st3(o + 3, d1);
    st3(o + 6, d2);
}

// out[v] = sum of contrib[item] (three floats each) over items[offsets[v] .. offsets[v+1]), in list order
__global__ void __launch_bounds__(256) k_gather_vertex(int V, int n_items, const int* __restrict__ offsets, const int* __restrict__ items,
                                                       const float* __restrict__ contrib, float* __restrict__ out)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    int lo = offsets[v], hi = offsets[v + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > n_items ? n_items : hi;
    V3 s = v3(0, 0, 0);
    for (int i = lo; i < hi; ++i) {
        const int it = items[i];
        if (it < 0 || it >= n_items) continue;
        s = s + ld3(contrib + 3 * (int64_t)it);
    }
    st3(out + 3 * (int64_t)v, s);
}

// ---------------------------------------------------------------------------------------------------- normal consistency
struct PairGeom {
    V3 e, ea, eb, n0, n1, x, y;
    float L0, L1;
};

__device__ __forceinline__ void pair_geom(V3 p0, V3 p1, V3 pa, V3 pb, PairGeom& g)
{
    g.e = p1 - p0;
    g.ea = pa - p0;
    g.eb = pb - p0;
    g.n0 = cross(g.e, g.ea);
    g.n1 = -cross(g.e, g.eb);
    g.x = normalize(g.n0, MB_EPS_COSINE, g.L0);          // cosine_similarity: x / max(|x|, eps) . y / max(|y|, eps)
    g.y = normalize(g.n1, MB_EPS_COSINE, g.L1);
}

__device__ __forceinline__ bool pair_ok(const int* q, int V)
{
    return q[0] >= 0 && q[0] < V && q[1] >= 0 && q[1] < V && q[2] >= 0 && q[2] < V && q[3] >= 0 && q[3] < V;
}

__global__ void __launch_bounds__(NC_THREADS) k_nc_forward(int n_pairs, int V, const float* __restrict__ verts, const int* __restrict__ pairs,
                                                            double* __restrict__ partials)
{
    __shared__ double red[NC_THREADS];
    double acc = 0.0;
    for (int64_t p = (int64_t)blockIdx.x * NC_THREADS + threadIdx.x; p < n_pairs; p += (int64_t)NC_BLOCKS * NC_THREADS) {
        const int* q = pairs + 4 * p;
        float loss = NAN;
        if (pair_ok(q, V)) {
            PairGeom g;
            pair_geom(ld3(verts + 3 * (int64_t)q[0]), ld3(verts + 3 * (int64_t)q[1]), ld3(verts + 3 * (int64_t)q[2]),
                      ld3(verts + 3 * (int64_t)q[3]), g);
            loss = 1.0f - dot(g.x, g.y);
        }
        acc += (double)loss;
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = NC_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) partials[blockIdx.x] = red[0];
}

__global__ void __launch_bounds__(NC_THREADS) k_nc_sum(int n_pairs, const double* __restrict__ partials, float* __restrict__ loss)
{
    __shared__ double red[NC_THREADS];
    double acc = 0.0;
    for (int i = threadIdx.x; i < NC_BLOCKS; i += NC_THREADS) acc += partials[i];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = NC_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = (float)(red[0] / (double)n_pairs);
}

// contrib[4p + s] = dL/d(slot s of pair p), slots (v0, v1, a, b); L = grad_loss / n_pairs * sum_p (1 - x_p . y_p)
__global__ void __launch_bounds__(256) k_nc_backward(int n_pairs, int V, const float* __restrict__ verts, const int* __restrict__ pairs,
                                                     const float* __restrict__ grad_loss, float* __restrict__ contrib)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pairs) return;
    const int* q = pairs + 4 * (int64_t)p;
    float* o = contrib + 12 * (int64_t)p;
    if (!pair_ok(q, V)) {
        for (int i = 0; i < 12; ++i) o[i] = NAN;
        return;
    }
    PairGeom g;
    pair_geom(ld3(verts + 3 * (int64_t)q[0]), ld3(verts + 3 * (int64_t)q[1]), ld3(verts + 3 * (int64_t)q[2]), ld3(verts + 3 * (int64_t)q[3]), g);
    const float w = -(grad_loss[0] / (float)n_pairs);
    const V3 dn0 = cosine_normalize_bwd(g.x, g.L0, MB_EPS_COSINE, w * g.y);
    const V3 dn1 = cosine_normalize_bwd(g.y, g.L1, MB_EPS_COSINE, w * g.x);
    // n0 = e x ea, n1 = -(e x eb)
    const V3 de = cross(g.ea, dn0) - cross(g.eb, dn1);
    const V3 dea = cross(dn0, g.e);
    const V3 deb = -cross(dn1, g.e);
    st3(o, -((de + dea) + deb));
    st3(o + 3, de);
    st3(o + 6, dea);
    st3(o + 9, deb);
}

const int64_t kMaxItems = ((int64_t)1 << 31) / 16;   // 3F, 4 n_pairs, F n: every flat float index stays below 2^31

}  // namespace

extern "C" {

int sgr_mesh_bind_forward(int F, int n, int V, const float* verts, const int32_t* faces, const float* bary, const float* scales,
                          const float* complex_numbers, const float* thickness, float* points, float* scaling, float* quaternions,
                          void* stream)
{
    if (F <= 0 || n <= 0 || (int64_t)F * n >= kMaxItems || (int64_t)F * 3 >= kMaxItems)
        return sgr_fail(SGR_E_INVALID, "mesh_bind_forward: F and n must be positive and F * max(n, 3) < 2^27");
    if (!points && !scaling && !quaternions) return sgr_fail(SGR_E_INVALID, "mesh_bind_forward: no output requested");
    if ((points || quaternions) && (V <= 0 || !verts || !faces)) return sgr_fail(SGR_E_INVALID, "mesh_bind_forward: verts / faces missing");
    if (points && !bary) return sgr_fail(SGR_E_INVALID, "mesh_bind_forward: points needs bary");
    if (scaling && (!scales || !thickness)) return sgr_fail(SGR_E_INVALID, "mesh_bind_forward: scaling needs scales and thickness");
    if (quaternions && !complex_numbers) return sgr_fail(SGR_E_INVALID, "mesh_bind_forward: quaternions needs complex_numbers");
    const int64_t P = (int64_t)F * n;
    hipLaunchKernelGGL(k_bind_forward, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, (hipStream_t)stream, F, n, V, verts, faces, bary,
                       scales, complex_numbers, thickness, points, scaling, quaternions);
    return hipGetLastError() == hipSuccess ? 0 : sgr_fail(SGR_E_HIP, "mesh_bind_forward: launch failed");
}

int sgr_mesh_bind_backward(int F, int n, int V, const float* verts, const int32_t* faces, const float* bary, const float* scales,
                           const float* complex_numbers, const float* dL_dpoints, const float* dL_dscaling, const float* dL_dquaternions,
                           const int32_t* vert_offsets, const int32_t* vert_items, float* contrib, float* dL_dverts, float* dL_dscales,
                           float* dL_dcomplex, void* stream)
{
    if (F <= 0 || n <= 0 || (int64_t)F * n >= kMaxItems || (int64_t)F * 3 >= kMaxItems)
        return sgr_fail(SGR_E_INVALID, "mesh_bind_backward: F and n must be positive and F * max(n, 3) < 2^27");
    if (!dL_dpoints && !dL_dscaling && !dL_dquaternions) return sgr_fail(SGR_E_INVALID, "mesh_bind_backward: no cotangent given");
    const bool mesh = dL_dpoints || dL_dquaternions;
    if (mesh && (V <= 0 || !faces || !vert_offsets || !vert_items || !contrib || !dL_dverts))
        return sgr_fail(SGR_E_INVALID, "mesh_bind_backward: faces, the vertex CSR, contrib and dL_dverts are needed");
    if (dL_dquaternions && !verts) return sgr_fail(SGR_E_INVALID, "mesh_bind_backward: dL_dquaternions needs verts");
    if (dL_dpoints && !bary) return sgr_fail(SGR_E_INVALID, "mesh_bind_backward: dL_dpoints needs bary");
    if (dL_dscaling && (!scales || !dL_dscales)) return sgr_fail(SGR_E_INVALID, "mesh_bind_backward: dL_dscaling needs scales and dL_dscales");
    if (dL_dquaternions && (!complex_numbers || !dL_dcomplex))
        return sgr_fail(SGR_E_INVALID, "mesh_bind_backward: dL_dquaternions needs complex_numbers and dL_dcomplex");
    hipLaunchKernelGGL(k_bind_backward, dim3((unsigned)((F + 255) / 256)), dim3(256), 0, (hipStream_t)stream, F, n, V, verts, faces, bary,
                       scales, complex_numbers, dL_dpoints, dL_dscaling, dL_dquaternions, contrib, dL_dscales, dL_dcomplex);
    if (mesh)
        hipLaunchKernelGGL(k_gather_vertex, dim3((unsigned)((V + 255) / 256)), dim3(256), 0, (hipStream_t)stream, V, 3 * F, vert_offsets,
                           vert_items, contrib, dL_dverts);
    return hipGetLastError() == hipSuccess ? 0 : sgr_fail(SGR_E_HIP, "mesh_bind_backward: launch failed");
}

size_t sgr_normal_consistency_scratch_bytes(void) { return (size_t)NC_BLOCKS * sizeof(double); }

int sgr_normal_consistency_forward(int n_pairs, int V, const float* verts, const int32_t* pairs, void* scratch, float* loss, void* stream)
{
    if (n_pairs <= 0 || V <= 0 || (int64_t)n_pairs * 4 >= kMaxItems || !verts || !pairs || !scratch || !loss)
        return sgr_fail(SGR_E_INVALID, "normal_consistency_forward: n_pairs, V must be positive (4 n_pairs < 2^27), no null pointer");
    double* partials = reinterpret_cast<double*>(scratch);
    hipLaunchKernelGGL(k_nc_forward, dim3(NC_BLOCKS), dim3(NC_THREADS), 0, (hipStream_t)stream, n_pairs, V, verts, pairs, partials);
    hipLaunchKernelGGL(k_nc_sum, dim3(1), dim3(NC_THREADS), 0, (hipStream_t)stream, n_pairs, partials, loss);
    return hipGetLastError() == hipSuccess ? 0 : sgr_fail(SGR_E_HIP, "normal_consistency_forward: launch failed");
}

int sgr_normal_consistency_backward(int n_pairs, int V, const float* verts, const int32_t* pairs, const float* grad_loss,
                                    const int32_t* vert_offsets, const int32_t* vert_items, float* contrib, float* dL_dverts, void* stream)
{
    if (n_pairs <= 0 || V <= 0 || (int64_t)n_pairs * 4 >= kMaxItems || !verts || !pairs || !grad_loss || !vert_offsets || !vert_items ||
        !contrib || !dL_dverts)
        return sgr_fail(SGR_E_INVALID, "normal_consistency_backward: n_pairs, V must be positive (4 n_pairs < 2^27), no null pointer");
    hipLaunchKernelGGL(k_nc_backward, dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n_pairs, V, verts, pairs,
                       grad_loss, contrib);
    hipLaunchKernelGGL(k_gather_vertex, dim3((unsigned)((V + 255) / 256)), dim3(256), 0, (hipStream_t)stream, V, 4 * n_pairs, vert_offsets,
                       vert_items, contrib, dL_dverts);
    return hipGetLastError() == hipSuccess ? 0 : sgr_fail(SGR_E_HIP, "normal_consistency_backward: launch failed");
}

}  // extern "C"
