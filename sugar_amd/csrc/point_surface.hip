// point_surface.hip -- a LOCAL implicit surface from an oriented point cloud (implicit moving least squares, IMLS), evaluated only in the
// 8 x 8 x 8-point bricks near the cloud and meshed by marching_cubes.hip (C ABI: sgr_point_surface_* in include/sugar_raster.h;
// sugar_amd.point_surface drives it).  This is NOT Poisson reconstruction: there is no global solve, every value depends on the K
// nearest cloud points of its query only, and nothing is filled in where no point is near -- unobserved regions stay open.
//
// The rules (restated in numpy by tests/point_surface_restatement.py):
//   inputs   points[N,3], normals[N,3] float32, finite, the normals towards LOWER density; a support radius > 0, h = radius / 2,
//            inv = 1 / (h h); the neighbour list idx[0 .. K) of a query x (the K nearest cloud points, in the k-NN's order), 1 <= K <= 32.
//   value    all in float32, every operation rounded on its own (the file is built with -ffp-contract=off):
//              d   = x - p_k                     per component
//              s_k = (dx dx + dy dy) + dz dz
//              c_k = (dx nx + dy ny) + dz nz
//              w_k = expf(-(s_k inv))
//              num = sum_k w_k c_k,  den = sum_k w_k            in list order, from 0
//            the query is DEFINED iff min_k s_k <= radius radius;
//              value  = -(num / den) where defined, NaN otherwise     (f <= 0 inside: marching_cubes(volume, 0) winds outwards)
//              weight = den          where defined, 0   otherwise
//            s_k is recomputed here in exactly this order (the k-NN's distances are not read), so the defined / undefined pattern is a
//            pure function of the inputs and the neighbour sets.  A list entry outside [0, N) is skipped.
//   bricks   the brick layout and linear index of sparse_sweep.hip.  Brick (i, j, k) is flagged iff a cloud point p lies in the box
//            [A[8 b_a] - r', A[min(8 b_a + 7, n_a - 1)] + r'] on every axis a, r' = radius (1 + 2^-20), in float64 arithmetic on the
//            float32 inputs.  The slack: a defined grid point has a cloud point with float32 s <= fl(radius radius); the five roundings
//            of s and the one of radius radius move the true distance by less than 4 x 2^-24 of itself, so that cloud point is within
//            radius (1 + 2^-22) of the grid point on every axis -- inside the grown box of the brick that holds the grid point.
//   spurious marching cubes counts a non-finite value as outside, so where f < 0 meets an undefined grid point it emits a wall at
//            t = 0.5.  A vertex with index coordinates c is SPURIOUS iff the volume at floor(c) or at ceil(c) (per component) is not
//            finite: an edge with a non-finite end always gets t = 0.5, and a vertex on a grid point has finite ends.
//
// Kernels (plain stores, no atomics: every output is a pure function of the inputs):
//   k_ps_mark      a lane per cloud point: binary searches for the brick range of each axis, then plain byte stores of 1 (a handful of
//                  bricks per point at the default radius of three spacings; racing identical stores need no atomic).
//   k_ps_pack      (point, normal) -> one 32-byte record, so that a neighbour is two 16-byte loads.
//   k_ps_eval      a lane per query (any query array: the brick points of the sweep and the mesh vertices alike).
//   k_ps_spurious  a lane per marching-cubes vertex.
#include "../../include/sugar_raster.h"
#include "sgr_common.h"

namespace {

#define PS_BRICK 8
#define PS_T 256
#define PS_MAX_K 32
#define PS_SLACK (1.0 + 1.0 / 1048576.0)   // r' = radius (1 + 2^-20)

struct PsGrid {
    int nx, ny, nz;
    int nbx, nby, nbz;
    const float* X;
    const float* Y;
    const float* Z;
};

// the inclusive range [lo, hi] of the bricks of one ascending axis whose grown span [A[8 b] - r, A[min(8 b + 7, n - 1)] + r] holds v;
// hi < lo: none.  Both ends of the spans ascend with b, so each bound is one binary search.
__device__ __forceinline__ void ps_axis_range(const float* __restrict__ A, int n, int nb, double v, double r, int& lo, int& hi)
{
    int a = 0, b = nb;                       // lo = the first brick whose upper end reaches v
    while (a < b) {
        const int mid = (a + b) >> 1;
        if ((double)A[min(mid * PS_BRICK + PS_BRICK - 1, n - 1)] + r >= v) b = mid; else a = mid + 1;
    }
    lo = a;
    a = 0; b = nb;                           // hi + 1 = the number of bricks whose lower end is at or below v
    while (a < b) {
        const int mid = (a + b) >> 1;
        if ((double)A[mid * PS_BRICK] - r <= v) a = mid + 1; else b = mid;
    }
    hi = a - 1;
}

__global__ void __launch_bounds__(PS_T) k_ps_mark(int N, const float* __restrict__ points, double r, PsGrid G, uint8_t* __restrict__ flags)
{
    const int g = blockIdx.x * PS_T + threadIdx.x;
    if (g >= N) return;
    const float px = points[3 * (int64_t)g], py = points[3 * (int64_t)g + 1], pz = points[3 * (int64_t)g + 2];
    if (!(fabsf(px) <= 3.402823466e+38f) || !(fabsf(py) <= 3.402823466e+38f) || !(fabsf(pz) <= 3.402823466e+38f)) return;
    int lo[3], hi[3];
    ps_axis_range(G.X, G.nx, G.nbx, (double)px, r, lo[0], hi[0]);
    ps_axis_range(G.Y, G.ny, G.nby, (double)py, r, lo[1], hi[1]);
    ps_axis_range(G.Z, G.nz, G.nbz, (double)pz, r, lo[2], hi[2]);
    if (hi[0] < lo[0] || hi[1] < lo[1] || hi[2] < lo[2]) return;
    for (int i = lo[0]; i <= hi[0]; ++i)
        for (int j = lo[1]; j <= hi[1]; ++j)
            for (int k = lo[2]; k <= hi[2]; ++k) {
                uint8_t* f = flags + ((int64_t)i * G.nby + j) * G.nbz + k;
                if (!*f) *f = 1;             // (most bricks of a dense cloud are flagged already; the racing read only saves stores)
            }
}

__global__ void __launch_bounds__(PS_T) k_ps_pack(int N, const float* __restrict__ points, const float* __restrict__ normals,
                                                  float4* __restrict__ packed)
{
    const int g = blockIdx.x * PS_T + threadIdx.x;
    if (g >= N) return;
    const float* p = points + 3 * (int64_t)g;
    const float* n = normals + 3 * (int64_t)g;
    packed[2 * (int64_t)g] = make_float4(p[0], p[1], p[2], n[0]);
    packed[2 * (int64_t)g + 1] = make_float4(n[1], n[2], 0.f, 0.f);
}

__global__ void __launch_bounds__(PS_T) k_ps_eval(int64_t n, int K, const float* __restrict__ x, const int64_t* __restrict__ idx, int N,
                                                  const float4* __restrict__ packed, float radius, float* __restrict__ value,
                                                  float* __restrict__ weight)
{
    const int64_t t = (int64_t)blockIdx.x * PS_T + threadIdx.x;
    if (t >= n) return;
    const float qx = x[3 * t], qy = x[3 * t + 1], qz = x[3 * t + 2];
    const float h = radius * 0.5f;
    const float inv = 1.0f / (h * h);
    const float r2 = radius * radius;
    const int64_t* row = idx + t * K;
    float num = 0.f, den = 0.f, smin = __int_as_float(0x7f800000);
    for (int k = 0; k < K; ++k) {
        const int64_t j = row[k];
        if (j < 0 || j >= N) continue;
        const float4 a = packed[2 * j], b = packed[2 * j + 1];
        const float dx = qx - a.x, dy = qy - a.y, dz = qz - a.z;
        const float s = (dx * dx + dy * dy) + dz * dz;
        const float c = (dx * a.w + dy * b.x) + dz * b.y;
        const float w = expf(-(s * inv));
        num = num + w * c;
        den = den + w;
        smin = fminf(smin, s);
    }
    const bool defined = smin <= r2;
    value[t] = defined ? -(num / den) : __int_as_float(0x7fc00000);
    if (weight) weight[t] = defined ? den : 0.f;
}

__device__ __forceinline__ bool ps_finite_at(const float* __restrict__ vol, const PsGrid G, float cx, float cy, float cz)
{
    const int i = min(max((int)cx, 0), G.nx - 1), j = min(max((int)cy, 0), G.ny - 1), k = min(max((int)cz, 0), G.nz - 1);
    return fabsf(vol[((int64_t)i * G.ny + j) * G.nz + k]) <= 3.402823466e+38f;
}

__global__ void __launch_bounds__(PS_T) k_ps_spurious(int V, const float* __restrict__ verts, PsGrid G, const float* __restrict__ vol,
                                                      uint8_t* __restrict__ spurious)
{
    const int v = blockIdx.x * PS_T + threadIdx.x;
    if (v >= V) return;
    const float cx = verts[3 * (int64_t)v], cy = verts[3 * (int64_t)v + 1], cz = verts[3 * (int64_t)v + 2];
    const bool ok = ps_finite_at(vol, G, floorf(cx), floorf(cy), floorf(cz)) && ps_finite_at(vol, G, ceilf(cx), ceilf(cy), ceilf(cz));
    spurious[v] = ok ? 0 : 1;                // (a NaN coordinate, which marching cubes never writes, reads grid point 0)
}

static bool ps_dims_ok(int nx, int ny, int nz) { return nx > 0 && ny > 0 && nz > 0 && (int64_t)nx * ny < ((int64_t)1 << 31) &&
                                                        (int64_t)nx * ny * nz < ((int64_t)1 << 31); }

static PsGrid ps_grid(int nx, int ny, int nz, const float* X, const float* Y, const float* Z)
{
    PsGrid G;
    G.nx = nx; G.ny = ny; G.nz = nz;
    G.nbx = (nx + PS_BRICK - 1) / PS_BRICK; G.nby = (ny + PS_BRICK - 1) / PS_BRICK; G.nbz = (nz + PS_BRICK - 1) / PS_BRICK;
    G.X = X; G.Y = Y; G.Z = Z;
    return G;
}

static inline unsigned ps_blocks(int64_t n) { return (unsigned)((n + PS_T - 1) / PS_T); }
static inline bool ps_radius_ok(float r) { return r > 0.f && r <= 3.402823466e+38f; }

}  // namespace

extern "C" {

int sgr_point_surface_mark(int N, const float* points, float radius, int nx, int ny, int nz, const float* X, const float* Y, const float* Z,
                           uint8_t* flags, int32_t* meta, void* stream)
{
    if (!ps_dims_ok(nx, ny, nz)) return sgr_fail(SGR_E_INVALID, "point_surface_mark: nx, ny, nz must be positive and nx * ny * nz < 2^31");
    if (N <= 0) return sgr_fail(SGR_E_INVALID, "point_surface_mark: N must be positive");
    if (!ps_radius_ok(radius)) return sgr_fail(SGR_E_INVALID, "point_surface_mark: radius must be finite and positive");
    if (!points || !X || !Y || !Z || !flags || !meta || ((uintptr_t)flags & 15)) return sgr_fail(SGR_E_INVALID, "point_surface_mark: null or misaligned pointer");
    const PsGrid G = ps_grid(nx, ny, nz, X, Y, Z);
    hipStream_t st = (hipStream_t)stream;
    const size_t padded = (size_t)(((int64_t)G.nbx * G.nby * G.nbz + 15) / 16 * 16);
    if (hipMemsetAsync(flags, 0, padded, st) != hipSuccess || hipMemsetAsync(meta, 0, 4 * sizeof(int32_t), st) != hipSuccess)
        return sgr_fail(SGR_E_HIP, "point_surface_mark: memset failed");
    hipLaunchKernelGGL(k_ps_mark, dim3(ps_blocks(N)), dim3(PS_T), 0, st, N, points, (double)radius * PS_SLACK, G, flags);
    return hipGetLastError() == hipSuccess ? 0 : sgr_fail(SGR_E_HIP, "point_surface_mark: launch failed");
}

int sgr_point_surface_pack(int N, const float* points, const float* normals, float* packed, void* stream)
{
    if (N <= 0) return sgr_fail(SGR_E_INVALID, "point_surface_pack: N must be positive");
    if (!points || !normals || !packed || ((uintptr_t)packed & 15)) return sgr_fail(SGR_E_INVALID, "point_surface_pack: null or misaligned pointer");
    hipLaunchKernelGGL(k_ps_pack, dim3(ps_blocks(N)), dim3(PS_T), 0, (hipStream_t)stream, N, points, normals, reinterpret_cast<float4*>(packed));
    return hipGetLastError() == hipSuccess ? 0 : sgr_fail(SGR_E_HIP, "point_surface_pack: launch failed");
}

int sgr_point_surface_eval(long long n, int K, const float* queries, const int64_t* idx, int N, const float* packed, float radius,
                           float* value, float* weight, void* stream)
{
    if (n < 0 || (n + PS_T - 1) / PS_T >= ((int64_t)1 << 31)) return sgr_fail(SGR_E_INVALID, "point_surface_eval: n must be in [0, 2^39)");
    if (n == 0) return 0;
    if (N <= 0 || K < 1 || K > PS_MAX_K) return sgr_fail(SGR_E_INVALID, "point_surface_eval: N must be positive and K in [1, 32]");
    if (!ps_radius_ok(radius)) return sgr_fail(SGR_E_INVALID, "point_surface_eval: radius must be finite and positive");
    if (!queries || !idx || !packed || !value || ((uintptr_t)packed & 15)) return sgr_fail(SGR_E_INVALID, "point_surface_eval: null or misaligned pointer");
    hipLaunchKernelGGL(k_ps_eval, dim3(ps_blocks(n)), dim3(PS_T), 0, (hipStream_t)stream, (int64_t)n, K, queries, idx, N,
                       reinterpret_cast<const float4*>(packed), radius, value, weight);
    return hipGetLastError() == hipSuccess ? 0 : sgr_fail(SGR_E_HIP, "point_surface_eval: launch failed");
}

int sgr_point_surface_spurious(int V, const float* verts_index, int nx, int ny, int nz, const float* volume, uint8_t* spurious, void* stream)
{
    if (!ps_dims_ok(nx, ny, nz)) return sgr_fail(SGR_E_INVALID, "point_surface_spurious: nx, ny, nz must be positive and nx * ny * nz < 2^31");
    if (V < 0) return sgr_fail(SGR_E_INVALID, "point_surface_spurious: V must not be negative");
    if (V == 0) return 0;
    if (!verts_index || !volume || !spurious) return sgr_fail(SGR_E_INVALID, "point_surface_spurious: null pointer");
    const PsGrid G = ps_grid(nx, ny, nz, nullptr, nullptr, nullptr);
    hipLaunchKernelGGL(k_ps_spurious, dim3(ps_blocks(V)), dim3(PS_T), 0, (hipStream_t)stream, V, verts_index, G, volume, spurious);
    return hipGetLastError() == hipSuccess ? 0 : sgr_fail(SGR_E_HIP, "point_surface_spurious: launch failed");
}

}  // extern "C"
