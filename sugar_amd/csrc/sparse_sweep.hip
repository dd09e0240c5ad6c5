// sparse_sweep.hip -- the active-brick list of the sparse density-grid sweep (C ABI: sgr_sparse_sweep_* in include/sugar_raster.h;
// sugar_amd.extract.density_grid_sparse drives it).  The grid meshgrid(X, Y, Z) is cut into bricks of 8 x 8 x 8 points (brick
// (i, j, k) holds the points 8i .. 8i+7 and so on; edge bricks are partial; linear brick index (i nby + j) nbz + k, z fastest like the
// volume).  Only the bricks a Gaussian can reach are swept by the k-NN and the density kernel; every other point keeps the value 0.
//
// The rule (restated in float64 numpy by tests/sparse_sweep_restatement.py; DESIGN.md section 13 has the derivation):
//   * a Gaussian g reaches iff 2 K s_g > level; its Mahalanobis radius is m_g = sqrt(2 ln(2 K s_g / level));
//   * its box has the half-extent e_a = max(1.01 m_g sqrt(S_aa), gap_a) on axis a, S_aa = sum_i B_ai^2 sigma_i^4 with
//     sigma_i = 1 / |column i of B_g| (no matrix is inverted: every term is non-negative), gap_a = the largest spacing of axis a;
//   * the index range of the grid points inside [c_a - e_a, c_a + e_a], per axis; empty on any axis: nothing is marked;
//   * otherwise the range is widened by one index on each side, clipped, and every brick the index box touches is flagged.
// All of it is float64 arithmetic on the float32 inputs: a million Gaussians cost a few dozen operations each, and the flags then
// agree with the float64 restatement except where a grid point sits within float64 rounding of a box face.
//
// Kernels (no float atomics; the flags are a pure function of the inputs):
//   k_sparse_mark        a lane per Gaussian.  A box of at most SS_SMALL_BOX bricks is flagged by the lane itself with plain byte stores
//                        of 1 (racing identical stores need no atomic); a larger one is appended to a list (one integer atomic for the
//                        slot; the order of the list does not reach the flags).
//   k_sparse_mark_big    a workgroup per listed Gaussian (grid-stride over the list, whose length stays on the device): the 256 threads
//                        share the bricks of the box, so that a background-sized Gaussian covering every brick costs its wave nothing.
//   k_sparse_compact     one workgroup: clears the flags of the bricks wholly inside the `zero_inside` box, then turns the flags into the
//                        ascending list of active bricks (16 flags per thread and tile, sgr_block_scan over the 1024 threads, a running
//                        base from tile to tile) and writes the count; it also checks that the axes are strictly ascending.
//   k_sparse_points      the 512 points of each brick of a chunk of the list, brick-major and z fastest inside the brick; a lane beyond
//                        the grid in an edge brick repeats the clamped in-grid point.
//   k_sparse_scatter     the chunk's densities to their volume positions, from in-grid lanes only.
#include "../../include/sugar_raster.h"
#include "sgr_device.h"

namespace {

#define SS_BRICK 8
#define SS_BRICK_POINTS 512
#define SS_SMALL_BOX 8           // bricks a lane flags itself (2 x 2 x 2: a Gaussian of a few grid spacings); above it: k_sparse_mark_big
#define SS_BIG_BLOCKS 1024       // workgroups of k_sparse_mark_big (grid-stride over the list)
#define SS_COMPACT_THREADS 1024
#define SS_META_COUNT 0          // meta[4] (int32, device): active bricks, axes not ascending, listed big Gaussians, unused
#define SS_META_BAD_AXIS 1
#define SS_META_BIG 2

struct SsGrid {
    int nx, ny, nz;
    int nbx, nby, nbz;
    const float* X;
    const float* Y;
    const float* Z;
};

struct SsBox {
    int lo[3], hi[3];  // brick ranges, inclusive; hi < lo on any axis: nothing to mark
};

// number of entries of the ascending axis A[n] that are < v (strict == true) or <= v; 0 when v is NaN
__device__ __forceinline__ int ss_count_below(const float* __restrict__ A, int n, double v, bool strict)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const double a = (double)A[mid];
        if (strict ? a < v : a <= v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the brick box of Gaussian g, or an empty one
__device__ __forceinline__ SsBox ss_box(const float4* __restrict__ packed, int g, int K, double level, const SsGrid G,
                                        const double* __restrict__ gap)
{
    SsBox box;
#pragma unroll
    for (int a = 0; a < 3; ++a) { box.lo[a] = 0; box.hi[a] = -1; }
    const float4* r = packed + 4 * (size_t)g;
    const float4 r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3];
    const double reach = 2.0 * (double)K * (double)r0.w;
    if (!(reach > level)) return box;
    const double m = sqrt(2.0 * log(reach / level));
    const double B[9] = {r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w, r3.x};   // row-major: B[3 a + i]
    double inv_n4[3];                                                              // sigma_i^4 = 1 / |column i|^4
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double n2 = B[i] * B[i] + B[3 + i] * B[3 + i] + B[6 + i] * B[6 + i];
        inv_n4[i] = 1.0 / (n2 * n2);
    }
    const double c[3] = {r0.x, r0.y, r0.z};
    const int n[3] = {G.nx, G.ny, G.nz};
    const float* A[3] = {G.X, G.Y, G.Z};
    int i0[3], i1[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double S = B[3 * a] * B[3 * a] * inv_n4[0] + B[3 * a + 1] * B[3 * a + 1] * inv_n4[1] + B[3 * a + 2] * B[3 * a + 2] * inv_n4[2];
        const double e = fmax(1.01 * m * sqrt(S), gap[a]);                         // (fmax drops a NaN first operand: the floor holds)
        i0[a] = ss_count_below(A[a], n[a], c[a] - e, true);
        i1[a] = ss_count_below(A[a], n[a], c[a] + e, false) - 1;
    }
    if (i1[0] < i0[0] || i1[1] < i0[1] || i1[2] < i0[2]) return box;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        box.lo[a] = max(i0[a] - 1, 0) / SS_BRICK;
        box.hi[a] = min(i1[a] + 1, n[a] - 1) / SS_BRICK;
    }
    return box;
}

__global__ void __launch_bounds__(256) k_sparse_mark(int P, const float4* __restrict__ packed, int K, double level, SsGrid G,
                                                     const double* __restrict__ gap, uint8_t* __restrict__ flags,
                                                     int32_t* __restrict__ big_list, int32_t* __restrict__ meta)
{
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= P) return;
    const SsBox b = ss_box(packed, g, K, level, G, gap);
    if (b.hi[0] < b.lo[0]) return;
    const int64_t cnt = (int64_t)(b.hi[0] - b.lo[0] + 1) * (b.hi[1] - b.lo[1] + 1) * (b.hi[2] - b.lo[2] + 1);
    if (cnt > SS_SMALL_BOX) {
        const int slot = atomicAdd(&meta[SS_META_BIG], 1);
        if (slot >= 0 && slot < P) big_list[slot] = g;
        return;
    }
    for (int i = b.lo[0]; i <= b.hi[0]; ++i)
        for (int j = b.lo[1]; j <= b.hi[1]; ++j)
            for (int k = b.lo[2]; k <= b.hi[2]; ++k) flags[((int64_t)i * G.nby + j) * G.nbz + k] = 1;
}

__global__ void __launch_bounds__(256) k_sparse_mark_big(int P, const float4* __restrict__ packed, int K, double level, SsGrid G,
                                                         const double* __restrict__ gap, uint8_t* __restrict__ flags,
                                                         const int32_t* __restrict__ big_list, const int32_t* __restrict__ meta)
{
    const int n_big = min(meta[SS_META_BIG], P);
    for (int e = blockIdx.x; e < n_big; e += gridDim.x) {
        const int g = big_list[e];
        if (g < 0 || g >= P) continue;
        const SsBox b = ss_box(packed, g, K, level, G, gap);   // (every thread forms the same box: no barrier, no LDS)
        if (b.hi[0] < b.lo[0]) continue;
        const int sy = b.hi[1] - b.lo[1] + 1, sz = b.hi[2] - b.lo[2] + 1;
        const int64_t cnt = (int64_t)(b.hi[0] - b.lo[0] + 1) * sy * sz;
        for (int64_t t = threadIdx.x; t < cnt; t += 256) {
            const int k = b.lo[2] + (int)(t % sz), j = b.lo[1] + (int)((t / sz) % sy), i = b.lo[0] + (int)(t / ((int64_t)sz * sy));
            uint8_t* f = flags + ((int64_t)i * G.nby + j) * G.nbz + k;
            if (!*f) *f = 1;   // (most bricks of a large box are flagged already; the racing read only saves stores)
        }
    }
}

// is every in-grid point of the bricks [b, b] of this axis strictly inside (lo, hi)?  The axis ascends: its two end points decide.
__device__ __forceinline__ bool ss_axis_inside(const float* __restrict__ A, int n, int b, float lo, float hi)
{
    return A[b * SS_BRICK] > lo && A[min(b * SS_BRICK + SS_BRICK - 1, n - 1)] < hi;
}

__global__ void __launch_bounds__(SS_COMPACT_THREADS) k_sparse_compact(SsGrid G, int has_box, float lo, float hi, int64_t n_bricks,
                                                                       uint8_t* __restrict__ flags, int32_t* __restrict__ list,
                                                                       int32_t* __restrict__ meta)
{
    __shared__ uint32_t s_wave[SS_COMPACT_THREADS / 64];
    const int tid = threadIdx.x;
    int bad = 0;
    for (int i = tid; i + 1 < G.nx; i += SS_COMPACT_THREADS) bad |= !(G.X[i] < G.X[i + 1]);
    for (int i = tid; i + 1 < G.ny; i += SS_COMPACT_THREADS) bad |= !(G.Y[i] < G.Y[i + 1]);
    for (int i = tid; i + 1 < G.nz; i += SS_COMPACT_THREADS) bad |= !(G.Z[i] < G.Z[i + 1]);
    bad = __syncthreads_or(bad);
    const int64_t groups = (n_bricks + 15) / 16;   // the flags are padded with zeros to a multiple of 16
    uint32_t base = 0;
    for (int64_t g0 = 0; g0 < groups; g0 += SS_COMPACT_THREADS) {
        const int64_t g = g0 + tid;
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        if (g < groups) {
            const uint4 v = reinterpret_cast<const uint4*>(flags)[g];
            w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        }
        if (has_box && (w[0] | w[1] | w[2] | w[3])) {
            bool changed = false;
            for (int k = 0; k < 16; ++k) {
                if (!((w[k >> 2] >> (8 * (k & 3))) & 0xFFu)) continue;
                const int64_t b = 16 * g + k;
                const int bk = (int)(b % G.nbz), bj = (int)((b / G.nbz) % G.nby), bi = (int)(b / ((int64_t)G.nbz * G.nby));
                if (ss_axis_inside(G.X, G.nx, bi, lo, hi) && ss_axis_inside(G.Y, G.ny, bj, lo, hi) && ss_axis_inside(G.Z, G.nz, bk, lo, hi)) {
                    w[k >> 2] &= ~(0xFFu << (8 * (k & 3)));
                    changed = true;
                }
            }
            if (changed) reinterpret_cast<uint4*>(flags)[g] = make_uint4(w[0], w[1], w[2], w[3]);
        }
        const uint32_t cnt = __popc(w[0]) + __popc(w[1]) + __popc(w[2]) + __popc(w[3]);   // a flag byte is 0 or 1
        uint32_t before;
        const uint32_t total = sgr_block_scan<SS_COMPACT_THREADS / 64>(cnt, s_wave, before);
        if (cnt) {
            int64_t pos = (int64_t)base + before;
            for (int k = 0; k < 16; ++k)
                if ((w[k >> 2] >> (8 * (k & 3))) & 0xFFu) {
                    if (pos < n_bricks) list[pos] = (int32_t)(16 * g + k);
                    ++pos;
                }
        }
        base += total;
    }
    if (tid == 0) {
        meta[SS_META_COUNT] = (int32_t)base;
        meta[SS_META_BAD_AXIS] = bad ? 1 : 0;
    }
}

// point t of the chunk -> its brick and the grid indices of its lane; false when the list entry is not a brick of this grid
__device__ __forceinline__ bool ss_lane(const SsGrid G, const int32_t* __restrict__ list, int b0, int64_t t, int& x, int& y, int& z)
{
    const int64_t b = list[b0 + (t >> 9)];
    if (b < 0 || b >= (int64_t)G.nbx * G.nby * G.nbz) return false;
    const int l = (int)(t & (SS_BRICK_POINTS - 1));
    x = (int)(b / ((int64_t)G.nbz * G.nby)) * SS_BRICK + (l >> 6);
    y = (int)((b / G.nbz) % G.nby) * SS_BRICK + ((l >> 3) & 7);
    z = (int)(b % G.nbz) * SS_BRICK + (l & 7);
    return true;
}

__global__ void __launch_bounds__(256) k_sparse_points(SsGrid G, const int32_t* __restrict__ list, int b0, int64_t n, float* __restrict__ out)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    int x = 0, y = 0, z = 0;
    ss_lane(G, list, b0, t, x, y, z);   // (an entry outside the grid, which the compaction never writes, gives the first grid point)
    float* o = out + 3 * t;
    o[0] = G.X[min(x, G.nx - 1)]; o[1] = G.Y[min(y, G.ny - 1)]; o[2] = G.Z[min(z, G.nz - 1)];
}

__global__ void __launch_bounds__(256) k_sparse_scatter(SsGrid G, const int32_t* __restrict__ list, int b0, int64_t n,
                                                        const float* __restrict__ dens, float* __restrict__ volume)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    int x, y, z;
    if (!ss_lane(G, list, b0, t, x, y, z)) return;
    if (x >= G.nx || y >= G.ny || z >= G.nz) return;
    volume[((int64_t)x * G.ny + y) * G.nz + z] = dens[t];
}

static bool ss_dims_ok(int nx, int ny, int nz) { return nx > 0 && ny > 0 && nz > 0 && (int64_t)nx * ny < ((int64_t)1 << 31) &&
                                                        (int64_t)nx * ny * nz < ((int64_t)1 << 31); }

static SsGrid ss_grid(int nx, int ny, int nz, const float* X, const float* Y, const float* Z)
{
    SsGrid G;
    G.nx = nx; G.ny = ny; G.nz = nz;
    G.nbx = (nx + SS_BRICK - 1) / SS_BRICK; G.nby = (ny + SS_BRICK - 1) / SS_BRICK; G.nbz = (nz + SS_BRICK - 1) / SS_BRICK;
    G.X = X; G.Y = Y; G.Z = Z;
    return G;
}

static int64_t ss_bricks(const SsGrid& G) { return (int64_t)G.nbx * G.nby * G.nbz; }

}  // namespace

extern "C" {

int sgr_sparse_sweep_mark(int P, const float* packed, int K, float level, int nx, int ny, int nz, const float* X, const float* Y,
                          const float* Z, const double* gap, uint8_t* flags, int32_t* big_list, int32_t* meta, void* stream)
{
    if (!ss_dims_ok(nx, ny, nz)) return sgr_fail(SGR_E_INVALID, "sparse_sweep_mark: nx, ny, nz must be positive and nx * ny * nz < 2^31");
    if (P <= 0 || K <= 0) return sgr_fail(SGR_E_INVALID, "sparse_sweep_mark: P and K must be positive");
    if (!(level > 0.f) || !(level <= 3.402823466e+38f)) return sgr_fail(SGR_E_INVALID, "sparse_sweep_mark: level must be finite and positive");
    if (!packed || !X || !Y || !Z || !gap || !flags || !big_list || !meta || ((uintptr_t)packed & 15) || ((uintptr_t)flags & 15))
        return sgr_fail(SGR_E_INVALID, "sparse_sweep_mark: null or misaligned pointer");
    const SsGrid G = ss_grid(nx, ny, nz, X, Y, Z);
    hipStream_t st = (hipStream_t)stream;
    const size_t padded = (size_t)((ss_bricks(G) + 15) / 16 * 16);
    if (hipMemsetAsync(flags, 0, padded, st) != hipSuccess || hipMemsetAsync(meta, 0, 4 * sizeof(int32_t), st) != hipSuccess)
        return sgr_fail(SGR_E_HIP, "sparse_sweep_mark: memset failed");
    const float4* pk = reinterpret_cast<const float4*>(packed);
    hipLaunchKernelGGL(k_sparse_mark, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, P, pk, K, (double)level, G, gap, flags, big_list, meta);
    hipLaunchKernelGGL(k_sparse_mark_big, dim3((unsigned)(P < SS_BIG_BLOCKS ? P : SS_BIG_BLOCKS)), dim3(256), 0, st, P, pk, K, (double)level, G,
                       gap, flags, big_list, meta);
    return hipGetLastError() == hipSuccess ? 0 : sgr_fail(SGR_E_HIP, "sparse_sweep_mark: launch failed");
}

int sgr_sparse_sweep_compact(int nx, int ny, int nz, const float* X, const float* Y, const float* Z, int has_box, float lo, float hi,
                             uint8_t* flags, int32_t* list, int32_t* meta, void* stream)
{
    if (!ss_dims_ok(nx, ny, nz)) return sgr_fail(SGR_E_INVALID, "sparse_sweep_compact: nx, ny, nz must be positive and nx * ny * nz < 2^31");
    if (!X || !Y || !Z || !flags || !list || !meta || ((uintptr_t)flags & 15))
        return sgr_fail(SGR_E_INVALID, "sparse_sweep_compact: null or misaligned pointer");
    const SsGrid G = ss_grid(nx, ny, nz, X, Y, Z);
    hipLaunchKernelGGL(k_sparse_compact, dim3(1), dim3(SS_COMPACT_THREADS), 0, (hipStream_t)stream, G, has_box ? 1 : 0, lo, hi, ss_bricks(G),
                       flags, list, meta);
    return hipGetLastError() == hipSuccess ? 0 : sgr_fail(SGR_E_HIP, "sparse_sweep_compact: launch failed");
}

int sgr_sparse_sweep_points(int nx, int ny, int nz, const float* X, const float* Y, const float* Z, const int32_t* list, int b0, int b1,
                            float* out, void* stream)
{
    if (!ss_dims_ok(nx, ny, nz)) return sgr_fail(SGR_E_INVALID, "sparse_sweep_points: nx, ny, nz must be positive and nx * ny * nz < 2^31");
    const SsGrid G = ss_grid(nx, ny, nz, X, Y, Z);
    if (b0 < 0 || b1 < b0 || b1 > ss_bricks(G)) return sgr_fail(SGR_E_INVALID, "sparse_sweep_points: [b0, b1) must lie inside the brick list");
    if (b1 == b0) return 0;
    if (!X || !Y || !Z || !list || !out) return sgr_fail(SGR_E_INVALID, "sparse_sweep_points: null pointer");
    const int64_t n = (int64_t)(b1 - b0) * SS_BRICK_POINTS;
    if ((n + 255) / 256 >= ((int64_t)1 << 31)) return sgr_fail(SGR_E_INVALID, "sparse_sweep_points: the chunk is too large");
    hipLaunchKernelGGL(k_sparse_points, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, G, list, b0, n, out);
    return hipGetLastError() == hipSuccess ? 0 : sgr_fail(SGR_E_HIP, "sparse_sweep_points: launch failed");
}

int sgr_sparse_sweep_scatter(int nx, int ny, int nz, const int32_t* list, int b0, int b1, const float* density, float* volume, void* stream)
{
    if (!ss_dims_ok(nx, ny, nz)) return sgr_fail(SGR_E_INVALID, "sparse_sweep_scatter: nx, ny, nz must be positive and nx * ny * nz < 2^31");
    const SsGrid G = ss_grid(nx, ny, nz, nullptr, nullptr, nullptr);
    if (b0 < 0 || b1 < b0 || b1 > ss_bricks(G)) return sgr_fail(SGR_E_INVALID, "sparse_sweep_scatter: [b0, b1) must lie inside the brick list");
    if (b1 == b0) return 0;
    if (!list || !density || !volume) return sgr_fail(SGR_E_INVALID, "sparse_sweep_scatter: null pointer");
    const int64_t n = (int64_t)(b1 - b0) * SS_BRICK_POINTS;
    if ((n + 255) / 256 >= ((int64_t)1 << 31)) return sgr_fail(SGR_E_INVALID, "sparse_sweep_scatter: the chunk is too large");
    hipLaunchKernelGGL(k_sparse_scatter, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, G, list, b0, n, density, volume);
    return hipGetLastError() == hipSuccess ? 0 : sgr_fail(SGR_E_HIP, "sparse_sweep_scatter: launch failed");
}

}  // extern "C"
