// marching_cubes.hip -- isosurface extraction of a dense scalar volume on gfx950 (C ABI: sgr_marching_cubes_*, sgr_mesh_vertex_normals,
// sgr_grid_points in include/sugar_raster.h).  The mesh-producing step of SuGaR's `use_marching_cubes` branch
// (sugar_extractors/coarse_mesh.py:623-757), which the reference runs on the host through PyMCubes.
//
// Volume: float32 [nx, ny, nz], contiguous, z fastest; point (x, y, z) has the linear index p = (x ny + y) nz + z.
//
// Semantics (restated serially by tests/mc_restatement.py, which reads the same mc_table.h; -ffp-contract=off keeps them bit-identical):
//   * a corner is INSIDE iff its value is finite and >= iso.  NaN and +-inf corners are OUTSIDE;
//   * a grid edge whose ends differ carries one vertex at t = (iso - a) / (b - a) from the outside end (a outside, b inside, three
//     individually rounded f32 operations), i.e. at index coordinate i + t when the lower end is outside and (i + 1) - t otherwise.
//     When the outside end is not finite, t = 0.5.  When b - a overflows to +inf, t = finite / inf = 0: the vertex sits exactly on
//     the outside grid point.  Only when iso - a overflows as well is t = inf / inf not finite, and then t = 0.5 too: never a NaN vertex;
//   * triangles come from mc_table.h, wound counter-clockwise seen from the lower values.
// Welding by ownership, no hash and no float atomics: every grid point owns its +x, +y, +z edges; the id of a vertex is the exclusive
// scan of the owned crossing edges in linear point order, then axis order; triangles are numbered in linear cell order (the cell of
// point p is the one with p as its lowest corner), then table order.  The output is a pure function of the volume.
//
// Passes:
//   k_mc_classify    one LDS tile of inside flags (8 x 8 x 32 points + a one-point halo) per workgroup; every value is read once per tile
//                    and compared once.  Writes a byte per point (bit a: the +a edge is crossed) and a byte per cell (the case).
//   k_mc_group_scan  16 points per thread (one 16-byte load of each byte array): vertex and triangle counts, an exclusive scan inside
//                    the workgroup (wave shuffles + 4 wave totals in LDS), one packed u32 per group and per workgroup.
//   k_mc_block_scan  one workgroup scans the workgroup totals in 64 bits and writes (n_vertices, n_faces).
//   k_mc_emit_verts / k_mc_emit_faces   four points / cells per thread; a face looks its three vertices up as
//                    base[owner's group] + (set bits of the group's mask bytes below the owner) + (owned edges below the axis).
// No kernel communicates with another workgroup inside a launch.
#include "../../include/sugar_raster.h"
#include "sgr_device.h"
#define MC_TABLE_QUAL static __device__ const
#include "mc_table.h"

namespace {

#define MC_TX 8
#define MC_TY 8
#define MC_TZ 32
#define MC_GROUP 16          // points per scan group: one 16-byte load of mask bytes
#define MC_SCAN_THREADS 256  // groups per workgroup of k_mc_group_scan: 4096 points, at most 12288 vertices / 20480 triangles (< 2^16)
#define MC_BLOCK_SCAN_THREADS 1024
#define MC_FLT_MAX 3.402823466e+38f

struct McLayout {
    size_t edge_mask, cell_case, grp, blk, blk_v, blk_t, total;
    int64_t N, N16, G, NB;
};

static McLayout mc_layout(int64_t N)
{
    McLayout L;
    L.N = N;
    L.N16 = (N + MC_GROUP - 1) / MC_GROUP * MC_GROUP;
    L.G = L.N16 / MC_GROUP;
    L.NB = (L.G + MC_SCAN_THREADS - 1) / MC_SCAN_THREADS;
    size_t off = 0;
    L.edge_mask = off; off = sgr_align(off + (size_t)L.N16);
    L.cell_case = off; off = sgr_align(off + (size_t)L.N16);
    L.grp = off;       off = sgr_align(off + (size_t)L.G * 4);
    L.blk = off;       off = sgr_align(off + (size_t)L.NB * 4);
    L.blk_v = off;     off = sgr_align(off + (size_t)L.NB * 4);
    L.blk_t = off;     off = sgr_align(off + (size_t)L.NB * 4);
    L.total = off;
    return L;
}

__device__ __forceinline__ bool mc_finite(float v) { return fabsf(v) <= MC_FLT_MAX; }
__device__ __forceinline__ bool mc_inside(float v, float iso) { return v >= iso && mc_finite(v); }

// ------------------------------------------------------------------------------------------------------------------- classify
__global__ void __launch_bounds__(256) k_mc_classify(int nx, int ny, int nz, int bx, int by, int bz, const float* __restrict__ vol, float iso,
                                                     uint8_t* __restrict__ edge_mask, uint8_t* __restrict__ cell_case)
{
    __shared__ uint8_t in_s[MC_TX + 1][MC_TY + 1][MC_TZ + 1];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int tz0 = (int)(b % bz) * MC_TZ;
    const int ty0 = (int)((b / bz) % by) * MC_TY;
    const int tx0 = (int)(b / ((int64_t)bz * by)) * MC_TX;
    for (int i = tid; i < (MC_TX + 1) * (MC_TY + 1) * (MC_TZ + 1); i += 256) {
        const int lz = i % (MC_TZ + 1);
        const int ly = (i / (MC_TZ + 1)) % (MC_TY + 1);
        const int lx = i / ((MC_TZ + 1) * (MC_TY + 1));
        const int x = tx0 + lx, y = ty0 + ly, z = tz0 + lz;
        uint8_t f = 0;
        if (x < nx && y < ny && z < nz) f = mc_inside(vol[((int64_t)x * ny + y) * nz + z], iso) ? 1 : 0;
        in_s[lx][ly][lz] = f;
    }
    __syncthreads();
    const int lz = tid & (MC_TZ - 1), ly = tid >> 5;
    const int y = ty0 + ly, z = tz0 + lz;
    if (y >= ny || z >= nz) return;
    const bool hy = y + 1 < ny, hz = z + 1 < nz;
#pragma unroll
    for (int lx = 0; lx < MC_TX; ++lx) {
        const int x = tx0 + lx;
        if (x >= nx) break;
        const bool hx = x + 1 < nx;
        const uint32_t c0 = in_s[lx][ly][lz], c1 = in_s[lx + 1][ly][lz], c2 = in_s[lx][ly + 1][lz], c3 = in_s[lx + 1][ly + 1][lz];
        const uint32_t c4 = in_s[lx][ly][lz + 1], c5 = in_s[lx + 1][ly][lz + 1], c6 = in_s[lx][ly + 1][lz + 1],
                       c7 = in_s[lx + 1][ly + 1][lz + 1];
        uint32_t m = 0;
        if (hx) m |= (c0 ^ c1);
        if (hy) m |= (c0 ^ c2) << 1;
        if (hz) m |= (c0 ^ c4) << 2;
        uint32_t cs = 0;
        if (hx && hy && hz) cs = c0 | (c1 << 1) | (c2 << 2) | (c3 << 3) | (c4 << 4) | (c5 << 5) | (c6 << 6) | (c7 << 7);
        const int64_t p = ((int64_t)x * ny + y) * nz + z;
        edge_mask[p] = (uint8_t)m;
        cell_case[p] = (uint8_t)cs;
    }
}

// ------------------------------------------------------------------------------------------------------------------- scans
__device__ __forceinline__ uint32_t mc_word_tris(uint32_t w, const uint8_t* ntri)
{
    if (w == 0u || w == 0xFFFFFFFFu) return 0u;
    return (uint32_t)ntri[w & 255u] + ntri[(w >> 8) & 255u] + ntri[(w >> 16) & 255u] + ntri[w >> 24];
}

// grp[g] = (vertices | triangles << 16) of the groups before g in its workgroup; blk[b] = the workgroup's totals, packed the same way
__global__ void __launch_bounds__(MC_SCAN_THREADS) k_mc_group_scan(int64_t G, const uint8_t* __restrict__ edge_mask,
                                                                   const uint8_t* __restrict__ cell_case, uint32_t* __restrict__ grp,
                                                                   uint32_t* __restrict__ blk)
{
    __shared__ uint8_t ntri[256];
    __shared__ uint32_t wave_tot[MC_SCAN_THREADS / 64];
    const int tid = threadIdx.x;
    ntri[tid] = MC_NTRI[tid];
    __syncthreads();
    const int64_t g = (int64_t)blockIdx.x * MC_SCAN_THREADS + tid;
    uint32_t x = 0;
    if (g < G) {
        const uint4 m = reinterpret_cast<const uint4*>(edge_mask)[g];
        const uint4 c = reinterpret_cast<const uint4*>(cell_case)[g];
        const uint32_t v = __popc(m.x) + __popc(m.y) + __popc(m.z) + __popc(m.w);
        const uint32_t t = mc_word_tris(c.x, ntri) + mc_word_tris(c.y, ntri) + mc_word_tris(c.z, ntri) + mc_word_tris(c.w, ntri);
        x = v | (t << 16);
    }
    uint32_t before;
    const uint32_t total = sgr_block_scan<MC_SCAN_THREADS / 64>(x, wave_tot, before);
    if (g < G) grp[g] = before;
    if (tid == 0) blk[blockIdx.x] = total;
}

// blk[NB] packed totals -> blk_v[NB], blk_t[NB]: exclusive offsets (low 32 bits; the caller refuses totals >= 2^31), counts[2] = totals
__global__ void __launch_bounds__(MC_BLOCK_SCAN_THREADS) k_mc_block_scan(int64_t NB, const uint32_t* __restrict__ blk, uint32_t* __restrict__ blk_v,
                                                                         uint32_t* __restrict__ blk_t, int64_t* __restrict__ counts)
{
    __shared__ unsigned long long sv[MC_BLOCK_SCAN_THREADS], st[MC_BLOCK_SCAN_THREADS];
    const int tid = threadIdx.x;
    const int64_t per = (NB + MC_BLOCK_SCAN_THREADS - 1) / MC_BLOCK_SCAN_THREADS;
    const int64_t lo = tid * per, hi = (lo + per < NB) ? lo + per : NB;
    unsigned long long v = 0, t = 0;
    for (int64_t i = lo; i < hi; ++i) {
        const uint32_t x = blk[i];
        v += x & 0xFFFFu;
        t += x >> 16;
    }
    sv[tid] = v;
    st[tid] = t;
    __syncthreads();
    for (int d = 1; d < MC_BLOCK_SCAN_THREADS; d <<= 1) {
        unsigned long long av = 0, at = 0;
        if (tid >= d) { av = sv[tid - d]; at = st[tid - d]; }
        __syncthreads();
        sv[tid] += av;
        st[tid] += at;
        __syncthreads();
    }
    unsigned long long ev = sv[tid] - v, et = st[tid] - t;   // exclusive
    for (int64_t i = lo; i < hi; ++i) {
        const uint32_t x = blk[i];
        blk_v[i] = (uint32_t)ev;
        blk_t[i] = (uint32_t)et;
        ev += x & 0xFFFFu;
        et += x >> 16;
    }
    if (tid == MC_BLOCK_SCAN_THREADS - 1) {
        counts[0] = (int64_t)sv[tid];
        counts[1] = (int64_t)st[tid];
    }
}

// ------------------------------------------------------------------------------------------------------------------- emit
// the id of the vertex on the +axis edge of point q (the edge must be crossed)
__device__ __forceinline__ uint32_t mc_vertex_id(int64_t q, int axis, const uint8_t* __restrict__ edge_mask, const uint32_t* __restrict__ grp,
                                                 const uint32_t* __restrict__ blk_v)
{
    const int64_t g = q >> 4;
    const int r = (int)(q & 15);
    const uint4 w4 = reinterpret_cast<const uint4*>(edge_mask)[g];
    const uint32_t w[4] = {w4.x, w4.y, w4.z, w4.w};
    uint32_t id = blk_v[g / MC_SCAN_THREADS] + (grp[g] & 0xFFFFu);
    const int k = r >> 2, sh = (r & 3) * 8;
#pragma unroll
    for (int i = 0; i < 3; ++i)
        if (i < k) id += __popc(w[i]);
    const uint32_t cur = w[k];
    id += __popc(cur & ((1u << sh) - 1u));
    id += __popc((cur >> sh) & ((1u << axis) - 1u));
    return id;
}

__global__ void __launch_bounds__(256) k_mc_emit_verts(int nx, int ny, int nz, int64_t N, const float* __restrict__ vol, float iso,
                                                       const uint8_t* __restrict__ edge_mask, const uint32_t* __restrict__ grp,
                                                       const uint32_t* __restrict__ blk_v, int64_t n_verts, float* __restrict__ verts)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;   // points 4i .. 4i+3
    if (4 * i >= N) return;
    const uint32_t word = reinterpret_cast<const uint32_t*>(edge_mask)[i];
    if (word == 0u) return;
    const int64_t g = i >> 2;
    uint32_t id = blk_v[g / MC_SCAN_THREADS] + (grp[g] & 0xFFFFu);
    for (int k = 0; k < (int)(i & 3); ++k) id += __popc(reinterpret_cast<const uint32_t*>(edge_mask)[4 * g + k]);
    const int64_t stride[3] = {(int64_t)ny * nz, nz, 1};
    for (int k = 0; k < 4; ++k) {
        const uint32_t m = (word >> (8 * k)) & 7u;
        if (!m) continue;
        const int64_t p = 4 * i + k;
        if (p >= N) break;
        const int z = (int)(p % nz), y = (int)((p / nz) % ny), x = (int)(p / ((int64_t)nz * ny));
        const float c[3] = {(float)x, (float)y, (float)z};
        const float va = vol[p];
        const bool lo_in = mc_inside(va, iso);
        for (int axis = 0; axis < 3; ++axis) {
            if (!((m >> axis) & 1u)) continue;
            const float vb = vol[p + stride[axis]];
            const float out_v = lo_in ? vb : va, in_v = lo_in ? va : vb;
            float t = (iso - out_v) / (in_v - out_v);
            if (!mc_finite(out_v) || !mc_finite(t)) t = 0.5f;
            float o[3] = {c[0], c[1], c[2]};
            o[axis] = lo_in ? (c[axis] + 1.0f) - t : c[axis] + t;
            if ((int64_t)id < n_verts) {
                float* dst = verts + 3 * (int64_t)id;
                dst[0] = o[0]; dst[1] = o[1]; dst[2] = o[2];
            }
            ++id;
        }
    }
}

__global__ void __launch_bounds__(256) k_mc_emit_faces(int nx, int ny, int nz, int64_t N, const uint8_t* __restrict__ edge_mask,
                                                       const uint8_t* __restrict__ cell_case, const uint32_t* __restrict__ grp,
                                                       const uint32_t* __restrict__ blk_v, const uint32_t* __restrict__ blk_t,
                                                       int64_t n_verts, int64_t n_faces, int64_t* __restrict__ faces)
{
    __shared__ uint8_t ntri[256];
    __shared__ int8_t tri[256][3 * MC_MAX_TRIS];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;   // cells 4i .. 4i+3
    uint32_t word = 0;
    if (4 * i < N) word = reinterpret_cast<const uint32_t*>(cell_case)[i];
    const bool active = word != 0u && word != 0xFFFFFFFFu;
    if (!__syncthreads_or(active)) return;                        // most workgroups see no surface: they skip the tables
    ntri[threadIdx.x] = MC_NTRI[threadIdx.x];
    for (int k = threadIdx.x; k < 256 * 3 * MC_MAX_TRIS; k += 256) (&tri[0][0])[k] = MC_TRI[k / (3 * MC_MAX_TRIS)][k % (3 * MC_MAX_TRIS)];
    __syncthreads();
    if (!active) return;
    const int64_t g = i >> 2;
    uint32_t fid = blk_t[g / MC_SCAN_THREADS] + (grp[g] >> 16);
    for (int k = 0; k < (int)(i & 3); ++k) fid += mc_word_tris(reinterpret_cast<const uint32_t*>(cell_case)[4 * g + k], ntri);
    const int64_t sx = (int64_t)ny * nz, sy = nz;
    for (int k = 0; k < 4; ++k) {
        const uint32_t cs = (word >> (8 * k)) & 255u;
        const int nt = ntri[cs];
        if (!nt) continue;
        const int64_t p = 4 * i + k;
        for (int t = 0; t < nt; ++t, ++fid) {
            int64_t vid[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int e = tri[cs][3 * t + c];
                const int axis = e >> 2, j = e & 3;
                const int u = j & 1, v = j >> 1;
                // the owner corner: offsets (u, v) along the two other axes, in ascending axis order
                const int dx = axis == 0 ? 0 : u;
                const int dy = axis == 0 ? u : (axis == 1 ? 0 : v);
                const int dz = axis == 2 ? 0 : v;
                const int64_t q = p + dx * sx + dy * sy + dz;
                int64_t id = -1;
                if (q < N) id = (int64_t)mc_vertex_id(q, axis, edge_mask, grp, blk_v);
                vid[c] = id < n_verts ? id : -1;
            }
            if ((int64_t)fid < n_faces) {
                int64_t* dst = faces + 3 * (int64_t)fid;
                dst[0] = vid[0]; dst[1] = vid[1]; dst[2] = vid[2];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------- companions
// normals[v] = normalize(sum over the incident (face, corner) items of the face's area-weighted normal (b - a) x (c - a)), summed in list
// order; a vertex without faces, or whose sum has no length, gets 0
__global__ void __launch_bounds__(256) k_vertex_normals(int V, int64_t F, const float* __restrict__ verts, const int64_t* __restrict__ faces,
                                                        const int* __restrict__ offsets, const int* __restrict__ items,
                                                        float* __restrict__ normals)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    const int64_t n_items = 3 * F;
    int64_t lo = offsets[v], hi = offsets[v + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > n_items ? n_items : hi;
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (int64_t i = lo; i < hi; ++i) {
        const int it = items[i];
        if (it < 0 || it >= n_items) continue;
        const int64_t* f = faces + 3 * (int64_t)(it / 3);
        const int64_t a = f[0], b = f[1], c = f[2];
        if (a < 0 || a >= V || b < 0 || b >= V || c < 0 || c >= V) continue;
        const float* pa = verts + 3 * a; const float* pb = verts + 3 * b; const float* pc = verts + 3 * c;
        const float ux = pb[0] - pa[0], uy = pb[1] - pa[1], uz = pb[2] - pa[2];
        const float wx = pc[0] - pa[0], wy = pc[1] - pa[1], wz = pc[2] - pa[2];
        sx += uy * wz - uz * wy;
        sy += uz * wx - ux * wz;
        sz += ux * wy - uy * wx;
    }
    const float len = sqrtf(sx * sx + sy * sy + sz * sz);
    float* o = normals + 3 * (int64_t)v;
    if (len > 0.f && mc_finite(len)) { o[0] = sx / len; o[1] = sy / len; o[2] = sz / len; }
    else { o[0] = 0.f; o[1] = 0.f; o[2] = 0.f; }
}

// out[i] = (X[ix], Y[iy], Z[iz]) of the linear grid point start + i
__global__ void __launch_bounds__(256) k_grid_points(int ny, int nz, const float* __restrict__ X, const float* __restrict__ Y,
                                                     const float* __restrict__ Z, int64_t start, int64_t n, float* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t p = start + i;
    const int z = (int)(p % nz), y = (int)((p / nz) % ny), x = (int)(p / ((int64_t)nz * ny));
    float* o = out + 3 * i;
    o[0] = X[x]; o[1] = Y[y]; o[2] = Z[z];
}

static bool mc_dims_ok(int nx, int ny, int nz) { return nx > 0 && ny > 0 && nz > 0 && (int64_t)nx * ny < ((int64_t)1 << 31) &&
                                                        (int64_t)nx * ny * nz < ((int64_t)1 << 31); }

}  // namespace

extern "C" {

size_t sgr_marching_cubes_scratch_bytes(int nx, int ny, int nz)
{
    if (!mc_dims_ok(nx, ny, nz)) return 0;
    return mc_layout((int64_t)nx * ny * nz).total;
}

int sgr_marching_cubes_count(int nx, int ny, int nz, const float* volume, float iso, void* scratch, int64_t* counts, void* stream)
{
    if (!mc_dims_ok(nx, ny, nz)) return sgr_fail(SGR_E_INVALID, "marching_cubes_count: nx, ny, nz must be positive and nx * ny * nz < 2^31");
    if (!(fabsf(iso) <= MC_FLT_MAX)) return sgr_fail(SGR_E_INVALID, "marching_cubes_count: iso must be finite");
    if (!volume || !scratch || !counts) return sgr_fail(SGR_E_INVALID, "marching_cubes_count: null pointer");
    const McLayout L = mc_layout((int64_t)nx * ny * nz);
    char* s = reinterpret_cast<char*>(scratch);
    uint8_t* edge_mask = reinterpret_cast<uint8_t*>(s + L.edge_mask);
    uint8_t* cell_case = reinterpret_cast<uint8_t*>(s + L.cell_case);
    uint32_t* grp = reinterpret_cast<uint32_t*>(s + L.grp);
    uint32_t* blk = reinterpret_cast<uint32_t*>(s + L.blk);
    uint32_t* blk_v = reinterpret_cast<uint32_t*>(s + L.blk_v);
    uint32_t* blk_t = reinterpret_cast<uint32_t*>(s + L.blk_t);
    hipStream_t st = (hipStream_t)stream;
    // the last group's bytes beyond N (the classify pass writes [0, N) only)
    if (hipMemsetAsync(edge_mask + L.N16 - MC_GROUP, 0, MC_GROUP, st) != hipSuccess ||
        hipMemsetAsync(cell_case + L.N16 - MC_GROUP, 0, MC_GROUP, st) != hipSuccess)
        return sgr_fail(SGR_E_HIP, "marching_cubes_count: memset failed");
    const int bx = (nx + MC_TX - 1) / MC_TX, by = (ny + MC_TY - 1) / MC_TY, bz = (nz + MC_TZ - 1) / MC_TZ;
    const int64_t tiles = (int64_t)bx * by * bz;   // <= N < 2^31
    hipLaunchKernelGGL(k_mc_classify, dim3((unsigned)tiles), dim3(256), 0, st, nx, ny, nz, bx, by, bz, volume, iso, edge_mask, cell_case);
    hipLaunchKernelGGL(k_mc_group_scan, dim3((unsigned)L.NB), dim3(MC_SCAN_THREADS), 0, st, L.G, edge_mask, cell_case, grp, blk);
    hipLaunchKernelGGL(k_mc_block_scan, dim3(1), dim3(MC_BLOCK_SCAN_THREADS), 0, st, L.NB, blk, blk_v, blk_t, counts);
    return hipGetLastError() == hipSuccess ? 0 : sgr_fail(SGR_E_HIP, "marching_cubes_count: launch failed");
}

int sgr_marching_cubes_emit(int nx, int ny, int nz, const float* volume, float iso, const void* scratch, int64_t n_verts, int64_t n_faces,
                            float* verts, int64_t* faces, void* stream)
{
    if (!mc_dims_ok(nx, ny, nz)) return sgr_fail(SGR_E_INVALID, "marching_cubes_emit: nx, ny, nz must be positive and nx * ny * nz < 2^31");
    if (n_verts < 0 || n_faces < 0 || n_verts >= ((int64_t)1 << 31) || n_faces >= ((int64_t)1 << 31))
        return sgr_fail(SGR_E_INVALID, "marching_cubes_emit: n_verts and n_faces must be in [0, 2^31)");
    if (!volume || !scratch || (n_verts && !verts) || (n_faces && !faces)) return sgr_fail(SGR_E_INVALID, "marching_cubes_emit: null pointer");
    const McLayout L = mc_layout((int64_t)nx * ny * nz);
    const char* s = reinterpret_cast<const char*>(scratch);
    const uint8_t* edge_mask = reinterpret_cast<const uint8_t*>(s + L.edge_mask);
    const uint8_t* cell_case = reinterpret_cast<const uint8_t*>(s + L.cell_case);
    const uint32_t* grp = reinterpret_cast<const uint32_t*>(s + L.grp);
    const uint32_t* blk_v = reinterpret_cast<const uint32_t*>(s + L.blk_v);
    const uint32_t* blk_t = reinterpret_cast<const uint32_t*>(s + L.blk_t);
    hipStream_t st = (hipStream_t)stream;
    const unsigned blocks = (unsigned)((L.N16 / 4 + 255) / 256);
    if (n_verts)
        hipLaunchKernelGGL(k_mc_emit_verts, dim3(blocks), dim3(256), 0, st, nx, ny, nz, L.N, volume, iso, edge_mask, grp, blk_v, n_verts, verts);
    if (n_faces)
        hipLaunchKernelGGL(k_mc_emit_faces, dim3(blocks), dim3(256), 0, st, nx, ny, nz, L.N, edge_mask, cell_case, grp, blk_v, blk_t, n_verts,
                           n_faces, faces);
    return hipGetLastError() == hipSuccess ? 0 : sgr_fail(SGR_E_HIP, "marching_cubes_emit: launch failed");
}

int sgr_mesh_vertex_normals(int V, int64_t F, const float* verts, const int64_t* faces, const int32_t* vert_offsets,
                            const int32_t* vert_items, float* normals, void* stream)
{
    if (V <= 0 || F < 0 || 3 * F >= ((int64_t)1 << 31) || !verts || !vert_offsets || !normals || (F && (!faces || !vert_items)))
        return sgr_fail(SGR_E_INVALID, "mesh_vertex_normals: V must be positive, 3 F < 2^31, no null pointer");
    hipLaunchKernelGGL(k_vertex_normals, dim3((unsigned)((V + 255) / 256)), dim3(256), 0, (hipStream_t)stream, V, F, verts, faces, vert_offsets,
                       vert_items, normals);
    return hipGetLastError() == hipSuccess ? 0 : sgr_fail(SGR_E_HIP, "mesh_vertex_normals: launch failed");
}

int sgr_grid_points(int nx, int ny, int nz, const float* X, const float* Y, const float* Z, int64_t start, int64_t n, float* out,
                    void* stream)
{
    if (!mc_dims_ok(nx, ny, nz)) return sgr_fail(SGR_E_INVALID, "grid_points: nx, ny, nz must be positive and nx * ny * nz < 2^31");
    if (start < 0 || n < 0 || start + n > (int64_t)nx * ny * nz)
        return sgr_fail(SGR_E_INVALID, "grid_points: [start, start + n) must lie inside the grid");
    if (n == 0) return 0;
    if (!X || !Y || !Z || !out) return sgr_fail(SGR_E_INVALID, "grid_points: null pointer");
    hipLaunchKernelGGL(k_grid_points, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ny, nz, X, Y, Z, start, n, out);
    return hipGetLastError() == hipSuccess ? 0 : sgr_fail(SGR_E_HIP, "grid_points: launch failed");
}

}  // extern "C"
