// mesh_decimate.hip -- quadric-error edge collapse in parallel rounds, and the mesh cleaning passes, on gfx950 (C ABI:
// sgr_mesh_decimate_* / sgr_mesh_clean_* in include/sugar_raster.h).  What the reference does between extraction and refinement with
// open3d's simplify_quadric_decimation and remove_* calls (sugar_extractors/coarse_mesh.py:586-605, :722-742), as native code.
//
// Everything is float64, individually rounded (-ffp-contract=off), in a stated operation order: tests/decimate_restatement.py restates
// every rule in numpy float64 and the GPU tests hold these kernels to it bit for bit.  No float atomics anywhere.
//
// State of a mesh during decimation: P[V,3] float64 (coordinates relative to the bounding-box centre), Q[V,10] float64 (the vertex
// quadric: the upper triangle of the symmetric 4 x 4 matrix, row-major: q0 q1 q2 q3 / q4 q5 q6 / q7 q8 / q9), faces[F,3] int32.
//
// Quadrics (k_md_vertex_quadrics, once):
//   * face (pa, pb, pc): n = (pb - pa) x (pc - pa), len = sqrt(n.n); a face with !(len > 0) contributes nothing.  Unit normal
//     (a, b, c) = n / len, d = -(a pa.x + b pa.y + c pa.z), weight w = 0.5 len (the area); K = md_plane_quadric(w, a, b, c, d);
//   * boundary edge k of the face (the edge opposite corner k, from vertex (k+1)%3 to vertex (k+2)%3; one incident face): e = pe - ps,
//     m = e x (a, b, c), ml = sqrt(m.m); nothing when !(ml > 0).  Plane normal m / ml through ps, weight boundary_weight * w;
//   * vertex v: Q[v] = sum over the items (face f, corner c) of its CSR list in ascending order of: K(f), then the boundary quadrics of
//     the edges k != c of f that are boundary edges, k ascending.  Every term is added to the running sum on its own.
// Edges (k_md_edge_build): incidence s = 3 f + k names edge k of face f; incidences are sorted by (lo * V + hi, s); edge id = rank of
// (lo, hi) among the distinct pairs.  An edge records its first two faces (ascending) and its face count capped at 3.
//
// Cost and position of edge (lo, hi) (k_md_edge_eval): Qe = Q[lo] + Q[hi];
//   c00 = q4 q7 - q5 q5, c01 = q2 q5 - q1 q7, c02 = q1 q5 - q2 q4, c11 = q0 q7 - q2 q2, c12 = q1 q2 - q0 q5, c22 = q0 q4 - q1 q1,
//   det = q0 c00 + q1 c01 + q2 c02, tr = q0 + q4 + q7;  x = -((c00 q3 + c01 q6 + c02 q8) / det), y, z alike with rows (c01 c11 c12), (c02 c12 c22).
//   The solve is used iff |det| > 1e-12 tr tr tr AND the point lies within one edge length of the edge midpoint (squared distances
//   compared; NaN fails).  Otherwise the candidates P[lo], P[hi], 0.5 (P[lo] + P[hi]) are tried in that order and the first with the
//   strictly smallest cost is taken.  cost = md_cost(Qe, x, y, z); a non-finite cost makes the edge invalid.
//   key of a valid edge = the cost's bits as an ordered int64 (negative values: bits ^ 0x7FFF...F); invalid edges get INT64_MAX.
// Validity: an edge is refused when
//   * it has more than two faces, or lo == hi, or its two opposite vertices coincide;
//   * it has two faces and both ends are boundary vertices (the collapse would pinch the surface);
//   * link condition: a vertex other than the opposite ones shares a face with both ends;
//   * both ends carry a surviving face over the two opposite vertices (the collapse would leave two faces on one vertex set);
//   * a surviving face (one at lo or hi that does not contain the other end) has dot(n_old, n_new) not > 0, with n = (p1 - ps) x (p2 - ps)
//     for the face's corners in cyclic order from the moved corner: a flip, and a zero-area (degenerate) face, whose dot is 0.
// Selection (k_md_claim, k_md_winners): the host sorts the keys (stable, so ties go to the lower edge id): rank r of a valid edge is its
// place in the order of (cost bits, edge id) -- a 64-bit integer that compares exactly as that pair does, and the value that is claimed
// with.  Candidates: ranks r < ceil(n_valid / 4), the lowest-keyed quarter of the valid edges.  SGR_MESH_DECIMATE_PASSES (4) selection
// passes per round: a live candidate (one that has not won, and none of whose vertices is locked by an earlier pass's winner) claims
// every vertex of every face at lo and at hi with a 64-bit integer atomicMin of r, and wins iff it holds every one of those claims; a
// winner locks those vertices.  Two winners of a round share no face, and the winners do not depend on scheduling.  (One pass alone
// picks about 1 edge in 75, which needs 67 rounds for a fourfold reduction; four passes need 22.)  The caller keeps winners in rank
// order while F - (faces removed by earlier winners) > target.
// Apply (k_md_apply_edges, k_md_apply_faces, k_md_compact_*): P[lo] = the position, Q[lo] += Q[hi] (lo's coefficient first), hi is renamed
// to lo; faces are renamed, those that repeat an index are dropped; vertices and faces are compacted by an inclusive scan of their keep
// flags (order kept).
#include "../../include/sugar_raster.h"
#include "sgr_common.h"

namespace {

#define MD_T 256
#define MD_KEY_INVALID 0x7FFFFFFFFFFFFFFFll
#define MD_DET_REL 1e-12

struct MdQ { double q0, q1, q2, q3, q4, q5, q6, q7, q8, q9; };

__device__ __forceinline__ MdQ md_zero() { MdQ r = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; return r; }
__device__ __forceinline__ MdQ md_load(const double* __restrict__ Q, int v)
{
    const double* p = Q + 10 * (int64_t)v;
    MdQ r = {p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9]};
    return r;
}
__device__ __forceinline__ void md_store(double* __restrict__ Q, int64_t v, const MdQ& r)
{
    double* p = Q + 10 * v;
    p[0] = r.q0; p[1] = r.q1; p[2] = r.q2; p[3] = r.q3; p[4] = r.q4; p[5] = r.q5; p[6] = r.q6; p[7] = r.q7; p[8] = r.q8; p[9] = r.q9;
}
__device__ __forceinline__ MdQ md_add(const MdQ& a, const MdQ& b)
{
    MdQ r = {a.q0 + b.q0, a.q1 + b.q1, a.q2 + b.q2, a.q3 + b.q3, a.q4 + b.q4, a.q5 + b.q5, a.q6 + b.q6, a.q7 + b.q7, a.q8 + b.q8, a.q9 + b.q9};
    return r;
}
// the quadric of the plane a x + b y + c z + d = 0 with weight w
__device__ __forceinline__ MdQ md_plane_quadric(double w, double a, double b, double c, double d)
{
    const double wa = w * a, wb = w * b, wc = w * c, wd = w * d;
    MdQ r = {wa * a, wa * b, wa * c, wa * d, wb * b, wb * c, wb * d, wc * c, wc * d, wd * d};
    return r;
}
__device__ __forceinline__ double md_cost(const MdQ& q, double x, double y, double z)
{
    return x * (q.q0 * x + q.q1 * y + q.q2 * z + q.q3) + y * (q.q1 * x + q.q4 * y + q.q5 * z + q.q6) +
           z * (q.q2 * x + q.q5 * y + q.q7 * z + q.q8) + (q.q3 * x + q.q6 * y + q.q8 * z + q.q9);
}
struct MdV { double x, y, z; };
__device__ __forceinline__ MdV md_point(const double* __restrict__ P, int v)
{
    const double* p = P + 3 * (int64_t)v;
    MdV r = {p[0], p[1], p[2]};
    return r;
}
__device__ __forceinline__ MdV md_sub(const MdV& a, const MdV& b) { MdV r = {a.x - b.x, a.y - b.y, a.z - b.z}; return r; }
__device__ __forceinline__ MdV md_cross(const MdV& u, const MdV& w)
{
    MdV r = {u.y * w.z - u.z * w.y, u.z * w.x - u.x * w.z, u.x * w.y - u.y * w.x};
    return r;
}
__device__ __forceinline__ double md_dot(const MdV& a, const MdV& b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ bool md_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

// the boundary quadric of the edge ps -> pe of a face with unit normal n and area w; false when the edge has no length
__device__ __forceinline__ bool md_boundary_quadric(const MdV& ps, const MdV& pe, const MdV& n, double w, double bw, MdQ* out)
{
    const MdV e = md_sub(pe, ps);
    const MdV m = md_cross(e, n);
    const double ml = sqrt(md_dot(m, m));
    if (!(ml > 0.0)) return false;
    const double a = m.x / ml, b = m.y / ml, c = m.z / ml;
    const double d = -(a * ps.x + b * ps.y + c * ps.z);
    *out = md_plane_quadric(bw * w, a, b, c, d);
    return true;
}

// ------------------------------------------------------------------------------------------------------------------- quadrics
__global__ void __launch_bounds__(MD_T) k_md_vertex_quadrics(int V, int F, const double* __restrict__ P, const int* __restrict__ faces,
                                                             const int* __restrict__ offsets, const int* __restrict__ items,
                                                             const uint8_t* __restrict__ bflag, double bw, double* __restrict__ Q)
{
    const int v = blockIdx.x * MD_T + threadIdx.x;
    if (v >= V) return;
    MdQ acc = md_zero();
    int lo = offsets[v], hi = offsets[v + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > 3 * F ? 3 * F : hi;
    for (int i = lo; i < hi; ++i) {
        const int it = items[i];
        if (it < 0 || it >= 3 * F) continue;
        const int f = it / 3, c = it - 3 * f;
        const int ia = faces[3 * f], ib = faces[3 * f + 1], ic = faces[3 * f + 2];
        if (ia < 0 || ia >= V || ib < 0 || ib >= V || ic < 0 || ic >= V) continue;
        const MdV pa = md_point(P, ia), pb = md_point(P, ib), pc = md_point(P, ic);
        const MdV n = md_cross(md_sub(pb, pa), md_sub(pc, pa));
        const double len = sqrt(md_dot(n, n));
        if (!(len > 0.0)) continue;
        const MdV nn = {n.x / len, n.y / len, n.z / len};
        const double d = -(nn.x * pa.x + nn.y * pa.y + nn.z * pa.z);
        const double w = 0.5 * len;
        acc = md_add(acc, md_plane_quadric(w, nn.x, nn.y, nn.z, d));
        MdQ b;
        if (c != 0 && bflag[3 * f + 0] && md_boundary_quadric(pb, pc, nn, w, bw, &b)) acc = md_add(acc, b);
        if (c != 1 && bflag[3 * f + 1] && md_boundary_quadric(pc, pa, nn, w, bw, &b)) acc = md_add(acc, b);
        if (c != 2 && bflag[3 * f + 2] && md_boundary_quadric(pa, pb, nn, w, bw, &b)) acc = md_add(acc, b);
    }
    md_store(Q, v, acc);
}

// ------------------------------------------------------------------------------------------------------------------- edges
// skey[n_inc] sorted (lo * V + hi), order[n_inc] the incidence of every sorted position, group[n_inc] the edge id of every sorted position.
// Writes one record per edge at its first sorted position; bflag[3F] and vbnd[V] must be zero on entry.
__global__ void __launch_bounds__(MD_T) k_md_edge_build(int n_inc, int V, const int64_t* __restrict__ skey, const int64_t* __restrict__ order,
                                                        const int64_t* __restrict__ group, int* __restrict__ e_lo, int* __restrict__ e_hi,
                                                        int* __restrict__ e_f0, int* __restrict__ e_f1, int* __restrict__ e_nf,
                                                        uint8_t* __restrict__ bflag, int* __restrict__ vbnd)
{
    const int i = blockIdx.x * MD_T + threadIdx.x;
    if (i >= n_inc) return;
    const int64_t k = skey[i];
    if (i > 0 && skey[i - 1] == k) return;
    int cnt = 1;
    while (cnt < 3 && i + cnt < n_inc && skey[i + cnt] == k) ++cnt;
    const int64_t e = group[i];
    if (e < 0 || e >= n_inc) return;
    const int lo = (int)(k / V), hi = (int)(k % V);
    e_lo[e] = lo;
    e_hi[e] = hi;
    e_f0[e] = (int)(order[i] / 3);
    e_f1[e] = cnt >= 2 ? (int)(order[i + 1] / 3) : -1;
    e_nf[e] = cnt;
    if (cnt == 1) {
        const int64_t s = order[i];
        if (s >= 0 && s < n_inc) bflag[s] = 1;
        if (lo >= 0 && lo < V) vbnd[lo] = 1;
        if (hi >= 0 && hi < V) vbnd[hi] = 1;
    }
}

__device__ __forceinline__ int md_opposite(const int* __restrict__ faces, int f, int lo, int hi)
{
    const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    if (a != lo && a != hi) return a;
    if (b != lo && b != hi) return b;
    if (c != lo && c != hi) return c;
    return -1;
}

// the checks of one end s of the edge (the other end is t): returns false when the collapse is refused; *has is set when a surviving
// face at s lies over the two opposite vertices
__device__ __forceinline__ bool md_check_end(int s, int t, int oa, int ob, const MdV& nb, const double* __restrict__ P,
                                             const int* __restrict__ faces, const int* __restrict__ offsets, const int* __restrict__ items,
                                             bool* has)
{
    const MdV ps = md_point(P, s);
    const int t0 = offsets[t], t1 = offsets[t + 1];
    for (int i = offsets[s]; i < offsets[s + 1]; ++i) {
        const int it = items[i];
        const int f = it / 3, c = it - 3 * f;
        const int v0 = faces[3 * f], v1 = faces[3 * f + 1], v2 = faces[3 * f + 2];
        if (v0 == t || v1 == t || v2 == t) continue;                       // a face of the edge: it goes
        const int w1 = c == 0 ? v1 : (c == 1 ? v2 : v0), w2 = c == 0 ? v2 : (c == 1 ? v0 : v1);
        if (ob >= 0 && ((w1 == oa && w2 == ob) || (w1 == ob && w2 == oa))) *has = true;
        for (int j = t0; j < t1; ++j) {                                     // link condition
            const int g = items[j] / 3;
            const int g0 = faces[3 * g], g1 = faces[3 * g + 1], g2 = faces[3 * g + 2];
            if (w1 != oa && w1 != ob && (g0 == w1 || g1 == w1 || g2 == w1)) return false;
            if (w2 != oa && w2 != ob && (g0 == w2 || g1 == w2 || g2 == w2)) return false;
        }
        const MdV p1 = md_point(P, w1), p2 = md_point(P, w2);
        const MdV n_old = md_cross(md_sub(p1, ps), md_sub(p2, ps));
        const MdV n_new = md_cross(md_sub(p1, nb), md_sub(p2, nb));
        if (!(md_dot(n_old, n_new) > 0.0)) return false;
    }
    return true;
}

// n_edges_m1[0] + 1 = the number of edges (the last entry of `group`); ekey must be filled with MD_KEY_INVALID on entry
__global__ void __launch_bounds__(MD_T) k_md_edge_eval(int cap, int V, int F, const int64_t* __restrict__ n_edges_m1, const double* __restrict__ P,
                                                       const double* __restrict__ Q, const int* __restrict__ faces,
                                                       const int* __restrict__ offsets, const int* __restrict__ items,
                                                       const int* __restrict__ e_lo, const int* __restrict__ e_hi, const int* __restrict__ e_f0,
                                                       const int* __restrict__ e_f1, const int* __restrict__ e_nf, const int* __restrict__ vbnd,
                                                       int64_t* __restrict__ ekey, double* __restrict__ vbar)
{
    const int e = blockIdx.x * MD_T + threadIdx.x;
    if (e >= cap || e > n_edges_m1[0]) return;
    const int lo = e_lo[e], hi = e_hi[e], nf = e_nf[e], f0 = e_f0[e], f1 = e_f1[e];
    if (nf > 2 || lo == hi || lo < 0 || lo >= V || hi < 0 || hi >= V || f0 < 0 || f0 >= F || f1 >= F) return;
    const int oa = md_opposite(faces, f0, lo, hi);
    const int ob = nf == 2 ? md_opposite(faces, f1, lo, hi) : -1;
    if (oa < 0 || (nf == 2 && (ob < 0 || oa == ob))) return;
    if (nf == 2 && vbnd[lo] && vbnd[hi]) return;
    const MdQ q = md_add(md_load(Q, lo), md_load(Q, hi));
    const MdV pl = md_point(P, lo), ph = md_point(P, hi);
    const MdV mid = {0.5 * (pl.x + ph.x), 0.5 * (pl.y + ph.y), 0.5 * (pl.z + ph.z)};
    const double c00 = q.q4 * q.q7 - q.q5 * q.q5, c01 = q.q2 * q.q5 - q.q1 * q.q7, c02 = q.q1 * q.q5 - q.q2 * q.q4;
    const double c11 = q.q0 * q.q7 - q.q2 * q.q2, c12 = q.q1 * q.q2 - q.q0 * q.q5, c22 = q.q0 * q.q4 - q.q1 * q.q1;
    const double det = q.q0 * c00 + q.q1 * c01 + q.q2 * c02;
    const double tr = q.q0 + q.q4 + q.q7;
    MdV nb = {0, 0, 0};
    double cost = 0;
    bool solved = false;
    if (fabs(det) > MD_DET_REL * tr * tr * tr) {
        nb.x = -((c00 * q.q3 + c01 * q.q6 + c02 * q.q8) / det);
        nb.y = -((c01 * q.q3 + c11 * q.q6 + c12 * q.q8) / det);
        nb.z = -((c02 * q.q3 + c12 * q.q6 + c22 * q.q8) / det);
        const MdV dm = md_sub(nb, mid), de = md_sub(ph, pl);
        if (md_dot(dm, dm) <= md_dot(de, de)) {
            solved = true;
            cost = md_cost(q, nb.x, nb.y, nb.z);
        }
    }
    if (!solved) {
        nb = pl;
        cost = md_cost(q, pl.x, pl.y, pl.z);
        const double ch = md_cost(q, ph.x, ph.y, ph.z);
        if (ch < cost) { cost = ch; nb = ph; }
        const double cm = md_cost(q, mid.x, mid.y, mid.z);
        if (cm < cost) { cost = cm; nb = mid; }
    }
    if (!md_finite(cost)) return;
    bool has_lo = false, has_hi = false;
    if (!md_check_end(lo, hi, oa, ob, nb, P, faces, offsets, items, &has_lo)) return;
    if (!md_check_end(hi, lo, oa, ob, nb, P, faces, offsets, items, &has_hi)) return;
    if (has_lo && has_hi) return;
    int64_t bits = __double_as_longlong(cost);
    if (bits < 0) bits ^= 0x7FFFFFFFFFFFFFFFll;
    ekey[e] = bits;
    double* o = vbar + 3 * (int64_t)e;
    o[0] = nb.x; o[1] = nb.y; o[2] = nb.z;
}

// ------------------------------------------------------------------------------------------------------------------- selection
__device__ __forceinline__ int64_t md_candidates(const int64_t* __restrict__ n_valid) { return (n_valid[0] + 3) / 4; }

// one selection pass.  A candidate is live while it has neither won nor died; it dies when one of its vertices is locked by the winner
// of an earlier pass.  claim[V] is all ones on entry of every pass; lock[V] and dead[cap] are zero on entry of the first.
__global__ void __launch_bounds__(MD_T) k_md_claim(int cap, int V, const int64_t* __restrict__ n_valid, const int64_t* __restrict__ order_e,
                                                   const int* __restrict__ e_lo, const int* __restrict__ e_hi, const int* __restrict__ faces,
                                                   const int* __restrict__ offsets, const int* __restrict__ items, const int* __restrict__ lock,
                                                   const int* __restrict__ win, uint8_t* __restrict__ dead,
                                                   unsigned long long* __restrict__ claim)
{
    const int r = blockIdx.x * MD_T + threadIdx.x;
    if (r >= cap || r >= md_candidates(n_valid) || win[r] || dead[r]) return;
    const int64_t e = order_e[r];
    if (e < 0 || e >= cap) return;
    for (int side = 0; side < 2; ++side) {
        const int s = side ? e_hi[e] : e_lo[e];
        for (int i = offsets[s]; i < offsets[s + 1]; ++i) {
            const int f = items[i] / 3;
            for (int c = 0; c < 3; ++c) {
                const int w = faces[3 * f + c];
                if (w >= 0 && w < V && lock[w]) { dead[r] = 1; return; }
            }
        }
    }
    for (int side = 0; side < 2; ++side) {
        const int s = side ? e_hi[e] : e_lo[e];
        for (int i = offsets[s]; i < offsets[s + 1]; ++i) {
            const int f = items[i] / 3;
            for (int c = 0; c < 3; ++c) {
                const int w = faces[3 * f + c];
                if (w >= 0 && w < V) atomicMin(&claim[w], (unsigned long long)r);
            }
        }
    }
}

// win[r] = the number of faces the collapse of the rank-r edge removes once it holds all its claims (win must be zero on entry of the
// first pass); a winner locks its vertices (no thread of this kernel reads lock)
__global__ void __launch_bounds__(MD_T) k_md_winners(int cap, int V, const int64_t* __restrict__ n_valid, const int64_t* __restrict__ order_e,
                                                     const int* __restrict__ e_lo, const int* __restrict__ e_hi, const int* __restrict__ e_nf,
                                                     const int* __restrict__ faces, const int* __restrict__ offsets, const int* __restrict__ items,
                                                     const unsigned long long* __restrict__ claim, const uint8_t* __restrict__ dead,
                                                     int* __restrict__ lock, int* __restrict__ win)
{
    const int r = blockIdx.x * MD_T + threadIdx.x;
    if (r >= cap || r >= md_candidates(n_valid) || win[r] || dead[r]) return;
    const int64_t e = order_e[r];
    if (e < 0 || e >= cap) return;
    bool ok = true;
    for (int side = 0; side < 2; ++side) {
        const int s = side ? e_hi[e] : e_lo[e];
        for (int i = offsets[s]; i < offsets[s + 1]; ++i) {
            const int f = items[i] / 3;
            for (int c = 0; c < 3; ++c) {
                const int w = faces[3 * f + c];
                if (w >= 0 && w < V && claim[w] != (unsigned long long)r) ok = false;
            }
        }
    }
    if (!ok) return;
    win[r] = e_nf[e];
    for (int side = 0; side < 2; ++side) {
        const int s = side ? e_hi[e] : e_lo[e];
        for (int i = offsets[s]; i < offsets[s + 1]; ++i) {
            const int f = items[i] / 3;
            for (int c = 0; c < 3; ++c) {
                const int w = faces[3 * f + c];
                if (w >= 0 && w < V) lock[w] = 1;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------- apply
// rename[V] must be the identity and vkeep[V] all ones on entry
__global__ void __launch_bounds__(MD_T) k_md_apply_edges(int cap, int V, const uint8_t* __restrict__ keep, const int64_t* __restrict__ order_e,
                                                         const int* __restrict__ e_lo, const int* __restrict__ e_hi, const double* __restrict__ vbar,
                                                         double* __restrict__ P, double* __restrict__ Q, int* __restrict__ rename,
                                                         int* __restrict__ vkeep)
{
    const int r = blockIdx.x * MD_T + threadIdx.x;
    if (r >= cap || !keep[r]) return;
    const int64_t e = order_e[r];
    if (e < 0 || e >= cap) return;
    const int u = e_lo[e], v = e_hi[e];
    if (u < 0 || u >= V || v < 0 || v >= V) return;
    const double* nb = vbar + 3 * e;
    double* p = P + 3 * (int64_t)u;
    p[0] = nb[0]; p[1] = nb[1]; p[2] = nb[2];
    md_store(Q, u, md_add(md_load(Q, u), md_load(Q, v)));
    rename[v] = u;
    vkeep[v] = 0;
}

// faces are renamed in place; fkeep[f] = the renamed face names three different vertices
__global__ void __launch_bounds__(MD_T) k_md_apply_faces(int F, int V, int* __restrict__ faces, const int* __restrict__ rename, int* __restrict__ fkeep)
{
    const int f = blockIdx.x * MD_T + threadIdx.x;
    if (f >= F) return;
    int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    if (a >= 0 && a < V) a = rename[a];
    if (b >= 0 && b < V) b = rename[b];
    if (c >= 0 && c < V) c = rename[c];
    faces[3 * f] = a; faces[3 * f + 1] = b; faces[3 * f + 2] = c;
    fkeep[f] = (a != b && b != c && a != c) ? 1 : 0;
}

// vpos / fpos: the inclusive scans of the keep flags
__global__ void __launch_bounds__(MD_T) k_md_compact_verts(int V, const int* __restrict__ vkeep, const int64_t* __restrict__ vpos,
                                                           const double* __restrict__ P, const double* __restrict__ Q, const float* __restrict__ vf,
                                                           double* __restrict__ P2, double* __restrict__ Q2, float* __restrict__ vf2)
{
    const int v = blockIdx.x * MD_T + threadIdx.x;
    if (v >= V || !vkeep[v]) return;
    const int64_t j = vpos[v] - 1;
    if (j < 0 || j >= V) return;
    if (P) { P2[3 * j] = P[3 * (int64_t)v]; P2[3 * j + 1] = P[3 * (int64_t)v + 1]; P2[3 * j + 2] = P[3 * (int64_t)v + 2]; }
    if (Q) md_store(Q2, j, md_load(Q, v));
    if (vf) { vf2[3 * j] = vf[3 * (int64_t)v]; vf2[3 * j + 1] = vf[3 * (int64_t)v + 1]; vf2[3 * j + 2] = vf[3 * (int64_t)v + 2]; }
}

__global__ void __launch_bounds__(MD_T) k_md_compact_faces(int F, int V, const int* __restrict__ fkeep, const int64_t* __restrict__ fpos,
                                                           const int64_t* __restrict__ vpos, const int* __restrict__ faces, int* __restrict__ faces2)
{
    const int f = blockIdx.x * MD_T + threadIdx.x;
    if (f >= F || !fkeep[f]) return;
    const int64_t j = fpos[f] - 1;
    if (j < 0 || j >= F) return;
    for (int c = 0; c < 3; ++c) {
        const int v = faces[3 * f + c];
        faces2[3 * j + c] = (v >= 0 && v < V) ? (int)(vpos[v] - 1) : -1;
    }
}

// ------------------------------------------------------------------------------------------------------------------- cleaning
// fkeep[f] &= the face names three different vertices
__global__ void __launch_bounds__(MD_T) k_md_clean_degenerate(int F, const int* __restrict__ faces, int* __restrict__ fkeep)
{
    const int f = blockIdx.x * MD_T + threadIdx.x;
    if (f >= F) return;
    const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    if (a == b || b == c || a == c) fkeep[f] = 0;
}

__device__ __forceinline__ void md_sort3(int& a, int& b, int& c)
{
    int t;
    if (a > b) { t = a; a = b; b = t; }
    if (b > c) { t = b; b = c; c = t; }
    if (a > b) { t = a; a = b; b = t; }
}

// perm[F]: the faces ordered by (sorted vertex triple, face id); a face whose triple equals its predecessor's is dropped
__global__ void __launch_bounds__(MD_T) k_md_clean_duplicate_faces(int F, const int* __restrict__ faces, const int64_t* __restrict__ perm,
                                                                   int* __restrict__ fkeep)
{
    const int i = blockIdx.x * MD_T + threadIdx.x;
    if (i >= F || i == 0) return;
    const int64_t f = perm[i], g = perm[i - 1];
    if (f < 0 || f >= F || g < 0 || g >= F) return;
    int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    int x = faces[3 * g], y = faces[3 * g + 1], z = faces[3 * g + 2];
    md_sort3(a, b, c);
    md_sort3(x, y, z);
    if (a == x && b == y && c == z) fkeep[f] = 0;
}

// perm[V]: the vertices ordered by (coordinate bits, vertex id); start[i] = 1 where sorted position i opens a run of bit-equal vertices
__global__ void __launch_bounds__(MD_T) k_md_clean_duplicate_verts(int V, const int32_t* __restrict__ bits, const int64_t* __restrict__ perm,
                                                                   int64_t* __restrict__ start)
{
    const int i = blockIdx.x * MD_T + threadIdx.x;
    if (i >= V) return;
    int64_t s = 1;
    if (i > 0) {
        const int64_t v = perm[i], u = perm[i - 1];
        if (v >= 0 && v < V && u >= 0 && u < V)
            s = (bits[3 * v] == bits[3 * u] && bits[3 * v + 1] == bits[3 * u + 1] && bits[3 * v + 2] == bits[3 * u + 2]) ? 0 : 1;
    }
    start[i] = s;
}

// one round of the non-manifold rule: every edge with more than two faces marks its smallest face (|(b - a) x (c - a)|^2 in float64,
// ties to the highest face id) for removal.  skey / order: the sorted incidences as for k_md_edge_build; fremove must be zero on entry.
__global__ void __launch_bounds__(MD_T) k_md_clean_nonmanifold(int n_inc, int V, const int64_t* __restrict__ skey, const int64_t* __restrict__ order,
                                                               const float* __restrict__ verts, const int* __restrict__ faces,
                                                               int* __restrict__ fremove)
{
    const int i = blockIdx.x * MD_T + threadIdx.x;
    if (i >= n_inc) return;
    const int64_t k = skey[i];
    if (i > 0 && skey[i - 1] == k) return;
    int cnt = 1;
    while (i + cnt < n_inc && skey[i + cnt] == k) ++cnt;
    if (cnt <= 2) return;
    double best = 0;
    int best_f = -1;
    for (int j = 0; j < cnt; ++j) {
        const int f = (int)(order[i + j] / 3);
        const int ia = faces[3 * f], ib = faces[3 * f + 1], ic = faces[3 * f + 2];
        if (ia < 0 || ia >= V || ib < 0 || ib >= V || ic < 0 || ic >= V) continue;
        const MdV pa = {(double)verts[3 * (int64_t)ia], (double)verts[3 * (int64_t)ia + 1], (double)verts[3 * (int64_t)ia + 2]};
        const MdV pb = {(double)verts[3 * (int64_t)ib], (double)verts[3 * (int64_t)ib + 1], (double)verts[3 * (int64_t)ib + 2]};
        const MdV pc = {(double)verts[3 * (int64_t)ic], (double)verts[3 * (int64_t)ic + 1], (double)verts[3 * (int64_t)ic + 2]};
        const MdV n = md_cross(md_sub(pb, pa), md_sub(pc, pa));
        const double a2 = md_dot(n, n);
        if (best_f < 0 || a2 < best || (a2 == best && f > best_f)) { best = a2; best_f = f; }
    }
    if (best_f >= 0) fremove[best_f] = 1;
}

__global__ void __launch_bounds__(MD_T) k_md_clean_mark_referenced(int F, int V, const int* __restrict__ faces, int* __restrict__ vref)
{
    const int f = blockIdx.x * MD_T + threadIdx.x;
    if (f >= F) return;
    for (int c = 0; c < 3; ++c) {
        const int v = faces[3 * f + c];
        if (v >= 0 && v < V) vref[v] = 1;
    }
}

static inline unsigned md_blocks(int64_t n) { return (unsigned)((n + MD_T - 1) / MD_T); }
static inline bool md_sizes_ok(int V, int F) { return V > 0 && F > 0 && (int64_t)3 * F < ((int64_t)1 << 31); }
#define MD_LAUNCHED(name) (hipGetLastError() == hipSuccess ? 0 : sgr_fail(SGR_E_HIP, name ": launch failed"))

}  // namespace

extern "C" {

int sgr_mesh_decimate_quadrics(int V, int F, const double* P, const int32_t* faces, const int32_t* vert_offsets, const int32_t* vert_items,
                               const uint8_t* boundary_flag, double boundary_weight, double* Q, void* stream)
{
    if (!md_sizes_ok(V, F)) return sgr_fail(SGR_E_INVALID, "mesh_decimate_quadrics: V and F must be positive and 3 F < 2^31");
    if (!P || !faces || !vert_offsets || !vert_items || !boundary_flag || !Q) return sgr_fail(SGR_E_INVALID, "mesh_decimate_quadrics: null pointer");
    hipLaunchKernelGGL(k_md_vertex_quadrics, dim3(md_blocks(V)), dim3(MD_T), 0, (hipStream_t)stream, V, F, P, faces, vert_offsets, vert_items,
                       boundary_flag, boundary_weight, Q);
    return MD_LAUNCHED("mesh_decimate_quadrics");
}

int sgr_mesh_decimate_edges(int V, int F, const int64_t* sorted_keys, const int64_t* sorted_incidence, const int64_t* sorted_edge,
                            int32_t* e_lo, int32_t* e_hi, int32_t* e_f0, int32_t* e_f1, int32_t* e_nf, uint8_t* boundary_flag,
                            int32_t* vert_boundary, void* stream)
{
    if (!md_sizes_ok(V, F)) return sgr_fail(SGR_E_INVALID, "mesh_decimate_edges: V and F must be positive and 3 F < 2^31");
    if (!sorted_keys || !sorted_incidence || !sorted_edge || !e_lo || !e_hi || !e_f0 || !e_f1 || !e_nf || !boundary_flag || !vert_boundary)
        return sgr_fail(SGR_E_INVALID, "mesh_decimate_edges: null pointer");
    hipLaunchKernelGGL(k_md_edge_build, dim3(md_blocks(3 * (int64_t)F)), dim3(MD_T), 0, (hipStream_t)stream, 3 * F, V, sorted_keys,
                       sorted_incidence, sorted_edge, e_lo, e_hi, e_f0, e_f1, e_nf, boundary_flag, vert_boundary);
    return MD_LAUNCHED("mesh_decimate_edges");
}

int sgr_mesh_decimate_eval(int V, int F, const int64_t* last_edge, const double* P, const double* Q, const int32_t* faces,
                           const int32_t* vert_offsets, const int32_t* vert_items, const int32_t* e_lo, const int32_t* e_hi,
                           const int32_t* e_f0, const int32_t* e_f1, const int32_t* e_nf, const int32_t* vert_boundary, int64_t* edge_key,
                           double* edge_pos, void* stream)
{
    if (!md_sizes_ok(V, F)) return sgr_fail(SGR_E_INVALID, "mesh_decimate_eval: V and F must be positive and 3 F < 2^31");
    if (!last_edge || !P || !Q || !faces || !vert_offsets || !vert_items || !e_lo || !e_hi || !e_f0 || !e_f1 || !e_nf || !vert_boundary ||
        !edge_key || !edge_pos)
        return sgr_fail(SGR_E_INVALID, "mesh_decimate_eval: null pointer");
    hipLaunchKernelGGL(k_md_edge_eval, dim3(md_blocks(3 * (int64_t)F)), dim3(MD_T), 0, (hipStream_t)stream, 3 * F, V, F, last_edge, P, Q, faces,
                       vert_offsets, vert_items, e_lo, e_hi, e_f0, e_f1, e_nf, vert_boundary, edge_key, edge_pos);
    return MD_LAUNCHED("mesh_decimate_eval");
}

int sgr_mesh_decimate_select(int V, int F, const int64_t* n_valid, const int64_t* edge_order, const int32_t* e_lo, const int32_t* e_hi,
                             const int32_t* e_nf, const int32_t* faces, const int32_t* vert_offsets, const int32_t* vert_items,
                             int64_t* claim, int32_t* lock, uint8_t* dead, int32_t* win, void* stream)
{
    if (!md_sizes_ok(V, F)) return sgr_fail(SGR_E_INVALID, "mesh_decimate_select: V and F must be positive and 3 F < 2^31");
    if (!n_valid || !edge_order || !e_lo || !e_hi || !e_nf || !faces || !vert_offsets || !vert_items || !claim || !lock || !dead || !win)
        return sgr_fail(SGR_E_INVALID, "mesh_decimate_select: null pointer");
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* cl = reinterpret_cast<unsigned long long*>(claim);
    for (int pass = 0; pass < SGR_MESH_DECIMATE_PASSES; ++pass) {
        if (hipMemsetAsync(claim, 0xFF, (size_t)V * 8, st) != hipSuccess) return sgr_fail(SGR_E_HIP, "mesh_decimate_select: memset failed");
        hipLaunchKernelGGL(k_md_claim, dim3(md_blocks(3 * (int64_t)F)), dim3(MD_T), 0, st, 3 * F, V, n_valid, edge_order, e_lo, e_hi, faces,
                           vert_offsets, vert_items, lock, win, dead, cl);
        hipLaunchKernelGGL(k_md_winners, dim3(md_blocks(3 * (int64_t)F)), dim3(MD_T), 0, st, 3 * F, V, n_valid, edge_order, e_lo, e_hi, e_nf,
                           faces, vert_offsets, vert_items, cl, dead, lock, win);
    }
    return MD_LAUNCHED("mesh_decimate_select");
}

int sgr_mesh_decimate_apply(int V, int F, const uint8_t* keep, const int64_t* edge_order, const int32_t* e_lo, const int32_t* e_hi,
                            const double* edge_pos, double* P, double* Q, int32_t* faces, int32_t* rename, int32_t* vert_keep,
                            int32_t* face_keep, void* stream)
{
    if (!md_sizes_ok(V, F)) return sgr_fail(SGR_E_INVALID, "mesh_decimate_apply: V and F must be positive and 3 F < 2^31");
    if (!keep || !edge_order || !e_lo || !e_hi || !edge_pos || !P || !Q || !faces || !rename || !vert_keep || !face_keep)
        return sgr_fail(SGR_E_INVALID, "mesh_decimate_apply: null pointer");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_md_apply_edges, dim3(md_blocks(3 * (int64_t)F)), dim3(MD_T), 0, st, 3 * F, V, keep, edge_order, e_lo, e_hi, edge_pos, P, Q,
                       rename, vert_keep);
    hipLaunchKernelGGL(k_md_apply_faces, dim3(md_blocks(F)), dim3(MD_T), 0, st, F, V, faces, rename, face_keep);
    return MD_LAUNCHED("mesh_decimate_apply");
}

int sgr_mesh_decimate_compact(int V, int F, const int32_t* vert_keep, const int64_t* vert_pos, const int32_t* face_keep, const int64_t* face_pos,
                              const double* P, const double* Q, const float* verts, const int32_t* faces, double* P_out, double* Q_out,
                              float* verts_out, int32_t* faces_out, void* stream)
{
    if (!md_sizes_ok(V, F)) return sgr_fail(SGR_E_INVALID, "mesh_decimate_compact: V and F must be positive and 3 F < 2^31");
    if (!vert_keep || !vert_pos || !face_keep || !face_pos || !faces || !faces_out || (P && !P_out) || (Q && !Q_out) || (verts && !verts_out))
        return sgr_fail(SGR_E_INVALID, "mesh_decimate_compact: null pointer");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_md_compact_verts, dim3(md_blocks(V)), dim3(MD_T), 0, st, V, vert_keep, vert_pos, P, Q, verts, P_out, Q_out, verts_out);
    hipLaunchKernelGGL(k_md_compact_faces, dim3(md_blocks(F)), dim3(MD_T), 0, st, F, V, face_keep, face_pos, vert_pos, faces, faces_out);
    return MD_LAUNCHED("mesh_decimate_compact");
}

int sgr_mesh_clean_degenerate(int F, const int32_t* faces, int32_t* face_keep, void* stream)
{
    if (F <= 0 || !faces || !face_keep) return sgr_fail(SGR_E_INVALID, "mesh_clean_degenerate: F must be positive, no null pointer");
    hipLaunchKernelGGL(k_md_clean_degenerate, dim3(md_blocks(F)), dim3(MD_T), 0, (hipStream_t)stream, F, faces, face_keep);
    return MD_LAUNCHED("mesh_clean_degenerate");
}

int sgr_mesh_clean_duplicate_faces(int F, const int32_t* faces, const int64_t* perm, int32_t* face_keep, void* stream)
{
    if (F <= 0 || !faces || !perm || !face_keep) return sgr_fail(SGR_E_INVALID, "mesh_clean_duplicate_faces: F must be positive, no null pointer");
    hipLaunchKernelGGL(k_md_clean_duplicate_faces, dim3(md_blocks(F)), dim3(MD_T), 0, (hipStream_t)stream, F, faces, perm, face_keep);
    return MD_LAUNCHED("mesh_clean_duplicate_faces");
}

int sgr_mesh_clean_duplicate_verts(int V, const float* verts, const int64_t* perm, int64_t* run_start, void* stream)
{
    if (V <= 0 || !verts || !perm || !run_start) return sgr_fail(SGR_E_INVALID, "mesh_clean_duplicate_verts: V must be positive, no null pointer");
    hipLaunchKernelGGL(k_md_clean_duplicate_verts, dim3(md_blocks(V)), dim3(MD_T), 0, (hipStream_t)stream, V,
                       reinterpret_cast<const int32_t*>(verts), perm, run_start);
    return MD_LAUNCHED("mesh_clean_duplicate_verts");
}

int sgr_mesh_clean_nonmanifold(int V, int F, const int64_t* sorted_keys, const int64_t* sorted_incidence, const float* verts,
                               const int32_t* faces, int32_t* face_remove, void* stream)
{
    if (!md_sizes_ok(V, F)) return sgr_fail(SGR_E_INVALID, "mesh_clean_nonmanifold: V and F must be positive and 3 F < 2^31");
    if (!sorted_keys || !sorted_incidence || !verts || !faces || !face_remove) return sgr_fail(SGR_E_INVALID, "mesh_clean_nonmanifold: null pointer");
    hipLaunchKernelGGL(k_md_clean_nonmanifold, dim3(md_blocks(3 * (int64_t)F)), dim3(MD_T), 0, (hipStream_t)stream, 3 * F, V, sorted_keys,
                       sorted_incidence, verts, faces, face_remove);
    return MD_LAUNCHED("mesh_clean_nonmanifold");
}

int sgr_mesh_clean_referenced(int V, int F, const int32_t* faces, int32_t* vert_referenced, void* stream)
{
    if (!md_sizes_ok(V, F)) return sgr_fail(SGR_E_INVALID, "mesh_clean_referenced: V and F must be positive and 3 F < 2^31");
    if (!faces || !vert_referenced) return sgr_fail(SGR_E_INVALID, "mesh_clean_referenced: null pointer");
    hipLaunchKernelGGL(k_md_clean_mark_referenced, dim3(md_blocks(F)), dim3(MD_T), 0, (hipStream_t)stream, F, V, faces, vert_referenced);
    return MD_LAUNCHED("mesh_clean_referenced");
}

}  // extern "C"
