// mesh_postprocess.hip -- the border-face peel of the refined-mesh export (sugar_extractors/refined_mesh.py:133-147).
//
// The rule.  Face (a, b, c) has three slots, s = 3 f + k, carrying the unordered vertex pairs {a,b}, {b,c}, {c,a} (k = 0, 1, 2).  With
// a live set of faces, the live count of a pair is the number of SLOTS of live faces that carry it: a face (i, j, j) carries {i,j}
// twice, two copies of one face make each other's pairs count 2, an edge with three faces counts 3.  One iteration: a live face stays
// live if and only if all three of its pairs have live count >= 2; every count is taken before any face of that iteration is removed.
// `iterations` such steps run, with no early exit; an empty set stays empty.  The reference asks the same question with a k-NN over
// the float pairs (second-nearest squared distance < 0.01); the two agree whenever vertex ids are below 2^24, above which the
// reference's float cast collides.  Here everything is integer arithmetic: the result is exact and the same bytes on every run.
//
// The form: per-edge gather, two launches per iteration, no atomics and nothing to clear.
//   k_peel_count   one lane per edge e sums live[item / 3] over its slot list items[offsets[e] .. offsets[e+1]) and stores the count,
//                  saturated at 255, as one byte.
//   k_peel_test    one lane per face: live[f] &= count[slot_edge[3f]] >= 2 && ... for its three slots.
// The second launch starts after the first has finished (stream order), so the decisions of an iteration read counts taken from the
// live set at its start, and the mask can be updated in place.
// Why not integer atomicAdd into a cleared counter array: that is 3F scattered one-dword atomics plus a clear per iteration.  On this
// chip global atomics execute at the memory side, uncached, and a wave instruction whose lanes each hit another row runs an order of
// magnitude below the rate of a contiguous one; the gather reads the same scattered bytes with plain loads that the L2 serves (the
// mask is F bytes, the counts E bytes: both stay resident across iterations), reads the slot lists contiguously (the slots of an edge
// are neighbours in `items`, the three edge ids of a face are neighbours in `slot_edge`), and its result cannot depend on arrival
// order.  The edge -> slots list depends on the faces alone and is built once, by sugar_amd/mesh_postprocess.py.
//
// Indices are validated in the kernels: an item outside [0, 3F) adds nothing, an edge id outside [0, E) counts as 0 (the face dies),
// an offsets pair that is not ascending inside [0, 3F] gives an empty list.  Nothing reads or writes out of bounds.
#include "../../include/sugar_raster.h"
#include "sgr_common.h"

namespace {

__global__ void __launch_bounds__(256) k_peel_count(int E, int n_slots, const int32_t* __restrict__ offsets, const int32_t* __restrict__ items,
                                                    const uint8_t* __restrict__ live, uint8_t* __restrict__ count)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const int b = max(offsets[e], 0), end = min(offsets[e + 1], n_slots);
    int c = 0;
    for (int i = b; i < end; i++) {
        const int s = items[i];
        if (s >= 0 && s < n_slots) c += live[s / 3] != 0;
    }
    count[e] = (uint8_t)min(c, 255);
}

__global__ void __launch_bounds__(256) k_peel_test(int F, int E, const int32_t* __restrict__ slot_edge, const uint8_t* __restrict__ count,
                                                   uint8_t* __restrict__ live)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    if (!live[f]) return;
    bool keep = true;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int e = slot_edge[3 * (int64_t)f + k];
        keep = keep && e >= 0 && e < E && count[e] >= 2;
    }
    live[f] = keep ? 1 : 0;
}

const int64_t kMaxSlots = (int64_t)1 << 30;   // 3F: every slot index, and the launch grids, stay well below 2^31

}  // namespace

extern "C" {

size_t sgr_mesh_peel_border_scratch_bytes(int E) { return E > 0 ? sgr_align((size_t)E) : 0; }

int sgr_mesh_peel_border(int F, int E, const int32_t* slot_edge, const int32_t* edge_offsets, const int32_t* edge_items, int iterations,
                         uint8_t* live, void* scratch, void* stream)
{
    if (F < 0 || iterations < 0) return sgr_fail(SGR_E_INVALID, "mesh_peel_border: F and iterations must not be negative");
    if (F == 0 || iterations == 0) return 0;
    if ((int64_t)F * 3 >= kMaxSlots) return sgr_fail(SGR_E_INVALID, "mesh_peel_border: 3 F must be below 2^30");
    if (E <= 0 || (int64_t)E > (int64_t)F * 3) return sgr_fail(SGR_E_INVALID, "mesh_peel_border: E must be in 1 .. 3 F");
    if (!slot_edge || !edge_offsets || !edge_items || !live || !scratch)
        return sgr_fail(SGR_E_INVALID, "mesh_peel_border: null pointer");
    uint8_t* count = reinterpret_cast<uint8_t*>(scratch);
    const dim3 grid_e((unsigned)((E + 255) / 256)), grid_f((unsigned)((F + 255) / 256));
    for (int it = 0; it < iterations; it++) {
        hipLaunchKernelGGL(k_peel_count, grid_e, dim3(256), 0, (hipStream_t)stream, E, 3 * F, edge_offsets, edge_items, live, count);
        hipLaunchKernelGGL(k_peel_test, grid_f, dim3(256), 0, (hipStream_t)stream, F, E, slot_edge, count, live);
    }
    return hipGetLastError() == hipSuccess ? 0 : sgr_fail(SGR_E_HIP, "mesh_peel_border: launch failed");
}

}  // extern "C"
