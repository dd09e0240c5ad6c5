"""Mesh simplification (quadric-error edge collapse in parallel rounds) and mesh cleaning on the HIP kernels of csrc/mesh_decimate.hip
(C ABI: sgr_mesh_decimate_* / sgr_mesh_clean_* in include/sugar_raster.h): what the reference does with open3d between extraction and
refinement -- `simplify_quadric_decimation(decimation_target)` and the `remove_*` calls of sugar_extractors/coarse_mesh.py:586-605,
:722-742 -- as native code.  This is not an open3d stand-in: there is no `open3d` module here.

  decimate(verts, faces, target_faces, boundary_weight=1.0) -> (verts[V',3] float32, faces[F',3] int64, info)
  clean(verts, faces, degenerate=True, duplicated_triangles=True, duplicated_vertices=True, non_manifold_edges=True)
      -> (verts, faces, vertex_map[V] int64: the new id of every input vertex, -1 for a removed one)

The rules are stated in full at the top of the kernel file and restated serially in tests/decimate_restatement.py; the kernels match
that restatement bit for bit, and two runs give identical bits.  In short, per round: the edges and the vertex -> face lists are
rebuilt (torch sorts and scans), every edge gets a cost, a position and a validity verdict (one kernel), the keys are sorted, the lowest
quarter of the valid edges claim their neighbourhoods with integer atomicMin (four passes) and the edges that hold all their claims collapse.  Winners
are kept in key order while F - (faces already removed this round) > target, so the result has target - 2 < F <= target faces whenever
enough valid collapses exist; otherwise the loop ends in the first round without a winner, or after `round_limit(F, target)` rounds.

Host synchronisation in `decimate`: one read before the first round (the check that every face names vertices in [0, V)), then exactly
ONE device-to-host read per round -- `counts.tolist()` in `_round`, the triple (vertices, faces, collapses) that sizes the next round.
`clean` reads one count per pass (and one per round of the non-manifold rule).  There is no CPU path: CPU tensors raise."""
from __future__ import annotations

import torch

from ._call import call, csr, need_gpu, ptr

KEY_INVALID = 2 ** 63 - 1


def _shapes(what, verts, faces):
    if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"{what}: verts must be [V,3] and faces [F,3]")
    if faces.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{what}: faces must be int32 or int64")
    if 3 * int(faces.shape[0]) >= 2 ** 31 or int(verts.shape[0]) >= 2 ** 31:
        raise ValueError(f"{what}: V and 3 F must stay below 2^31")


def round_limit(n_faces: int, target: int) -> int:
    """8 ceil(log2(F / target)) + 32 rounds (target 0 counts as 1)"""
    t, k = max(int(target), 1), 0
    while (t << k) < int(n_faces):
        k += 1
    return 8 * k + 32


def _sorted_incidences(faces32, V):
    """(sorted keys lo * V + hi, the incidence 3 f + k of every sorted position): edge k of face (a, b, c) is (b, c), (c, a), (a, b)"""
    f = faces32.to(torch.int64)
    e0 = torch.stack([f[:, 1], f[:, 2], f[:, 0]], dim=1).reshape(-1)
    e1 = torch.stack([f[:, 2], f[:, 0], f[:, 1]], dim=1).reshape(-1)
    key = torch.minimum(e0, e1) * V + torch.maximum(e0, e1)
    return torch.sort(key, stable=True)


class _Edges:
    """the edge records of one faces tensor (every array has 3 F entries; the first n_edges are used)"""

    def __init__(self, faces32, V):
        dev = faces32.device
        F_ = int(faces32.shape[0])
        n = 3 * F_
        skey, order = _sorted_incidences(faces32, V)
        new = torch.ones(n, dtype=torch.int64, device=dev)
        new[1:] = (skey[1:] != skey[:-1]).to(torch.int64)
        group = torch.cumsum(new, 0) - 1
        self.last_edge = group[n - 1:]                      # device scalar: n_edges - 1
        i32 = lambda: torch.empty(n, dtype=torch.int32, device=dev)
        self.lo, self.hi, self.f0, self.f1, self.nf = i32(), i32(), i32(), i32(), i32()
        self.bflag = torch.zeros(n, dtype=torch.uint8, device=dev)
        self.vbnd = torch.zeros(V, dtype=torch.int32, device=dev)
        call("sgr_mesh_decimate_edges", dev, V, F_, ptr(skey), ptr(order), ptr(group), ptr(self.lo), ptr(self.hi), ptr(self.f0),
             ptr(self.f1), ptr(self.nf), ptr(self.bflag), ptr(self.vbnd))


def _round(P, Q, faces32, target):
    """one round of collapses; returns (P, Q, faces, n_collapsed).  The one host read of the round is `counts.tolist()`."""
    dev = P.device
    V, F_ = int(P.shape[0]), int(faces32.shape[0])
    n = 3 * F_
    ed = _Edges(faces32, V)
    offsets, items = csr(faces32, V)
    ekey = torch.full((n,), KEY_INVALID, dtype=torch.int64, device=dev)
    epos = torch.empty(n, 3, dtype=torch.float64, device=dev)
    call("sgr_mesh_decimate_eval", dev, V, F_, ptr(ed.last_edge), ptr(P), ptr(Q), ptr(faces32), ptr(offsets), ptr(items), ptr(ed.lo),
         ptr(ed.hi), ptr(ed.f0), ptr(ed.f1), ptr(ed.nf), ptr(ed.vbnd), ptr(ekey), ptr(epos))
    order_e = torch.sort(ekey, stable=True).indices
    n_valid = (ekey != KEY_INVALID).sum().reshape(1)
    claim = torch.empty(V, dtype=torch.int64, device=dev)
    lock = torch.zeros(V, dtype=torch.int32, device=dev)
    dead = torch.zeros(n, dtype=torch.uint8, device=dev)
    win = torch.zeros(n, dtype=torch.int32, device=dev)
    call("sgr_mesh_decimate_select", dev, V, F_, ptr(n_valid), ptr(order_e), ptr(ed.lo), ptr(ed.hi), ptr(ed.nf), ptr(faces32), ptr(offsets),
         ptr(items), ptr(claim), ptr(lock), ptr(dead), ptr(win))
    removed = win.to(torch.int64)
    before = torch.cumsum(removed, 0) - removed             # faces removed by the winners of lower rank
    keep = (win > 0) & ((F_ - before) > int(target))
    keep8 = keep.to(torch.uint8)
    rename = torch.arange(V, dtype=torch.int32, device=dev)
    vkeep = torch.ones(V, dtype=torch.int32, device=dev)
    fkeep = torch.empty(F_, dtype=torch.int32, device=dev)
    call("sgr_mesh_decimate_apply", dev, V, F_, ptr(keep8), ptr(order_e), ptr(ed.lo), ptr(ed.hi), ptr(epos), ptr(P), ptr(Q), ptr(faces32),
         ptr(rename), ptr(vkeep), ptr(fkeep))
    vpos, fpos = torch.cumsum(vkeep, 0, dtype=torch.int64), torch.cumsum(fkeep, 0, dtype=torch.int64)
    P2, Q2, faces2 = torch.empty_like(P), torch.empty_like(Q), torch.empty_like(faces32)
    call("sgr_mesh_decimate_compact", dev, V, F_, ptr(vkeep), ptr(vpos), ptr(fkeep), ptr(fpos), ptr(P), ptr(Q), None, ptr(faces32), ptr(P2),
         ptr(Q2), None, ptr(faces2))
    counts = torch.stack([vpos[-1], fpos[-1], keep.sum()])
    n_verts, n_faces, n_collapsed = counts.tolist()          # the one device-to-host read of the round
    return P2[:n_verts], Q2[:n_verts], faces2[:n_faces], n_collapsed


def decimate(verts: torch.Tensor, faces: torch.Tensor, target_faces: int, boundary_weight: float = 1.0):
    """Collapses edges in order of quadric error until at most `target_faces` faces remain.  verts[V,3] (float32 is used), faces[F,3]
    int32 / int64 on a ROCm device; the mesh should be clean (see `clean`): faces with a repeated index and edges with more than two
    faces are never collapsed.  Returns (verts float32, faces int64, info) with info = dict(rounds, faces, target, target_met,
    round_limit).  A target of at least F returns the input (as float32 / int64) unchanged."""
    need_gpu("decimate", verts=verts, faces=faces)
    _shapes("decimate", verts, faces)
    target = int(target_faces)
    if target < 0:
        raise ValueError("decimate: target_faces must not be negative")
    v32 = verts.detach().to(torch.float32).contiguous()
    f64 = faces.detach().to(torch.int64).contiguous()
    V, F_ = int(v32.shape[0]), int(f64.shape[0])
    limit = round_limit(F_, target)
    info = dict(rounds=0, faces=F_, target=target, target_met=F_ <= target, round_limit=limit)
    if F_ <= target or F_ == 0 or V == 0:
        return v32, f64, info
    if bool(((f64 < 0) | (f64 >= V)).any()):                 # the read before the first round
        raise ValueError(f"decimate: a face names a vertex outside [0, {V})")
    dev = v32.device
    faces32 = f64.to(torch.int32)
    centre = 0.5 * (v32.min(dim=0).values.to(torch.float64) + v32.max(dim=0).values.to(torch.float64))
    P = (v32.to(torch.float64) - centre).contiguous()
    ed = _Edges(faces32, V)
    offsets, items = csr(faces32, V)
    Q = torch.empty(V, 10, dtype=torch.float64, device=dev)
    call("sgr_mesh_decimate_quadrics", dev, V, F_, ptr(P), ptr(faces32), ptr(offsets), ptr(items), ptr(ed.bflag), float(boundary_weight),
         ptr(Q))
    del ed, offsets, items
    rounds = 0
    while faces32.shape[0] > target and rounds < limit:
        P, Q, faces32, n_collapsed = _round(P, Q, faces32, target)
        rounds += 1
        if n_collapsed == 0 or faces32.shape[0] == 0:
            break
    F_out = int(faces32.shape[0])
    info.update(rounds=rounds, faces=F_out, target_met=F_out <= target)
    return (P + centre).to(torch.float32), faces32.to(torch.int64), info


# ---------------------------------------------------------------------------------------------------------------------- cleaning
def _lexsort_rows(rows):
    """the permutation ordering the rows of an integer [N,3] tensor by (column 0, 1, 2, row id)"""
    perm = torch.arange(rows.shape[0], device=rows.device)
    for col in (2, 1, 0):
        perm = perm[torch.sort(rows[perm, col], stable=True).indices]
    return perm.contiguous()


def clean(verts: torch.Tensor, faces: torch.Tensor, degenerate: bool = True, duplicated_triangles: bool = True,
          duplicated_vertices: bool = True, non_manifold_edges: bool = True):
    """The reference's cleaning calls, in its order (coarse_mesh.py:598-602), each with a deterministic rule:
      degenerate            faces that repeat an index are removed;
      duplicated_triangles  of the faces over one vertex set (in any order or orientation) the lowest face id survives;
      duplicated_vertices   of the vertices with bit-equal coordinates the lowest id survives, faces are renamed;
      non_manifold_edges    while an edge has more than two faces, every such edge removes its smallest face
                            (|(b - a) x (c - a)|^2 in float64; ties to the highest face id), in rounds;
    then vertices that no face names are removed (always).  Faces and vertices keep their relative order.
    Returns (verts float32, faces int64, vertex_map int64[V])."""
    need_gpu("clean", verts=verts, faces=faces)
    _shapes("clean", verts, faces)
    v = verts.detach().to(torch.float32).contiguous()
    f = faces.detach().to(torch.int32).contiguous()
    dev = v.device
    V = int(v.shape[0])
    vmap = torch.arange(V, dtype=torch.int64, device=dev)
    if V and f.shape[0] and bool(((f < 0) | (f >= V)).any()):
        raise ValueError(f"clean: a face names a vertex outside [0, {V})")

    def ones(n):
        return torch.ones(n, dtype=torch.int32, device=dev)

    if degenerate and f.shape[0]:
        keep = ones(f.shape[0])
        call("sgr_mesh_clean_degenerate", dev, int(f.shape[0]), ptr(f), ptr(keep))
        f = f[keep.bool()].contiguous()
    if duplicated_triangles and f.shape[0]:
        perm = _lexsort_rows(torch.sort(f, dim=1).values)
        keep = ones(f.shape[0])
        call("sgr_mesh_clean_duplicate_faces", dev, int(f.shape[0]), ptr(f), ptr(perm), ptr(keep))
        f = f[keep.bool()].contiguous()
    if duplicated_vertices and V:
        perm = _lexsort_rows(v.view(torch.int32))
        start = torch.empty(V, dtype=torch.int64, device=dev)
        call("sgr_mesh_clean_duplicate_verts", dev, V, ptr(v), ptr(perm), ptr(start))
        pos = torch.arange(V, device=dev)
        leader = torch.cummax(torch.where(start == 1, pos, torch.zeros_like(pos)), 0).values
        vmap = torch.empty(V, dtype=torch.int64, device=dev)
        vmap[perm] = perm[leader]
        if f.shape[0]:
            f = vmap[f.to(torch.int64)].to(torch.int32).contiguous()
    while non_manifold_edges and f.shape[0] and V:
        skey, order = _sorted_incidences(f, V)
        remove = torch.zeros(f.shape[0], dtype=torch.int32, device=dev)
        call("sgr_mesh_clean_nonmanifold", dev, V, int(f.shape[0]), ptr(skey), ptr(order), ptr(v), ptr(f), ptr(remove))
        if int(remove.sum()) == 0:
            break
        f = f[remove == 0].contiguous()
    F_ = int(f.shape[0])
    if V == 0 or F_ == 0:
        return v[:0], torch.zeros(0, 3, dtype=torch.int64, device=dev), torch.full((V,), -1, dtype=torch.int64, device=dev)
    ref = torch.zeros(V, dtype=torch.int32, device=dev)
    call("sgr_mesh_clean_referenced", dev, V, F_, ptr(f), ptr(ref))
    vpos = torch.cumsum(ref, 0, dtype=torch.int64)
    fkeep = ones(F_)
    fpos = torch.cumsum(fkeep, 0, dtype=torch.int64)
    v2, f2 = torch.empty_like(v), torch.empty_like(f)
    call("sgr_mesh_decimate_compact", dev, V, F_, ptr(ref), ptr(vpos), ptr(fkeep), ptr(fpos), None, None, ptr(v), ptr(f), None, None,
         ptr(v2), ptr(f2))
    n_verts = int(vpos[-1])
    new_id = torch.where(ref > 0, vpos - 1, torch.full_like(vpos, -1))
    return v2[:n_verts], f2.to(torch.int64), new_id[vmap]


def remove_vertices_by_mask(verts: torch.Tensor, faces: torch.Tensor, mask: torch.Tensor, *per_vertex, unreferenced: bool = False):
    """open3d's `TriangleMesh.remove_vertices_by_mask` (coarse_mesh.py:395) with a stated rule: every vertex with mask[v] set is
    removed, and with it every face that names one; `unreferenced=True` then also removes every vertex that no surviving face names.
    The surviving vertices and faces keep their relative order (a stable compaction; faces are renumbered).  `per_vertex`: any number
    of [V, ...] tensors, compacted like the vertices.  Returns (verts float32 [V',3], faces int64 [F',3], *per_vertex).
    ONE device-to-host read: the pair (V', F'), which sizes the outputs.  A face naming a vertex outside [0, V) is removed."""
    need_gpu("remove_vertices_by_mask", verts=verts, faces=faces, mask=mask)
    _shapes("remove_vertices_by_mask", verts, faces)
    V, F_ = int(verts.shape[0]), int(faces.shape[0])
    if mask.dim() != 1 or int(mask.shape[0]) != V:
        raise ValueError("remove_vertices_by_mask: mask must be [V]")
    for a in per_vertex:
        if not torch.is_tensor(a) or not a.is_cuda or a.dim() < 1 or int(a.shape[0]) != V:
            raise ValueError("remove_vertices_by_mask: every per-vertex tensor must be a device tensor with V rows")
    v = verts.detach().to(torch.float32).contiguous()
    dev = v.device
    gone = mask.detach().to(device=dev) != 0
    if V == 0:
        return (v, torch.zeros(0, 3, dtype=torch.int64, device=dev), *per_vertex)
    if F_ == 0:
        ids = torch.zeros(0, dtype=torch.int64, device=dev) if unreferenced else (~gone).nonzero(as_tuple=True)[0]   # (the one read)
        return (v[ids], torch.zeros(0, 3, dtype=torch.int64, device=dev), *(a[ids] for a in per_vertex))
    f = faces.detach().to(torch.int32).contiguous()
    inside = ((f >= 0) & (f < V)).all(dim=1)
    fkeep_b = inside & ~gone[f.clamp(0, V - 1).to(torch.int64)].any(dim=1)
    fkeep = fkeep_b.to(torch.int32)
    if unreferenced:
        vkeep = torch.zeros(V, dtype=torch.int32, device=dev)
        marked = torch.where(fkeep_b[:, None], f, torch.full_like(f, -1)).contiguous()    # (the kernel skips an index outside [0, V))
        call("sgr_mesh_clean_referenced", dev, V, F_, ptr(marked), ptr(vkeep))
        vkeep = vkeep * (~gone).to(torch.int32)
    else:
        vkeep = (~gone).to(torch.int32)
    vpos, fpos = torch.cumsum(vkeep, 0, dtype=torch.int64), torch.cumsum(fkeep, 0, dtype=torch.int64)
    v2, f2 = torch.empty_like(v), torch.empty_like(f)
    call("sgr_mesh_decimate_compact", dev, V, F_, ptr(vkeep), ptr(vpos), ptr(fkeep), ptr(fpos), None, None, ptr(v), ptr(f), None, None,
         ptr(v2), ptr(f2))
    src = torch.empty(V + 1, dtype=torch.int64, device=dev)       # src[j] = the input id of output vertex j (slot V: the removed ones)
    src.scatter_(0, torch.where(vkeep > 0, vpos - 1, torch.full_like(vpos, V)), torch.arange(V, device=dev))
    n_verts, n_faces = torch.stack([vpos[-1], fpos[-1]]).tolist()  # the one device-to-host read
    return (v2[:n_verts], f2[:n_faces].to(torch.int64), *(a[src[:n_verts]] for a in per_vertex))
