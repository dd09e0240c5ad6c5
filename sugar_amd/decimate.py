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

import ctypes as C

import torch

from . import _lib

KEY_INVALID = 2 ** 63 - 1


def _vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _check(rc, name):
    if rc < 0:
        raise RuntimeError(f"{name} failed ({rc}): {_lib.last_error()}")


def _need_gpu(what, **tensors):
    for name, t in tensors.items():
        if not torch.is_tensor(t) or not t.is_cuda:
            raise RuntimeError(f"{what}: {name} must be a tensor on a ROCm device; there is no CPU fallback")


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


def _vertex_csr(faces32, V):
    """the vertex -> (face, corner) list as sugar_amd.marching_cubes.vertex_normals builds it (no host read)"""
    sorted_flat, items = torch.sort(faces32.reshape(-1).to(torch.int64), stable=True)
    offsets = torch.searchsorted(sorted_flat, torch.arange(V + 1, device=faces32.device))
    return offsets.to(torch.int32), items.to(torch.int32)


class _Edges:
    """the edge records of one faces tensor (every array has 3 F entries; the first n_edges are used)"""

    def __init__(self, lib, faces32, V):
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
        with torch.cuda.device(dev):
            rc = lib.sgr_mesh_decimate_edges(V, F_, _vp(skey), _vp(order), _vp(group), _vp(self.lo), _vp(self.hi), _vp(self.f0),
                                             _vp(self.f1), _vp(self.nf), _vp(self.bflag), _vp(self.vbnd), _stream(dev))
        _check(rc, "sgr_mesh_decimate_edges")


def _round(lib, P, Q, faces32, target):
    """one round of collapses; returns (P, Q, faces, n_collapsed).  The one host read of the round is `counts.tolist()`."""
    dev = P.device
    V, F_ = int(P.shape[0]), int(faces32.shape[0])
    n = 3 * F_
    st = _stream(dev)
    ed = _Edges(lib, faces32, V)
    offsets, items = _vertex_csr(faces32, V)
    ekey = torch.full((n,), KEY_INVALID, dtype=torch.int64, device=dev)
    epos = torch.empty(n, 3, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        rc = lib.sgr_mesh_decimate_eval(V, F_, _vp(ed.last_edge), _vp(P), _vp(Q), _vp(faces32), _vp(offsets), _vp(items), _vp(ed.lo),
                                        _vp(ed.hi), _vp(ed.f0), _vp(ed.f1), _vp(ed.nf), _vp(ed.vbnd), _vp(ekey), _vp(epos), st)
    _check(rc, "sgr_mesh_decimate_eval")
    order_e = torch.sort(ekey, stable=True).indices
    n_valid = (ekey != KEY_INVALID).sum().reshape(1)
    claim = torch.empty(V, dtype=torch.int64, device=dev)
    lock = torch.zeros(V, dtype=torch.int32, device=dev)
    dead = torch.zeros(n, dtype=torch.uint8, device=dev)
    win = torch.zeros(n, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = lib.sgr_mesh_decimate_select(V, F_, _vp(n_valid), _vp(order_e), _vp(ed.lo), _vp(ed.hi), _vp(ed.nf), _vp(faces32), _vp(offsets),
                                          _vp(items), _vp(claim), _vp(lock), _vp(dead), _vp(win), st)
    _check(rc, "sgr_mesh_decimate_select")
    removed = win.to(torch.int64)
    before = torch.cumsum(removed, 0) - removed             # faces removed by the winners of lower rank
    keep = (win > 0) & ((F_ - before) > int(target))
    keep8 = keep.to(torch.uint8)
    rename = torch.arange(V, dtype=torch.int32, device=dev)
    vkeep = torch.ones(V, dtype=torch.int32, device=dev)
    fkeep = torch.empty(F_, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = lib.sgr_mesh_decimate_apply(V, F_, _vp(keep8), _vp(order_e), _vp(ed.lo), _vp(ed.hi), _vp(epos), _vp(P), _vp(Q), _vp(faces32),
                                         _vp(rename), _vp(vkeep), _vp(fkeep), st)
    _check(rc, "sgr_mesh_decimate_apply")
    vpos, fpos = torch.cumsum(vkeep, 0, dtype=torch.int64), torch.cumsum(fkeep, 0, dtype=torch.int64)
    P2, Q2, faces2 = torch.empty_like(P), torch.empty_like(Q), torch.empty_like(faces32)
    with torch.cuda.device(dev):
        rc = lib.sgr_mesh_decimate_compact(V, F_, _vp(vkeep), _vp(vpos), _vp(fkeep), _vp(fpos), _vp(P), _vp(Q), None, _vp(faces32), _vp(P2),
                                           _vp(Q2), None, _vp(faces2), st)
    _check(rc, "sgr_mesh_decimate_compact")
    counts = torch.stack([vpos[-1], fpos[-1], keep.sum()])
    n_verts, n_faces, n_collapsed = counts.tolist()          # the one device-to-host read of the round
    return P2[:n_verts], Q2[:n_verts], faces2[:n_faces], n_collapsed


def decimate(verts: torch.Tensor, faces: torch.Tensor, target_faces: int, boundary_weight: float = 1.0):
    """Collapses edges in order of quadric error until at most `target_faces` faces remain.  verts[V,3] (float32 is used), faces[F,3]
    int32 / int64 on a ROCm device; the mesh should be clean (see `clean`): faces with a repeated index and edges with more than two
    faces are never collapsed.  Returns (verts float32, faces int64, info) with info = dict(rounds, faces, target, target_met,
    round_limit).  A target of at least F returns the input (as float32 / int64) unchanged."""
    _need_gpu("decimate", verts=verts, faces=faces)
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
    lib = _lib.load()
    dev = v32.device
    faces32 = f64.to(torch.int32)
    centre = 0.5 * (v32.min(dim=0).values.to(torch.float64) + v32.max(dim=0).values.to(torch.float64))
    P = (v32.to(torch.float64) - centre).contiguous()
    ed = _Edges(lib, faces32, V)
    offsets, items = _vertex_csr(faces32, V)
    Q = torch.empty(V, 10, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        rc = lib.sgr_mesh_decimate_quadrics(V, F_, _vp(P), _vp(faces32), _vp(offsets), _vp(items), _vp(ed.bflag), float(boundary_weight),
                                            _vp(Q), _stream(dev))
    _check(rc, "sgr_mesh_decimate_quadrics")
    del ed, offsets, items
    rounds = 0
    while faces32.shape[0] > target and rounds < limit:
        P, Q, faces32, n_collapsed = _round(lib, P, Q, faces32, target)
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
    _need_gpu("clean", verts=verts, faces=faces)
    _shapes("clean", verts, faces)
    lib = _lib.load()
    v = verts.detach().to(torch.float32).contiguous()
    f = faces.detach().to(torch.int32).contiguous()
    dev = v.device
    V = int(v.shape[0])
    st = lambda: _stream(dev)
    vmap = torch.arange(V, dtype=torch.int64, device=dev)
    if V and f.shape[0] and bool(((f < 0) | (f >= V)).any()):
        raise ValueError(f"clean: a face names a vertex outside [0, {V})")

    def ones(n):
        return torch.ones(n, dtype=torch.int32, device=dev)

    if degenerate and f.shape[0]:
        keep = ones(f.shape[0])
        with torch.cuda.device(dev):
            _check(lib.sgr_mesh_clean_degenerate(int(f.shape[0]), _vp(f), _vp(keep), st()), "sgr_mesh_clean_degenerate")
        f = f[keep.bool()].contiguous()
    if duplicated_triangles and f.shape[0]:
        perm = _lexsort_rows(torch.sort(f, dim=1).values)
        keep = ones(f.shape[0])
        with torch.cuda.device(dev):
            _check(lib.sgr_mesh_clean_duplicate_faces(int(f.shape[0]), _vp(f), _vp(perm), _vp(keep), st()), "sgr_mesh_clean_duplicate_faces")
        f = f[keep.bool()].contiguous()
    if duplicated_vertices and V:
        perm = _lexsort_rows(v.view(torch.int32))
        start = torch.empty(V, dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            _check(lib.sgr_mesh_clean_duplicate_verts(V, _vp(v), _vp(perm), _vp(start), st()), "sgr_mesh_clean_duplicate_verts")
        pos = torch.arange(V, device=dev)
        leader = torch.cummax(torch.where(start == 1, pos, torch.zeros_like(pos)), 0).values
        vmap = torch.empty(V, dtype=torch.int64, device=dev)
        vmap[perm] = perm[leader]
        if f.shape[0]:
            f = vmap[f.to(torch.int64)].to(torch.int32).contiguous()
    while non_manifold_edges and f.shape[0] and V:
        skey, order = _sorted_incidences(f, V)
        remove = torch.zeros(f.shape[0], dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            _check(lib.sgr_mesh_clean_nonmanifold(V, int(f.shape[0]), _vp(skey), _vp(order), _vp(v), _vp(f), _vp(remove), st()),
                   "sgr_mesh_clean_nonmanifold")
        if int(remove.sum()) == 0:
            break
        f = f[remove == 0].contiguous()
    F_ = int(f.shape[0])
    if V == 0 or F_ == 0:
        return v[:0], torch.zeros(0, 3, dtype=torch.int64, device=dev), torch.full((V,), -1, dtype=torch.int64, device=dev)
    ref = torch.zeros(V, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _check(lib.sgr_mesh_clean_referenced(V, F_, _vp(f), _vp(ref), st()), "sgr_mesh_clean_referenced")
    vpos = torch.cumsum(ref, 0, dtype=torch.int64)
    fkeep = ones(F_)
    fpos = torch.cumsum(fkeep, 0, dtype=torch.int64)
    v2, f2 = torch.empty_like(v), torch.empty_like(f)
    with torch.cuda.device(dev):
        rc = lib.sgr_mesh_decimate_compact(V, F_, _vp(ref), _vp(vpos), _vp(fkeep), _vp(fpos), None, None, _vp(v), _vp(f), None, None, _vp(v2),
                                           _vp(f2), st())
    _check(rc, "sgr_mesh_decimate_compact")
    n_verts = int(vpos[-1])
    new_id = torch.where(ref > 0, vpos - 1, torch.full_like(vpos, -1))
    return v2[:n_verts], f2.to(torch.int64), new_id[vmap]
