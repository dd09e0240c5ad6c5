"""The optional border-face postprocess of SuGaR's refined-mesh export (sugar_extractors/refined_mesh.py:125-187) on the HIP kernels of
csrc/mesh_postprocess.hip (C ABI: sgr_mesh_peel_border in include/sugar_raster.h).

The peel rule.  Face (a, b, c) has three slots carrying the unordered pairs {a,b}, {b,c}, {c,a}.  With a live set of faces, the live
count of a pair is the number of SLOTS of live faces that carry it (a face (i, j, j) carries {i,j} twice; two copies of one face make
each other's pairs count 2; an edge with three faces counts 3).  One iteration: a live face stays live iff all three of its pairs have
live count >= 2, every count taken before any face of that iteration is removed.  `iterations` such steps run, with no early exit; an
empty set stays empty.  The reference asks the same question by running `knn_points` (K = 2) over the float tensor of the live faces'
sorted pairs once per iteration and testing the second-nearest squared distance against 0.01; the two agree whenever vertex ids are below
2^24, above which the reference's float cast collides and its result is not defined.  Here the arithmetic is integer and exact.

  * `peel_border_faces`: the peel.  What depends on the faces alone (`PeelTopology`: the edge id of every slot and the edge -> slots
    list) is built once with torch operations; the loop is one call of the C ABI that enqueues every iteration and never waits.
  * `readd_dense_faces` (:150-152): a dead face whose centre lies where the Gaussians' density exceeds a threshold comes back; the
    16-NN and the density are the package's HIP k-NN and density field, the rest is torch indexing (not a hot path).
  * `postprocess_bound_mesh`: the whole block for a model bound to the mesh with n Gaussians per triangle.

There is no CPU path: CPU tensors raise."""
from __future__ import annotations

from typing import NamedTuple

import torch

from . import _lib
from ._call import call, csr, need_gpu, ptr

READD_NEIGHBOURS = 16   # the extractor builds its model with keep_track_of_knn=False: get_gaussians_closest_to_samples falls to 16


def _check_faces(what, faces):
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{what}: faces must be an int32 / int64 tensor of shape [F,3]")


class PeelTopology:
    """What the peel needs of a faces tensor, built once: `slot_edge` [3F] int32 (slot 3 f + k carries pair k of face f: {a,b}, {b,c},
    {c,a}; equal pairs have equal ids), `n_edges`, and the edge -> slots list `edge_offsets` [E+1] / `edge_items` [3F] (int32).  Building
    it reads the vertex range and the edge count from the device; nothing after it does."""

    def __init__(self, faces: torch.Tensor, n_verts: int | None = None):
        _check_faces("PeelTopology", faces)
        f = faces.detach().to(torch.int64)
        self.n_faces = int(f.shape[0])
        self.device = f.device
        self.n_verts, self.n_edges = int(n_verts or 0), 0
        if self.n_faces:                          # (arguments are judged before the device: a bad tensor is a ValueError anywhere)
            lo_id, hi_id = int(f.min()), int(f.max())
            self.n_verts = hi_id + 1 if n_verts is None else int(n_verts)
            if lo_id < 0 or hi_id >= self.n_verts:
                raise ValueError(f"PeelTopology: a face names a vertex outside [0, {self.n_verts})")
        need_gpu("PeelTopology", faces=faces)
        if self.n_faces == 0:
            self.slot_edge = self.edge_items = torch.empty(0, dtype=torch.int32, device=f.device)
            self.edge_offsets = torch.zeros(1, dtype=torch.int32, device=f.device)
            return
        e = torch.stack([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], dim=1).reshape(3 * self.n_faces, 2)
        key = e.min(dim=1).values * self.n_verts + e.max(dim=1).values
        uniq, inverse = torch.unique(key, return_inverse=True)
        self.n_edges = int(uniq.shape[0])
        self.slot_edge = inverse.to(torch.int32).contiguous()
        self.edge_offsets, self.edge_items = csr(inverse, self.n_edges)


def peel_border_faces(faces: torch.Tensor, iterations: int, face_mask: torch.Tensor | None = None, n_verts: int | None = None,
                      topology: PeelTopology | None = None) -> torch.Tensor:
    """bool[F]: the faces still live after `iterations` steps of the peel rule (module docstring), starting from `face_mask`
    (bool[F]; None: all faces).  faces[F,3] int32 / int64 on a ROCm device; a face naming a vertex outside [0, n_verts) raises
    ValueError (`n_verts=None`: max(faces) + 1).  `topology`: a `PeelTopology` of the same faces, to build it once for several calls."""
    _check_faces("peel_border_faces", faces)
    iterations = int(iterations)
    if iterations < 0:
        raise ValueError("peel_border_faces: iterations must not be negative")
    F_ = int(faces.shape[0])
    if face_mask is not None and (not torch.is_tensor(face_mask) or face_mask.dtype != torch.bool or tuple(face_mask.shape) != (F_,)
                                  or face_mask.device != faces.device):
        raise ValueError(f"peel_border_faces: face_mask must be a bool tensor of shape [{F_}] on the faces' device")
    topo = PeelTopology(faces, n_verts) if topology is None else topology
    need_gpu("peel_border_faces", faces=faces)
    if face_mask is None:
        live = torch.ones(F_, dtype=torch.uint8, device=faces.device)
    else:
        live = face_mask.to(torch.uint8)          # (a copy: the kernel updates it in place)
    if topo.n_faces != F_ or topo.device != faces.device:
        raise ValueError("peel_border_faces: the topology belongs to another faces tensor")
    if F_ == 0 or iterations == 0:                # nothing to launch
        return live.bool()
    scratch = torch.empty(_lib.load().sgr_mesh_peel_border_scratch_bytes(topo.n_edges), dtype=torch.uint8, device=faces.device)
    call("sgr_mesh_peel_border", faces.device, F_, topo.n_edges, ptr(topo.slot_edge), ptr(topo.edge_offsets), ptr(topo.edge_items),
         iterations, ptr(live), ptr(scratch))
    return live.bool()


def readd_dense_faces(verts, faces, face_mask, points, scaling, quaternions, strengths, density_threshold: float,
                      n_closest: int = READD_NEIGHBOURS) -> torch.Tensor:
    """bool[F]: `face_mask` with every dead face revived whose density is strictly above `density_threshold` (:150-152).  The centre of
    a face is `verts[faces].mean(-2)` (torch's rounding), its density `SuGaR.compute_density` (sugar_model.py:1345-1368) over the
    `n_closest` nearest of the Gaussians points[P,3] / scaling[P,3] / quaternions[P,4] / strengths[P] or [P,1], density_factor 1.
    With no dead face the mask comes back unchanged and nothing is launched."""
    from .field import density_field, scaled_rotation
    from .knn import knn_points
    need_gpu("readd_dense_faces", verts=verts, faces=faces, face_mask=face_mask, points=points, scaling=scaling, quaternions=quaternions,
             strengths=strengths)
    _check_faces("readd_dense_faces", faces)
    F_, P = int(faces.shape[0]), int(points.shape[0])
    if verts.dim() != 2 or verts.shape[1] != 3:
        raise ValueError("readd_dense_faces: verts must be [V,3]")
    if face_mask.dtype != torch.bool or tuple(face_mask.shape) != (F_,):
        raise ValueError(f"readd_dense_faces: face_mask must be a bool tensor of shape [{F_}]")
    if tuple(points.shape) != (P, 3) or tuple(scaling.shape) != (P, 3) or tuple(quaternions.shape) != (P, 4) or strengths.numel() != P:
        raise ValueError("readd_dense_faces: points[P,3], scaling[P,3], quaternions[P,4] and strengths[P] must describe the same Gaussians")
    if P < int(n_closest):
        raise ValueError(f"readd_dense_faces: the density needs at least {int(n_closest)} Gaussians, got {P}")
    out = face_mask.clone()
    dead = (~face_mask).nonzero(as_tuple=True)[0]
    if dead.numel() == 0:
        return out
    with torch.no_grad():
        centres = verts.detach().float()[faces[dead].to(torch.int64)].mean(-2).contiguous()
        pts = points.detach().float().contiguous()
        idx = knn_points(centres[None], pts[None], K=int(n_closest)).idx[0]
        B = scaled_rotation(quaternions.detach(), scaling.detach(), inverse_scales=True)
        _, density = density_field(centres, idx, pts, B, strengths.detach().reshape(P), 1.0)
        out[dead] = density > float(density_threshold)
    return out


def bary_coords(n: int) -> torch.Tensor:
    """[n,3]: the barycentric coordinates of the n Gaussians of a triangle (sugar_model.py:171-213); n in {1, 3, 4, 6}"""
    from .synthetic import _BARY
    if int(n) not in _BARY:
        raise ValueError(f"{n} Gaussians per triangle: the bound model exists for 1, 3, 4 and 6")
    return torch.tensor(_BARY[int(n)][0], dtype=torch.float32)


def compact_rows(t: torch.Tensor, face_mask: torch.Tensor, n: int) -> torch.Tensor:
    """the rows of the kept faces of a per-Gaussian tensor [F*n, ...] (triangle-major, Gaussian g = f * n + k), in order"""
    F_ = int(face_mask.shape[0])
    if t.shape[0] != F_ * n:
        raise ValueError(f"a per-Gaussian tensor has {t.shape[0]} rows, expected F*n = {F_ * n}")
    return t.reshape(F_, n, *t.shape[1:])[face_mask].reshape(-1, *t.shape[1:])


class PostprocessedMesh(NamedTuple):
    face_mask: torch.Tensor        # bool[F]
    faces: torch.Tensor            # [F',3]: the kept faces in their original order, the dtype handed in
    per_gaussian: tuple            # every per-Gaussian tensor handed in, reduced to the rows of the kept faces


def postprocess_bound_mesh(verts, faces, n: int, scales, complex_numbers, all_densities, thickness, *extra, iterations: int = 5,
                           density_threshold: float = 0.1) -> PostprocessedMesh:
    """refined_mesh.py:125-187 for a model bound to the mesh verts[V,3] / faces[F,3] with n Gaussians per triangle: peel the border
    faces `iterations` times, revive the dead faces of density > `density_threshold`, keep the rest.  scales[F*n,2] (`_scales`),
    complex_numbers[F*n,2] (`_quaternions`), all_densities[F*n,1] or [F*n] (before the sigmoid), thickness (`surface_mesh_thickness`: a
    one-element tensor or a float); `extra`: further per-Gaussian tensors [F*n, ...] (the SH coefficients).  `per_gaussian` of the result
    holds scales, complex_numbers, all_densities and the extras, each reduced to the rows of the kept faces.  Vertices are not touched
    (the reference keeps all of them), so the kept faces may leave vertices unreferenced.
    Works for n in {1, 3, 4, 6}.  The reference's own block only completes for n = 1: its mask comes from `strengths` and has F*n
    entries, which index the F faces only when n = 1; here the mask has one entry per face."""
    from . import mesh_bind
    need_gpu("postprocess_bound_mesh", verts=verts, faces=faces, scales=scales, complex_numbers=complex_numbers, all_densities=all_densities)
    _check_faces("postprocess_bound_mesh", faces)
    n = int(n)
    bary = bary_coords(n).to(verts.device)
    F_ = int(faces.shape[0])
    rows = (scales, complex_numbers, all_densities, *extra)
    for t in rows:
        if not torch.is_tensor(t) or not t.is_cuda:
            raise RuntimeError("postprocess_bound_mesh: every per-Gaussian tensor must be on a ROCm device; there is no CPU fallback")
        if t.shape[0] != F_ * n:
            raise ValueError(f"postprocess_bound_mesh: a per-Gaussian tensor has {t.shape[0]} rows, expected F*n = {F_ * n}")
    if F_ == 0:
        return PostprocessedMesh(torch.zeros(0, dtype=torch.bool, device=faces.device), faces, rows)
    with torch.no_grad():
        mask = peel_border_faces(faces, iterations, n_verts=int(verts.shape[0]))
        points = mesh_bind.bound_points(verts.detach(), faces, bary)
        scaling = mesh_bind.bound_scaling(scales.detach(), thickness)
        quats = mesh_bind.bound_quaternions(verts.detach(), faces, complex_numbers.detach(), n)
        strengths = torch.sigmoid(all_densities.detach().float().reshape(-1))
        mask = readd_dense_faces(verts, faces, mask, points, scaling, quats, strengths, density_threshold)
        return PostprocessedMesh(mask, faces[mask], tuple(compact_rows(t, mask, n) for t in rows))
