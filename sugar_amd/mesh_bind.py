"""The refine stage's mesh binding and normal-consistency regulariser on the HIP kernels of csrc/mesh_bind.hip (C ABI:
sgr_mesh_bind_* / sgr_normal_consistency_* in include/sugar_raster.h).

A refine-mode SuGaR model derives its Gaussians from the surface mesh it is bound to (sugar_scene/sugar_model.py:383-479): Gaussian
g = f * n + k sits on face f at the barycentric coordinates bary[k], is flat (the thickness along the face normal, exp(_scales) in the
plane) and is oriented by the face frame turned in the plane by a learned complex number.  The reference evaluates each of the three
properties as a chain of small tensor operations every time it is read, and `mesh_normal_consistency` rebuilds the mesh's edge topology
every iteration.  Here:

  * `bound_points`, `bound_scaling`, `bound_quaternions`: one `torch.autograd.Function` each (the reference reads the properties
    independently, several times per step), one forward and one backward call of the C ABI each;
  * `normal_consistency(verts, faces)`: the stand-in `pytorch3d.loss.mesh_normal_consistency` of one mesh, over a pair list;
  * `MeshTopology.get(faces)`: everything that depends on the faces alone -- int32 faces, the vertex -> (face, corner) list, the pairs
    of faces sharing an edge and the vertex -> (pair, slot) list -- built with torch operations ONCE per faces tensor and cached.  After
    that no call of this module waits on the device.

Vertex gradients are deterministic: per-(face, corner) and per-(pair, slot) contributions are written out and every vertex adds its own in
the order of its list; there are no float atomics.  There is no CPU path: CPU tensors raise."""
from __future__ import annotations

from collections import OrderedDict

import torch

from . import _lib
from ._call import call, csr, need_gpu as _need_gpu, ptr

CACHE_ENTRIES = 4


def edge_pairs(faces: torch.Tensor, n_verts: int):
    """(pairs[n_pairs,4] int64: v0 < v1 of the shared edge, then the opposite vertices a, b of the two faces;
    pair_faces[n_pairs,2] int64: the two faces, first < second).  One entry per pair of faces sharing an edge: an edge with k faces
    gives k(k-1)/2 entries, a boundary edge none -- the pairs the stand-in `mesh_normal_consistency` derives, with its rule for the
    opposite vertex (the largest face vertex that is neither v0 nor v1; 0 for a face that has none).  A face that repeats a vertex,
    (i, j, j), carries the edge (i, j) twice and so forms a pair with itself, as it does in the stand-in: such faces are not rejected."""
    f = faces.to(torch.int64)
    F_ = f.shape[0]
    dev = f.device
    V = max(int(n_verts), 1)
    # incidence s = 3 face + k: face (a, b, c) has the edges (b, c), (c, a), (a, b)
    e = torch.stack([f[:, [1, 2]], f[:, [2, 0]], f[:, [0, 1]]], dim=1).reshape(3 * F_, 2)
    lo, hi = e.min(dim=1).values, e.max(dim=1).values
    key = lo * V + hi
    skey, order = torch.sort(key, stable=True)                   # incidences grouped by edge, by face within an edge
    new = torch.ones(3 * F_, dtype=torch.bool, device=dev)
    new[1:] = skey[1:] != skey[:-1]
    group = torch.cumsum(new.to(torch.int64), 0) - 1             # edge id of every sorted incidence
    count = torch.bincount(group)
    start = torch.cumsum(count, 0) - count
    pos = torch.arange(3 * F_, device=dev)
    reps = count[group] - 1 - (pos - start[group])               # partners later in the same group
    first = torch.repeat_interleave(pos, reps)
    base = torch.cumsum(reps, 0) - reps
    second = first + 1 + (torch.arange(first.shape[0], device=dev) - base[first])
    face_of = torch.div(order, 3, rounding_mode="floor")
    fv = f[face_of]                                              # the face of every sorted incidence
    v0, v1 = lo[order], hi[order]
    opposite = (fv != v0[:, None]) & (fv != v1[:, None])
    other = torch.where(opposite, fv, torch.full_like(fv, -1)).max(dim=1).values.clamp_min(0)
    pairs = torch.stack([v0[first], v1[first], other[first], other[second]], dim=1)
    return pairs.contiguous(), torch.stack([face_of[first], face_of[second]], dim=1).contiguous()


class MeshTopology:
    """What the kernels need of a faces tensor, built once: `faces` [F,3] int32, `vert_offsets` [V+1] / `vert_items` [3F] (the vertex ->
    (face, corner) list, item = 3 face + corner, ascending), `pairs` [n_pairs,4] int32, `pair_faces` [n_pairs,2], `pair_offsets` [V+1] /
    `pair_items` [4 n_pairs] (the vertex -> (pair, slot) list, item = 4 pair + slot), `n_pairs`, `n_faces`, `n_verts`."""
    _cache: "OrderedDict[tuple, MeshTopology]" = OrderedDict()

    def __init__(self, faces: torch.Tensor, n_verts: int):
        if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype not in (torch.int32, torch.int64):
            raise ValueError("MeshTopology: faces must be an int32 / int64 tensor of shape [F,3]")
        f = faces.detach()
        self.n_faces = int(f.shape[0])
        self.n_verts = int(n_verts)
        if self.n_faces == 0 or self.n_verts <= 0:
            raise ValueError("MeshTopology: need at least one face and one vertex")
        if bool(((f < 0) | (f >= self.n_verts)).any()):
            raise ValueError(f"MeshTopology: a face names a vertex outside [0, {self.n_verts})")
        self.faces = f.to(torch.int32).contiguous()
        self.vert_offsets, self.vert_items = csr(f, self.n_verts)
        pairs, self.pair_faces = edge_pairs(f, self.n_verts)
        self.n_pairs = int(pairs.shape[0])
        self.pairs = pairs.to(torch.int32).contiguous()
        self.pair_offsets, self.pair_items = csr(pairs, self.n_verts)
        self.device = f.device
        self._keepalive = faces        # the cache key holds its data_ptr: keep the storage from being reused

    @classmethod
    def get(cls, faces: torch.Tensor, n_verts: int | None = None) -> "MeshTopology":
        """the cached topology of `faces` (keyed by the tensor's storage pointer, shape, dtype, version counter and device, and the
        vertex count; `n_verts=None` reads max(faces) + 1 from the device when the entry is built)"""
        key = (faces.data_ptr(), tuple(faces.shape), faces.dtype, faces._version, str(faces.device), n_verts)
        hit = cls._cache.get(key)
        if hit is not None:
            cls._cache.move_to_end(key)
            return hit
        topo = cls(faces, int(faces.max()) + 1 if n_verts is None else n_verts)
        cls._cache[key] = topo
        while len(cls._cache) > CACHE_ENTRIES:
            cls._cache.popitem(last=False)
        return topo

    @classmethod
    def clear(cls) -> None:
        cls._cache.clear()


def _f32c(t):
    t = t.detach()
    return t if (t.dtype == torch.float32 and t.is_contiguous()) else t.to(torch.float32).contiguous()


def _bary(bary, device):
    b = bary.detach().to(device=device, dtype=torch.float32)
    if b.dim() == 3 and b.shape[-1] == 1:
        b = b[..., 0]
    if b.dim() != 2 or b.shape[1] != 3:
        raise ValueError("barycentric coordinates must be [n,3] (or [n,3,1])")
    return b.contiguous()


def _backward(topo, n, verts, bary, scales, cplx, g_points, g_scaling, g_quats):
    """one sgr_mesh_bind_backward call; returns (d_verts, d_scales, d_cplx), None where not requested"""
    mesh = g_points is not None or g_quats is not None
    dev = (g_points if g_points is not None else g_quats if g_quats is not None else g_scaling).device
    F_, V = topo.n_faces, topo.n_verts
    d_verts = torch.empty(V, 3, dtype=torch.float32, device=dev) if mesh else None
    contrib = torch.empty(3 * F_, 3, dtype=torch.float32, device=dev) if mesh else None
    d_scales = torch.empty(F_ * n, 2, dtype=torch.float32, device=dev) if g_scaling is not None else None
    d_cplx = torch.empty(F_ * n, 2, dtype=torch.float32, device=dev) if g_quats is not None else None
    call("sgr_mesh_bind_backward", dev, F_, n, V, ptr(verts), ptr(topo.faces), ptr(bary), ptr(scales), ptr(cplx), ptr(g_points),
         ptr(g_scaling), ptr(g_quats), ptr(topo.vert_offsets), ptr(topo.vert_items), ptr(contrib), ptr(d_verts), ptr(d_scales), ptr(d_cplx))
    return d_verts, d_scales, d_cplx


class _BoundPoints(torch.autograd.Function):
    @staticmethod
    def forward(ctx, verts, topo, bary):
        v = _f32c(verts)
        n = int(bary.shape[0])
        out = torch.empty(topo.n_faces * n, 3, dtype=torch.float32, device=v.device)
        call("sgr_mesh_bind_forward", v.device, topo.n_faces, n, topo.n_verts, ptr(v), ptr(topo.faces), ptr(bary), None, None, None,
             ptr(out), None, None)
        ctx.topo, ctx.bary, ctx.n = topo, bary, n
        return out

    @staticmethod
    def backward(ctx, grad):
        d_verts, _, _ = _backward(ctx.topo, ctx.n, None, ctx.bary, None, None, _f32c(grad), None, None)
        return d_verts, None, None


class _BoundScaling(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scales, thickness):
        s = _f32c(scales)
        P = int(s.shape[0])
        out = torch.empty(P, 3, dtype=torch.float32, device=s.device)
        call("sgr_mesh_bind_forward", s.device, P, 1, 0, None, None, None, ptr(s), None, ptr(thickness), None, ptr(out), None)
        ctx.save_for_backward(s)
        return out

    @staticmethod
    def backward(ctx, grad):
        (s,) = ctx.saved_tensors
        g = _f32c(grad)
        P = int(s.shape[0])
        d_scales = torch.empty(P, 2, dtype=torch.float32, device=g.device)
        call("sgr_mesh_bind_backward", g.device, P, 1, 0, None, None, None, ptr(s), None, None, ptr(g), None, None, None, None, None,
             ptr(d_scales), None)
        return d_scales, None


class _BoundQuaternions(torch.autograd.Function):
    @staticmethod
    def forward(ctx, verts, cplx, topo, n):
        v, z = _f32c(verts), _f32c(cplx)
        out = torch.empty(topo.n_faces * n, 4, dtype=torch.float32, device=v.device)
        call("sgr_mesh_bind_forward", v.device, topo.n_faces, n, topo.n_verts, ptr(v), ptr(topo.faces), None, None, ptr(z), None, None,
             None, ptr(out))
        ctx.save_for_backward(v, z)
        ctx.topo, ctx.n = topo, n
        return out

    @staticmethod
    def backward(ctx, grad):
        v, z = ctx.saved_tensors
        d_verts, _, d_cplx = _backward(ctx.topo, ctx.n, v, None, None, z, None, None, _f32c(grad))
        return d_verts, d_cplx, None, None


def _topology(verts, faces):
    if verts.dim() != 2 or verts.shape[1] != 3:
        raise ValueError("verts must be [V,3]")
    return MeshTopology.get(faces, int(verts.shape[0]))


def bound_points(verts: torch.Tensor, faces: torch.Tensor, bary: torch.Tensor) -> torch.Tensor:
    """`SuGaR.points` of a bound model (:392-398): [F*n,3], row f*n+k = sum_c verts[faces[f,c]] * bary[k,c].  verts[V,3] float32 (may
    require grad), faces[F,3] int32 / int64, bary[n,3] or [n,3,1]."""
    _need_gpu("bound_points", verts=verts, faces=faces)
    return _BoundPoints.apply(verts, _topology(verts, faces), _bary(bary, verts.device))


def bound_scaling(scales: torch.Tensor, thickness) -> torch.Tensor:
    """`SuGaR.scaling` of a bound model with `scale_activation = torch.exp` (:420, :438-441): [P,3] = (thickness, exp(scales)).
    scales[P,2]; thickness: a tensor with one element on the device (the model's `surface_mesh_thickness`), or a Python float."""
    _need_gpu("bound_scaling", scales=scales)
    if scales.dim() != 2 or scales.shape[1] != 2:
        raise ValueError("scales must be [P,2]")
    if torch.is_tensor(thickness):
        if thickness.numel() != 1:
            raise ValueError("thickness must hold one element")
        th = thickness.detach().to(device=scales.device, dtype=torch.float32).reshape(1)
    else:
        th = torch.full((1,), float(thickness), dtype=torch.float32, device=scales.device)
    return _BoundScaling.apply(scales, th)


def bound_quaternions(verts: torch.Tensor, faces: torch.Tensor, complex_numbers: torch.Tensor, n: int) -> torch.Tensor:
    """`SuGaR.quaternions` of a bound, non-editable model (:449-479): [F*n,4], unit, real part first.  complex_numbers[F*n,2]."""
    _need_gpu("bound_quaternions", verts=verts, faces=faces, complex_numbers=complex_numbers)
    topo = _topology(verts, faces)
    n = int(n)
    if n <= 0 or tuple(complex_numbers.shape) != (topo.n_faces * n, 2):
        raise ValueError(f"complex_numbers must be [F*n,2] = [{topo.n_faces * n},2]")
    return _BoundQuaternions.apply(verts, complex_numbers, topo, n)


class _NormalConsistency(torch.autograd.Function):
    @staticmethod
    def forward(ctx, verts, topo):
        lib = _lib.load()
        v = _f32c(verts)
        loss = torch.empty(1, dtype=torch.float32, device=v.device)
        scratch = torch.empty(lib.sgr_normal_consistency_scratch_bytes() // 8, dtype=torch.float64, device=v.device)
        call("sgr_normal_consistency_forward", v.device, topo.n_pairs, topo.n_verts, ptr(v), ptr(topo.pairs), ptr(scratch), ptr(loss))
        ctx.save_for_backward(v)
        ctx.topo = topo
        return loss.reshape(())

    @staticmethod
    def backward(ctx, grad):
        (v,) = ctx.saved_tensors
        topo = ctx.topo
        g = _f32c(grad).reshape(1)
        d_verts = torch.empty(topo.n_verts, 3, dtype=torch.float32, device=v.device)
        contrib = torch.empty(4 * topo.n_pairs, 3, dtype=torch.float32, device=v.device)
        call("sgr_normal_consistency_backward", v.device, topo.n_pairs, topo.n_verts, ptr(v), ptr(topo.pairs), ptr(g),
             ptr(topo.pair_offsets), ptr(topo.pair_items), ptr(contrib), ptr(d_verts))
        return d_verts, None


def normal_consistency(verts: torch.Tensor, faces: torch.Tensor) -> torch.Tensor:
    """`pytorch3d.loss.mesh_normal_consistency` of ONE mesh as the stand-in of sugar_amd.shims defines it: a 0-dim tensor,
    differentiable in verts.  A mesh without a pair of faces sharing an edge gives 0 (and no gradient), as the stand-in does."""
    _need_gpu("normal_consistency", verts=verts, faces=faces)
    topo = _topology(verts, faces)
    if topo.n_pairs == 0:
        return verts.sum() * 0.0
    return _NormalConsistency.apply(verts, topo)
