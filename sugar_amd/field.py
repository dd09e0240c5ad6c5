"""Host side of SuGaR's density field and level-set sampler (C ABI: sgr_density_field_*, sgr_level_set_points).

`density_field(x, nbr_idx, centers, inv_scaled_rot, strengths)` is the differentiable core of
SuGaR.get_field_values (sugar_scene/sugar_model.py:1247-1281); `level_set_points(...)` is the per-pixel part of
SuGaR.compute_level_surface_points_from_camera_fast (:1971-2079).  Both read the same tensors SuGaR already holds
(`self.points`, `self.get_covariance(return_full_matrix=True, return_sqrt=True, inverse_scales=True)`, `self.strengths`,
`self.knn_idx`).  GPU tensors only; the HIP library must be built.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._call import call, ptr, stream

_p, _stream = ptr, stream    # the names tests/test_gpu_field.py drives the C ABI through


def _pack(lib, ce, Bm, st):
    """one 64-byte record per Gaussian for the kernels' neighbour gathers (sgr_pack_gaussians).  `lib` is no longer read (`call` loads
    the library itself); it stays in the signature because tests/test_gpu_field.py and scripts/marching_cubes_bench.py pass it."""
    P, dev = ce.shape[0], ce.device
    packed = torch.empty(P, 16, device=dev)
    call("sgr_pack_gaussians", dev, P, ptr(ce), ptr(Bm), ptr(st), ptr(packed))
    return packed


def _prep(x, nbr_idx, centers, B, strengths):
    if not x.is_cuda:
        raise RuntimeError("the HIP density field needs tensors on a ROCm device; there is no CPU fallback")
    P = centers.shape[0]
    return (x.contiguous().float(), nbr_idx.contiguous().to(torch.int64), centers.contiguous().float(),
            B.reshape(P, 9).contiguous().float(), strengths.reshape(P).contiguous().float())


class _DensityField(torch.autograd.Function):
    use_gather = True  # False: the 13-float-atomics-per-pair kernel (kept for comparison)

    @staticmethod
    def forward(ctx, x, nbr_idx, centers, inv_scaled_rot, strengths, density_factor):
        lib = _lib.load()
        xs, nb, ce, Bm, st = _prep(x, nbr_idx, centers, inv_scaled_rot, strengths)
        N, K = nb.shape
        dev = xs.device
        opac = torch.empty(N, K, device=dev)
        dens = torch.empty(N, device=dev)
        packed = _pack(lib, ce, Bm, st)
        call("sgr_density_field_forward", dev, N, K, ptr(xs), ptr(nb), ptr(ce), ptr(Bm), ptr(st), float(density_factor), ptr(opac),
             ptr(dens), ptr(packed))
        ctx.save_for_backward(xs, nb, ce, Bm, st, packed)
        ctx.factor = float(density_factor)
        ctx.shapes = (inv_scaled_rot.shape, strengths.shape)
        return opac, dens

    @staticmethod
    def backward(ctx, g_opac, g_dens):
        lib = _lib.load()
        xs, nb, ce, Bm, st, packed = ctx.saved_tensors
        N, K = nb.shape
        dev = xs.device
        P = ce.shape[0]
        dx = torch.empty(N, 3, device=dev)
        go = g_opac.contiguous().float() if g_opac is not None else None
        gd = g_dens.contiguous().float() if g_dens is not None else None
        if _DensityField.use_gather:
            # one integer atomic per pair + a per-Gaussian gather (every output row is written)
            dce = torch.empty(P, 3, device=dev); dB = torch.empty(P, 9, device=dev); dst = torch.empty(P, device=dev)
            scratch = torch.empty(lib.sgr_density_field_backward_scratch_bytes(N, K, P), dtype=torch.uint8, device=dev)
            call("sgr_density_field_backward_gather", dev, N, K, P, ptr(xs), ptr(nb), ptr(ce), ptr(Bm), ptr(st), ctx.factor, ptr(go), ptr(gd),
                 ptr(dx), ptr(dce), ptr(dB), ptr(dst), ptr(scratch), ptr(packed))
        else:
            dce = torch.zeros(P, 3, device=dev); dB = torch.zeros(P, 9, device=dev); dst = torch.zeros(P, device=dev)
            call("sgr_density_field_backward", dev, N, K, ptr(xs), ptr(nb), ptr(ce), ptr(Bm), ptr(st), ctx.factor, ptr(go), ptr(gd), ptr(dx),
                 ptr(dce), ptr(dB), ptr(dst), ptr(packed))
        Bshape, sshape = ctx.shapes
        return dx, None, dce, dB.reshape(Bshape), dst.reshape(sshape), None


class _ScaledRotation(torch.autograd.Function):
    @staticmethod
    def forward(ctx, quaternions, scaling, inverse_scales):
        if not quaternions.is_cuda:
            raise RuntimeError("the HIP scaled-rotation op needs tensors on a ROCm device; there is no CPU fallback")
        q, s = quaternions.contiguous().float(), scaling.contiguous().float()
        P, dev = q.shape[0], q.device
        out = torch.empty(P, 3, 3, device=dev)
        call("sgr_scaled_rotation_forward", dev, P, ptr(q), ptr(s), int(bool(inverse_scales)), ptr(out))
        ctx.save_for_backward(q, s)
        ctx.inverse = int(bool(inverse_scales))
        return out

    @staticmethod
    def backward(ctx, g):
        q, s = ctx.saved_tensors
        P, dev = q.shape[0], q.device
        dq, ds = torch.empty_like(q), torch.empty_like(s)
        g = g.contiguous().float()  # (kept referenced until the call is enqueued: a temporary's block goes back to the allocator at once)
        call("sgr_scaled_rotation_backward", dev, P, ptr(q), ptr(s), ctx.inverse, ptr(g), ptr(dq), ptr(ds))
        return dq, ds, None


def scaled_rotation(quaternions, scaling, inverse_scales: bool = False):
    """SuGaR.get_covariance(return_sqrt=True, inverse_scales=...) (sugar_scene/sugar_model.py:730-736):
    quaternion_to_matrix(quaternions) * s[:, None] with s = scaling or 1 / scaling.clamp(min=1e-8); differentiable."""
    return _ScaledRotation.apply(quaternions, scaling, inverse_scales)


def density_field(x, nbr_idx, centers, inv_scaled_rot, strengths, density_factor: float = 1.0):
    """Returns (neighbor_opacities[N,K], densities[N]) exactly as sugar_model.py:1270-1276, differentiable w.r.t. x,
    centers, inv_scaled_rot and strengths."""
    return _DensityField.apply(x, nbr_idx, centers, inv_scaled_rot, strengths, density_factor)


def level_set_points(world_points, nbr_idx, cam_center, centers, inv_scaled_rot, strengths, gaussian_std,
                     surface_levels=(0.1, 0.3, 0.5), n_points_in_range: int = 21, range_size: float = 3.0,
                     density_factor: float = 1.0, return_normals: bool = True, raw: bool = False):
    """Per level: dict(valid=bool[N], valid_idx=int64[n_valid], intersection_points=[n_valid,3], normals=[n_valid,3]) -- the `outputs` of
    sugar_model.py:2013-2081 (rows where the reference's empty_pixels is False).
    `raw=True`: no gathering (and no host round trip): returns (valid uint8[L,N], points[L,N,3], normals[L,N,3] or None) as the kernel
    wrote them -- sugar_amd.sampler compacts them on the device."""
    lib = _lib.load()
    wp, nb, ce, Bm, st = _prep(world_points, nbr_idx, centers, inv_scaled_rot, strengths)
    dev = wp.device
    N, K = nb.shape
    L = len(surface_levels)
    cam = cam_center.reshape(3).contiguous().float().to(dev)
    gstd = gaussian_std.reshape(-1).contiguous().float()
    valid = torch.empty(L, N, dtype=torch.uint8, device=dev)
    pts = torch.empty(L, N, 3, device=dev)
    nrm = torch.empty(L, N, 3, device=dev) if return_normals else None
    lv = (C.c_float * L)(*[float(v) for v in surface_levels])
    packed = _pack(lib, ce, Bm, st)
    call("sgr_level_set_points", dev, N, K, ptr(wp), ptr(nb), ptr(cam), ptr(ce), ptr(Bm), ptr(st), ptr(gstd), L, lv, int(n_points_in_range),
         float(range_size), float(density_factor), ptr(valid), ptr(pts), ptr(nrm), ptr(packed))
    if raw:
        return valid, pts, nrm
    out = {}
    for i, level in enumerate(surface_levels):
        m = valid[i].bool()
        rows = m.nonzero(as_tuple=True)[0]      # one host round trip per level; every per-level output is gathered with it
        out[level] = dict(valid=m, valid_idx=rows, intersection_points=pts[i].index_select(0, rows),
                          normals=(nrm[i].index_select(0, rows) if return_normals else None))
    return out
