"""Host side of the coarse stage's SDF regulariser kernels (csrc/sdf_regulariser.hip; C ABI: sgr_sample_transform_*,
sgr_smallest_axis_*, sgr_depth_lookup_*, sgr_sdf_field_*): one autograd Function per operation, each one forward and one backward
call.  `sugar_amd.sugar_patch.install_regulariser` binds them to the four methods of the reference's `SuGaR` class that the unmodified
coarse trainer calls (sugar_trainers/coarse_sdf.py:566-716):

    sample_transform   the arithmetic of SuGaR.sample_points_in_gaussians after its random draws      sugar_model.py:924-926
    smallest_axis      SuGaR.get_smallest_axis, and get_normals() of a model that is not mesh-bound   :930-968
    depth_lookup       SuGaR.get_points_depth_in_depth_map                                            :1318-1333
    sdf_field          SuGaR.get_field_values with beta_mode 'average', without sdf_grad              :1247-1307

GPU tensors only; the HIP library must be built.  Per-Gaussian gradients are written completely by the kernels (rows nothing references
are zero) and are bit-identical from run to run; the depth map's gradient is accumulated with float atomics, as torch's own
grid_sampler_2d_backward does, and is not."""
from __future__ import annotations

import torch

from . import _lib
from ._call import call, need_gpu, ptr


def _f32c(t):
    return t if (t.dtype == torch.float32 and t.is_contiguous()) else t.contiguous().float()


def _plain(t):
    """a RowGatherTensor (what `patch_gathers` makes the SuGaR properties return) as the plain tensor it views; same autograd history"""
    return t.as_subclass(torch.Tensor) if type(t) is not torch.Tensor and isinstance(t, torch.Tensor) else t


class _SampleTransform(torch.autograd.Function):
    @staticmethod
    def forward(ctx, points, quaternions, scaling, idx, noise, factor):
        need_gpu("sample_transform", points=points, quaternions=quaternions, scaling=scaling, idx=idx, noise=noise)
        pts, q, s, eps = _f32c(points), _f32c(quaternions), _f32c(scaling), _f32c(noise)
        ix = idx.reshape(-1).contiguous().to(torch.int64)
        N, P, dev = ix.shape[0], pts.shape[0], pts.device
        out = torch.empty(N, 3, device=dev)
        call("sgr_sample_transform_forward", dev, N, P, ptr(ix), ptr(pts), ptr(q), ptr(s), ptr(eps), float(factor), ptr(out))
        ctx.save_for_backward(q, s, ix, eps)
        ctx.factor = float(factor)
        return out

    @staticmethod
    def backward(ctx, g):
        q, s, ix, eps = ctx.saved_tensors
        N, P, dev = ix.shape[0], q.shape[0], q.device
        g = _f32c(g)
        dpts, dq, ds = torch.empty(P, 3, device=dev), torch.empty(P, 4, device=dev), torch.empty(P, 3, device=dev)
        scratch = torch.empty(_lib.load().sgr_sample_transform_backward_scratch_bytes(N, P), dtype=torch.uint8, device=dev)
        call("sgr_sample_transform_backward", dev, N, P, ptr(ix), ptr(q), ptr(s), ptr(eps), ctx.factor, ptr(g), ptr(dpts), ptr(dq), ptr(ds),
             ptr(scratch))
        return dpts, dq, ds, None, None, None


class _SmallestAxis(torch.autograd.Function):
    @staticmethod
    def forward(ctx, quaternions, scaling):
        need_gpu("smallest_axis", quaternions=quaternions, scaling=scaling)
        q, s = _f32c(quaternions), _f32c(scaling)
        P, dev = q.shape[0], q.device
        axis = torch.empty(P, 3, device=dev)
        axis_idx = torch.empty(P, dtype=torch.int64, device=dev)
        call("sgr_smallest_axis_forward", dev, P, ptr(q), ptr(s), ptr(axis), ptr(axis_idx))
        ctx.save_for_backward(q, s)
        ctx.mark_non_differentiable(axis_idx)
        return axis, axis_idx

    @staticmethod
    def backward(ctx, g, _g_idx):
        q, s = ctx.saved_tensors
        P, dev = q.shape[0], q.device
        g = _f32c(g)
        dq = torch.empty(P, 4, device=dev)
        call("sgr_smallest_axis_backward", dev, P, ptr(q), ptr(s), ptr(g), ptr(dq))
        return dq, None


class _DepthLookup(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, points_cam, projection):
        need_gpu("depth_lookup", depth=depth, points_cam=points_cam, projection=projection)
        if depth.dim() != 2 or depth.dtype != torch.float32:
            raise RuntimeError("depth_lookup: depth must be a float32 [H, W] tensor (any strides)")
        pts = _f32c(points_cam.reshape(-1, 3))
        Pm = _f32c(projection.reshape(16))
        H, W = depth.shape
        M, dev = pts.shape[0], pts.device
        out = torch.empty(M, device=dev)
        call("sgr_depth_lookup_forward", dev, M, ptr(pts), ptr(Pm), ptr(depth), depth.stride(0), depth.stride(1), H, W, ptr(out))
        ctx.save_for_backward(depth, pts, Pm)     # (the strided view itself: never copied)
        ctx.pts_shape = points_cam.shape
        return out

    @staticmethod
    def backward(ctx, g):
        depth, pts, Pm = ctx.saved_tensors
        H, W = depth.shape
        M, dev = pts.shape[0], pts.device
        g = _f32c(g)
        ddepth = torch.empty(H, W, device=dev) if ctx.needs_input_grad[0] else None     # zeroed by the call
        dpts = torch.empty(M, 3, device=dev) if ctx.needs_input_grad[1] else None
        if ddepth is not None or dpts is not None:
            call("sgr_depth_lookup_backward", dev, M, ptr(pts), ptr(Pm), ptr(depth), depth.stride(0), depth.stride(1), H, W, ptr(g),
                 ptr(dpts), ptr(ddepth))
        return ddepth, (dpts.reshape(ctx.pts_shape) if dpts is not None else None), None


class _SdfField(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, nbr_idx, centers, inv_scaled_rot, strengths, min_scaling, density_factor, density_threshold, opacity_min_clamp):
        need_gpu("sdf_field", x=x, nbr_idx=nbr_idx, centers=centers, inv_scaled_rot=inv_scaled_rot, strengths=strengths,
                 min_scaling=min_scaling)
        P = centers.shape[0]
        xs, nb, ce = _f32c(x), nbr_idx.contiguous().to(torch.int64), _f32c(centers)
        Bm, st, ms = _f32c(inv_scaled_rot.reshape(P, 9)), _f32c(strengths.reshape(P)), _f32c(min_scaling.reshape(P))
        N, K = nb.shape
        dev = xs.device
        opac, dens = torch.empty(N, K, device=dev), torch.empty(N, device=dev)
        beta, sdf = torch.empty(N, device=dev), torch.empty(N, device=dev)
        packed = torch.empty(P, 16, device=dev)
        call("sgr_pack_gaussians", dev, P, ptr(ce), ptr(Bm), ptr(st), ptr(packed))
        consts = (float(density_factor), float(density_threshold), float(opacity_min_clamp))
        call("sgr_sdf_field_forward", dev, N, K, P, ptr(xs), ptr(nb), ptr(ce), ptr(Bm), ptr(st), ptr(ms), *consts, ptr(opac), ptr(dens),
             ptr(beta), ptr(sdf), ptr(packed))
        ctx.save_for_backward(xs, nb, ce, Bm, st, packed, dens, beta)
        ctx.consts = consts
        ctx.shapes = (inv_scaled_rot.shape, strengths.shape, min_scaling.shape)
        ctx.set_materialize_grads(False)
        return opac, dens, beta, sdf

    @staticmethod
    def backward(ctx, g_opac, g_dens, g_beta, g_sdf):
        xs, nb, ce, Bm, st, packed, dens, beta = ctx.saved_tensors
        N, K = nb.shape
        P, dev = ce.shape[0], xs.device
        go, gd, gb, gs = [(_f32c(g) if g is not None else None) for g in (g_opac, g_dens, g_beta, g_sdf)]
        dx = torch.empty(N, 3, device=dev) if ctx.needs_input_grad[0] else None
        dce, dB, dst, dms = (torch.empty(P, 3, device=dev), torch.empty(P, 9, device=dev), torch.empty(P, device=dev),
                             torch.empty(P, device=dev))
        scratch = torch.empty(_lib.load().sgr_sdf_field_backward_scratch_bytes(N, K, P), dtype=torch.uint8, device=dev)
        call("sgr_sdf_field_backward", dev, N, K, P, ptr(xs), ptr(nb), ptr(ce), ptr(Bm), ptr(st), *ctx.consts, ptr(dens), ptr(beta),
             ptr(go), ptr(gd), ptr(gb), ptr(gs), ptr(dx), ptr(dce), ptr(dB), ptr(dst), ptr(dms), ptr(scratch), ptr(packed))
        Bshape, sshape, mshape = ctx.shapes
        return dx, None, dce, dB.reshape(Bshape), dst.reshape(sshape), dms.reshape(mshape), None, None, None


def sample_transform(points, quaternions, scaling, idx, noise, factor: float = 1.0):
    """points[idx] + quaternion_apply(quaternions[idx], factor * scaling[idx] * noise)  (sugar_model.py:924-926): [N,3] from the
    per-Gaussian [P,3] / [P,4] / [P,3] tensors, int64 idx[N] and noise[N,3]; differentiable w.r.t. the three per-Gaussian tensors.
    The quaternions are used as given (pytorch3d's quaternion_apply does not normalise)."""
    return _SampleTransform.apply(_plain(points), _plain(quaternions), _plain(scaling), idx, noise, factor)


def smallest_axis(quaternions, scaling):
    """(axis[P,3], axis_idx[P] int64): the column of quaternion_to_matrix(quaternions) at the smallest scaling, the lowest index on
    ties (sugar_model.py:939-943); differentiable w.r.t. the quaternions."""
    return _SmallestAxis.apply(_plain(quaternions), _plain(scaling))


def depth_lookup(projection, depth, points_in_camera_space):
    """SuGaR.get_points_depth_in_depth_map (sugar_model.py:1318-1333) for a depth map that has the model's image size: `projection` is
    `fov_camera.get_projection_transform().get_matrix()` ([1,4,4] or [4,4], row vectors, on the device), `depth` a float32 [H,W] tensor
    of any strides (read in place), the points [M,3].  Differentiable w.r.t. the points and the depth map."""
    return _DepthLookup.apply(depth, points_in_camera_space, projection)


def sdf_field(x, nbr_idx, centers, inv_scaled_rot, strengths, min_scaling, density_factor: float = 1.0, density_threshold: float = 1.0,
              opacity_min_clamp: float = 1e-16):
    """(neighbor_opacities[N,K], density[N], beta[N], sdf[N]) of SuGaR.get_field_values with beta_mode 'average' (sugar_model.py:
    1266-1307; `density` is the value before the normalisation of the rows >= 1, as fields['density']).  `min_scaling` is
    `scaling.min(-1)[0]` ([P]); differentiable w.r.t. x, centers, inv_scaled_rot, strengths and min_scaling.  Rows with density >= 1
    get the reference's own sqrt(0) and its non-finite gradient."""
    return _SdfField.apply(_plain(x), nbr_idx, _plain(centers), _plain(inv_scaled_rot), _plain(strengths), _plain(min_scaling),
                           density_factor, density_threshold, opacity_min_clamp)
