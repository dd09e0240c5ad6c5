"""Host side of the coarse trainers' inline loss terms (csrc/coarse_loss.hip; C ABI: sgr_surface_band, sgr_estimation_loss_*,
sgr_projection_loss_*, sgr_better_normal_*): the statements that sugar_trainers/coarse_sdf.py:606-716 (and coarse_density.py:610-730) write between the calls
of `sample_points_in_gaussians`, `get_field_values` and `get_normals`, as three operations and one composite:

    surface_band        the close-to-surface mask of the Gaussians and their view-dependent std                 coarse_sdf.py:610-623
    estimation_losses   the SDF-estimation (mode 'sdf' or 'density') and samples-on-surface means over the
                        samples in front of the camera, and their count M                                       :644-686
    better_normal_loss  the "better normal" mean over the samples                                               :688-716
    regulariser_terms   the whole of :606-716 for any object with SuGaR's attributes                            :606-716
    opacity_entropy     the entropy term the loop adds before the regulariser starts (sgr_opacity_entropy_*)    :543-551
    projection_estimation_losses   the same two means with est = <x - mu_g, n_g> of the sample's own Gaussian
                        (`use_projection_as_estimation`, coarse_density.py's default), over every sample        coarse_density.py:651-700
    density_regulariser_terms      the whole of coarse_density.py:574-730 under that option: no camera, no depth  coarse_density.py:574-730

GPU tensors only; the HIP library must be built.  No operation synchronises with the host; camera matrices (pytorch3d's row vectors)
and `znear` are read on the device; the depth map is read through its strides.  The scalar means and every per-Gaussian gradient are
summed in a fixed order and are bit-identical from run to run; the depth map's gradient is accumulated with float atomics, as
`sdf_regulariser.depth_lookup`'s, and is not."""
from __future__ import annotations

import torch

from . import _lib
from ._call import call, need_gpu, ptr
from .sdf_regulariser import _f32c, _plain

_SQUARED_EST, _SQUARED_SURFACE, _WITH_EST, _WITH_SURFACE = 1, 2, 4, 8     # SGR_CL_* of include/sugar_raster.h
MODES = ("sdf", "density")


def _scratch(nbytes, dev):
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=dev)


def _mat16(m, what):
    if m.numel() != 16:
        raise RuntimeError(f"{what} must be one 4 x 4 matrix (row vectors), got shape {tuple(m.shape)}")
    return _f32c(m.detach().reshape(16))


def _depth2d(depth, what):
    if depth.dim() != 2 or depth.dtype != torch.float32:
        raise RuntimeError(f"{what}: depth must be a float32 [H, W] tensor (any strides)")
    return depth


def _idx(t):
    return t.contiguous().to(torch.int64)


def surface_band(points, quaternions, scaling, world_to_view, cam_center, projection, depth, threshold: float = 2.0):
    """(close[P] bool, std[P]) of coarse_sdf.py:610-623, without a graph: `std = |scaling * R(q)^T normalize(cam_center - points)|` for
    the unit `quaternions` the model hands out, `close = |map_z - z| < threshold * std` with z the centre's depth under `world_to_view`
    and map_z its lookup in `depth` ([H,W] float32, any strides) through `projection`.  The matrices are
    `fov_camera.get_world_to_view_transform().get_matrix()` / `.get_projection_transform().get_matrix()`, `cam_center` is
    `fov_camera.get_camera_center()`; all on the device."""
    need_gpu("surface_band", points=points, quaternions=quaternions, scaling=scaling, world_to_view=world_to_view, cam_center=cam_center,
             projection=projection, depth=depth)
    with torch.no_grad():
        pts, q, s = _f32c(_plain(points).detach()), _f32c(_plain(quaternions).detach()), _f32c(_plain(scaling).detach())
        V, Pm, cc = _mat16(world_to_view, "world_to_view"), _mat16(projection, "projection"), _f32c(cam_center.detach().reshape(-1))
        if cc.numel() != 3:
            raise RuntimeError("surface_band: cam_center must hold one camera's 3 coordinates")
        d = _depth2d(depth.detach(), "surface_band")
        P, dev = pts.shape[0], pts.device
        if q.shape != (P, 4) or s.shape != (P, 3) or pts.shape != (P, 3):
            raise RuntimeError("surface_band: expected points[P,3], quaternions[P,4], scaling[P,3]")
        close, std = torch.empty(P, dtype=torch.bool, device=dev), torch.empty(P, device=dev)
        H, W = d.shape
        call("sgr_surface_band", dev, P, ptr(pts), ptr(q), ptr(s), ptr(V), ptr(cc), ptr(Pm), ptr(d), d.stride(0), d.stride(1), H, W,
             float(threshold), ptr(close), ptr(std))
    return close, std


class _EstimationLosses(torch.autograd.Function):
    @staticmethod
    def forward(ctx, samples, field, beta, depth, sample_idx, std, V, Pm, znear, mode, flags, scale, clamp_max):
        x = _f32c(samples)
        N, dev = x.shape[0], x.device
        f = _f32c(field.reshape(-1)) if field is not None else None
        b = _f32c(beta.reshape(-1)) if beta is not None else None
        ix = _idx(sample_idx.reshape(-1)) if std is not None else None
        sd = _f32c(std.detach().reshape(-1)) if std is not None else None
        P = sd.shape[0] if sd is not None else 0
        H, W = depth.shape
        out = torch.zeros(2, device=dev)
        M = torch.empty((), dtype=torch.int64, device=dev)
        scratch = _scratch(_lib.load().sgr_estimation_loss_scratch_bytes(N), dev)
        head = (N, P, mode, flags, ptr(x), ptr(f), ptr(b), ptr(ix), ptr(sd), scale, clamp_max, ptr(V), ptr(Pm), ptr(znear))
        call("sgr_estimation_loss_forward", dev, *head, ptr(depth), depth.stride(0), depth.stride(1), H, W,
             ptr(out[0:]) if flags & _WITH_EST else None, ptr(out[1:]) if flags & _WITH_SURFACE else None, ptr(M), ptr(scratch))
        ctx.save_for_backward(x, f, b, depth, ix, sd, V, Pm, znear, M)     # (the strided depth view itself: never copied)
        ctx.consts = (N, P, mode, flags, scale, clamp_max)
        ctx.shapes = (samples.shape, field.shape if field is not None else None, beta.shape if beta is not None else None)
        ctx.mark_non_differentiable(M)
        return out[0], out[1], M

    @staticmethod
    def backward(ctx, g_est, g_surf, _g_M):
        x, f, b, depth, ix, sd, V, Pm, znear, M = ctx.saved_tensors
        N, P, mode, flags, scale, clamp_max = ctx.consts
        dev = x.device
        H, W = depth.shape
        need = ctx.needs_input_grad
        dx = torch.empty(N, 3, device=dev) if need[0] else None
        df = torch.empty(N, device=dev) if need[1] and f is not None else None
        db = torch.empty(N, device=dev) if need[2] and b is not None and mode == 1 else None
        dd = torch.empty(H, W, device=dev) if need[3] else None                 # zeroed by the call
        if dx is not None or df is not None or db is not None or dd is not None:
            head = (N, P, mode, flags, ptr(x), ptr(f), ptr(b), ptr(ix), ptr(sd), scale, clamp_max, ptr(V), ptr(Pm), ptr(znear))
            call("sgr_estimation_loss_backward", dev, *head, ptr(depth), depth.stride(0), depth.stride(1), H, W, ptr(M),
                 ptr(_f32c(g_est)), ptr(_f32c(g_surf)), ptr(df), ptr(db), ptr(dx), ptr(dd))
        s_shape, f_shape, b_shape = ctx.shapes
        if need[2] and b is not None and db is None:
            db = torch.zeros(N, device=dev)                                     # mode 'sdf' does not read beta
        return (dx.reshape(s_shape) if dx is not None else None, df.reshape(f_shape) if df is not None else None,
                db.reshape(b_shape) if db is not None else None, dd) + (None,) * 9


def estimation_losses(samples, depth, world_to_view, projection, znear, *, mode: str = "sdf", sdf=None, density=None, beta=None,
                      scale=None, std=None, sample_idx=None, clamp_max: float = float("inf"), with_estimation: bool = True,
                      with_surface: bool = False, squared_estimation: bool = False, squared_surface: bool = False):
    """(estimation, surface, M) of coarse_sdf.py:644-686: the means of the per-sample terms over the samples with z > znear, as 0-dim
    device tensors (None for a term that was not asked for), and their count M (int64, 0-dim).  `mode='sdf'` reads `sdf[N]`,
    `mode='density'` reads `density[N]` and `beta[N]`.  The samples' scale is `std[sample_idx]` when `std` ([P], e.g. `surface_band`'s;
    no gradient) is given, the number `scale` otherwise.  `znear`: the camera's tensor (read on the device) or a number.
    Differentiable w.r.t. samples, sdf / density, beta and the depth map."""
    if mode not in MODES:
        raise ValueError(f"Unknown sdf_estimation_mode: {mode}")
    if not (with_estimation or with_surface):
        raise ValueError("estimation_losses: neither term was asked for")
    field = (sdf if mode == "sdf" else density) if with_estimation else None
    b = beta if (with_estimation and mode == "density") else None
    tensors = dict(samples=samples, depth=depth, world_to_view=world_to_view, projection=projection)
    if with_estimation:
        if field is None or (mode == "density" and b is None):
            raise ValueError("estimation_losses: mode 'sdf' needs sdf=, mode 'density' needs density= and beta=")
        tensors["sdf" if mode == "sdf" else "density"] = field
        if b is not None:
            tensors["beta"] = b
    if std is not None:
        if sample_idx is None:
            raise ValueError("estimation_losses: std= needs sample_idx=")
        tensors.update(std=std, sample_idx=sample_idx)
    elif scale is None:
        raise ValueError("estimation_losses: give the samples' scale as scale= (a number) or std= with sample_idx=")
    need_gpu("estimation_losses", **tensors)
    if samples.dim() != 2 or samples.shape[1] != 3 or samples.shape[0] < 1:
        raise RuntimeError("estimation_losses: samples must be [N, 3] with N >= 1")
    N, dev = samples.shape[0], samples.device
    for name in ("sdf", "density", "beta", "sample_idx"):
        if name in tensors and tensors[name].numel() != N:
            raise RuntimeError(f"estimation_losses: {name} must have one entry per sample")
    depth = _depth2d(_plain(depth), "estimation_losses")
    V, Pm = _mat16(world_to_view, "world_to_view"), _mat16(projection, "projection")
    zn = torch.as_tensor(znear, dtype=torch.float32, device=dev).detach().reshape(-1)[:1].contiguous()
    flags = ((_WITH_EST if with_estimation else 0) | (_WITH_SURFACE if with_surface else 0)
             | (_SQUARED_EST if squared_estimation else 0) | (_SQUARED_SURFACE if squared_surface else 0))
    est, surf, M = _EstimationLosses.apply(_plain(samples), _plain(field) if field is not None else None,
                                           _plain(b) if b is not None else None, depth, sample_idx, std, V, Pm, zn, MODES.index(mode), flags,
                                           float(scale) if std is None else 0.0, float(clamp_max))
    return (est if with_estimation else None), (surf if with_surface else None), M


class _ProjectionLosses(torch.autograd.Function):
    @staticmethod
    def forward(ctx, samples, field, beta, points, normals, sample_idx, mode, flags, scale, clamp_max):
        x, pts, nrm = _f32c(samples), _f32c(points), _f32c(normals)
        N, P, dev = x.shape[0], pts.shape[0], x.device
        f = _f32c(field.reshape(-1)) if field is not None else None
        b = _f32c(beta.reshape(-1)) if beta is not None else None
        ix = _idx(sample_idx.reshape(-1))
        out = torch.zeros(2, device=dev)
        scratch = _scratch(_lib.load().sgr_projection_loss_scratch_bytes(N), dev)
        call("sgr_projection_loss_forward", dev, N, P, mode, flags, ptr(x), ptr(ix), ptr(pts), ptr(nrm), ptr(f), ptr(b), scale, clamp_max,
             ptr(out[0:]) if flags & _WITH_EST else None, ptr(out[1:]) if flags & _WITH_SURFACE else None, ptr(scratch))
        ctx.save_for_backward(x, f, b, pts, nrm, ix)
        ctx.consts = (N, P, mode, flags, scale, clamp_max)
        ctx.shapes = (samples.shape, field.shape if field is not None else None, beta.shape if beta is not None else None)
        return out[0], out[1]

    @staticmethod
    def backward(ctx, g_est, g_surf):
        x, f, b, pts, nrm, ix = ctx.saved_tensors
        N, P, mode, flags, scale, clamp_max = ctx.consts
        dev = x.device
        need = ctx.needs_input_grad
        dx = torch.empty(N, 3, device=dev) if need[0] else None
        df = torch.empty(N, device=dev) if need[1] and f is not None else None
        db = torch.empty(N, device=dev) if need[2] and b is not None and mode == 1 else None
        dp = torch.empty(P, 3, device=dev) if need[3] else None
        dn = torch.empty(P, 3, device=dev) if need[4] else None
        if any(t is not None for t in (dx, df, db, dp, dn)):
            scratch = _scratch(_lib.load().sgr_projection_loss_backward_scratch_bytes(N, P), dev)
            call("sgr_projection_loss_backward", dev, N, P, mode, flags, ptr(x), ptr(ix), ptr(pts), ptr(nrm), ptr(f), ptr(b), scale, clamp_max,
                 ptr(_f32c(g_est)), ptr(_f32c(g_surf)), ptr(df), ptr(db), ptr(dx), ptr(dp), ptr(dn), ptr(scratch))
        s_shape, f_shape, b_shape = ctx.shapes
        if need[2] and b is not None and db is None:
            db = torch.zeros(N, device=dev)                                     # mode 'sdf' does not read beta
        return (dx.reshape(s_shape) if dx is not None else None, df.reshape(f_shape) if df is not None else None,
                db.reshape(b_shape) if db is not None else None, dp, dn) + (None,) * 5


def projection_estimation_losses(samples, sample_idx, points, normals, *, mode: str = "density", sdf=None, density=None, beta=None,
                                 scale=None, clamp_max: float = float("inf"), with_estimation: bool = True, with_surface: bool = False,
                                 squared_estimation: bool = False, squared_surface: bool = False):
    """(estimation, surface) of coarse_density.py:651-700 with `use_projection_as_estimation`: the signed distance estimate of a sample
    is its offset from its own Gaussian's centre along that Gaussian's normal, `est = <samples - points[sample_idx], normals[sample_idx]>`,
    every sample counts, and the terms are `estimation_losses`'s: `mode='density'` reads `density[N]` and `beta[N]`, `mode='sdf'` reads
    `sdf[N]` and the number `scale`; the on-surface term needs `scale` too.  Returns the two means over all N samples as 0-dim device
    tensors (None for a term that was not asked for).  Differentiable w.r.t. samples, sdf / density, beta, points and normals; the
    per-Gaussian gradients are summed in a fixed order and every result is bit-identical from run to run.  N < 2^32 - 1."""
    if mode not in MODES:
        raise ValueError(f"Unknown sdf_estimation_mode: {mode}")
    if not (with_estimation or with_surface):
        raise ValueError("projection_estimation_losses: neither term was asked for")
    field = (sdf if mode == "sdf" else density) if with_estimation else None
    b = beta if (with_estimation and mode == "density") else None
    tensors = dict(samples=samples, sample_idx=sample_idx, points=points, normals=normals)
    if with_estimation:
        if field is None or (mode == "density" and b is None):
            raise ValueError("projection_estimation_losses: mode 'sdf' needs sdf=, mode 'density' needs density= and beta=")
        tensors["sdf" if mode == "sdf" else "density"] = field
        if b is not None:
            tensors["beta"] = b
    if scale is None and (with_surface or (with_estimation and mode == "sdf")):
        raise ValueError("projection_estimation_losses: give the samples' scale as scale= (a number)")
    need_gpu("projection_estimation_losses", **tensors)
    if samples.dim() != 2 or samples.shape[1] != 3 or samples.shape[0] < 1:
        raise RuntimeError("projection_estimation_losses: samples must be [N, 3] with N >= 1")
    N = samples.shape[0]
    if points.dim() != 2 or points.shape[1] != 3 or points.shape[0] < 1 or normals.shape != points.shape:
        raise RuntimeError("projection_estimation_losses: expected points[P,3] and normals[P,3] with P >= 1")
    for name in ("sdf", "density", "beta", "sample_idx"):
        if name in tensors and tensors[name].numel() != N:
            raise RuntimeError(f"projection_estimation_losses: {name} must have one entry per sample")
    if N >= 2 ** 32 - 1:
        raise RuntimeError("projection_estimation_losses: N must stay below 2^32 - 1")
    flags = ((_WITH_EST if with_estimation else 0) | (_WITH_SURFACE if with_surface else 0)
             | (_SQUARED_EST if squared_estimation else 0) | (_SQUARED_SURFACE if squared_surface else 0))
    est, surf = _ProjectionLosses.apply(_plain(samples), _plain(field) if field is not None else None, _plain(b) if b is not None else None,
                                        _plain(points), _plain(normals), sample_idx, MODES.index(mode), flags,
                                        float(scale) if scale is not None else 1.0, float(clamp_max))
    return (est if with_estimation else None), (surf if with_surface else None)


class _BetterNormal(torch.autograd.Function):
    @staticmethod
    def forward(ctx, samples, normals, points, sample_idx, knn_idx, min_scaling, opacities, only):
        x, nrm, pts = _f32c(samples), _f32c(normals), _f32c(points)
        ix, knn = _idx(sample_idx.reshape(-1)), _idx(knn_idx)
        ms, op = _f32c(min_scaling.detach().reshape(-1)), _f32c(opacities.detach())
        N, (P, K), dev = x.shape[0], knn.shape, x.device
        loss = torch.empty((), device=dev)
        scratch = _scratch(_lib.load().sgr_better_normal_forward_scratch_bytes(N, K), dev)
        call("sgr_better_normal_forward", dev, N, K, P, ptr(x), ptr(ix), ptr(knn), ptr(nrm), ptr(pts), ptr(ms), ptr(op), ptr(loss), ptr(scratch))
        ctx.save_for_backward(x, ix, knn, nrm, pts, ms, op)
        ctx.only = bool(only)
        return loss

    @staticmethod
    def backward(ctx, g):
        x, ix, knn, nrm, pts, ms, op = ctx.saved_tensors
        N, (P, K), dev, only = x.shape[0], knn.shape, x.device, ctx.only
        dn = torch.empty(P, 3, device=dev)
        dp = None if only else torch.empty(P, 3, device=dev)
        dx = None if only else torch.empty(N, 3, device=dev)
        scratch = _scratch(_lib.load().sgr_better_normal_backward_scratch_bytes(N, K, P, int(only)), dev)
        call("sgr_better_normal_backward", dev, N, K, P, ptr(x), ptr(ix), ptr(knn), ptr(nrm), ptr(pts), ptr(ms), ptr(op), int(only),
             ptr(_f32c(g)), ptr(dn), ptr(dp), ptr(dx), ptr(scratch))
        return dx, dn, dp, None, None, None, None, None


def better_normal_loss(samples, sample_idx, knn_idx, normals, points, min_scaling, opacities, through_normal_only: bool = True):
    """The "better normal" loss of coarse_sdf.py:688-716 as a 0-dim device tensor: samples[N,3], sample_idx[N], knn_idx[P,K],
    normals[P,3] (`get_normals()`), points[P,3], min_scaling[P] (`scaling.min(-1)[0]`) and opacities[N,K] (the field's
    `closest_gaussian_opacities`); the last two carry no gradient, as in the trainer.  With `through_normal_only` only the normals get
    a gradient; without it the samples and the points do too.  N * (K + 1) < 2^32."""
    need_gpu("better_normal_loss", samples=samples, sample_idx=sample_idx, knn_idx=knn_idx, normals=normals, points=points,
             min_scaling=min_scaling, opacities=opacities)
    if knn_idx.dim() != 2 or samples.dim() != 2 or samples.shape[1] != 3 or samples.shape[0] < 1:
        raise RuntimeError("better_normal_loss: samples must be [N, 3] with N >= 1 and knn_idx [P, K]")
    N, (P, K) = samples.shape[0], knn_idx.shape
    if (normals.shape != (P, 3) or points.shape != (P, 3) or min_scaling.numel() != P or opacities.shape != (N, K)
            or sample_idx.numel() != N):
        raise RuntimeError("better_normal_loss: expected normals[P,3], points[P,3], min_scaling[P], opacities[N,K], sample_idx[N]")
    if N * (K + 1) >= 2 ** 32:
        raise RuntimeError("better_normal_loss: N * (K + 1) must stay below 2^32")
    return _BetterNormal.apply(_plain(samples), _plain(normals), _plain(points), sample_idx, knn_idx, _plain(min_scaling), opacities,
                               through_normal_only)


class _OpacityEntropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, opacities, visible):
        o = _f32c(opacities.reshape(-1))
        vis = visible.reshape(-1).contiguous()
        P, dev = o.shape[0], o.device
        loss = torch.empty((), device=dev)
        count = torch.empty((), dtype=torch.int64, device=dev)
        scratch = _scratch(_lib.load().sgr_opacity_entropy_scratch_bytes(P), dev)
        call("sgr_opacity_entropy_forward", dev, P, ptr(o), ptr(vis), ptr(loss), ptr(count), ptr(scratch))
        ctx.save_for_backward(o, vis, count)
        ctx.shape = opacities.shape
        return loss

    @staticmethod
    def backward(ctx, g):
        o, vis, count = ctx.saved_tensors
        P, dev = o.shape[0], o.device
        do = torch.empty(P, device=dev)
        call("sgr_opacity_entropy_backward", dev, P, ptr(o), ptr(vis), ptr(count), ptr(_f32c(g)), ptr(do))
        return do.reshape(ctx.shape), None


def opacity_entropy(opacities, visible):
    """The entropy term of coarse_sdf.py:543-551 as a 0-dim device tensor:
    `(-o * log(o + 1e-10) - (1 - o) * log(1 - o + 1e-10))[visible].mean()` for opacities [P,1] or [P] and the bool [P] mask `visible`
    (the trainer's `radii > 0`).  The visible rows are counted on the device; with none the value is NaN (torch's mean of an empty
    tensor) and the gradient zero.  Differentiable w.r.t. the opacities: every row of the gradient is written, zero where invisible."""
    need_gpu("opacity_entropy", opacities=opacities, visible=visible)
    P = visible.numel()
    if visible.dtype != torch.bool or opacities.numel() != P or P < 1 or opacities.dim() > 2:
        raise RuntimeError("opacity_entropy: expected opacities[P,1] or [P] and a bool visible[P], P >= 1")
    return _OpacityEntropy.apply(_plain(opacities), visible)


def regulariser_terms(sugar, fov_camera, depth, visibility_filter, *, sdf_estimation_mode: str = "sdf",
                      use_sdf_estimation_loss: bool = True, enforce_samples_to_be_on_surface: bool = False,
                      squared_sdf_estimation_loss: bool = False, squared_samples_on_surface_loss: bool = False,
                      normalize_by_sdf_std: bool = False, sample_only_in_gaussians_close_to_surface: bool = True,
                      close_gaussian_threshold: float = 2.0, use_projection_as_estimation: bool = False,
                      use_sdf_better_normal_loss: bool = True, sdf_better_normal_gradient_through_normal_only: bool = True,
                      density_factor: float = 1.0 / 16.0, density_threshold: float = 1.0,
                      n_samples_for_sdf_regularization: int = 1_000_000, sdf_sampling_scale_factor: float = 1.5,
                      sdf_sampling_proportional_to_volume: bool = False, cameras_spatial_extent=None):
    """coarse_sdf.py:606-716 for one camera: the band mask, `sugar.sample_points_in_gaussians` (its draws and its `n > 0` check stay its
    own), `sugar.get_field_values`, `sugar.get_normals`, then `estimation_losses` and `better_normal_loss`.  `sugar` is any object with
    SuGaR's attributes (points, scaling, quaternions, knn_idx and the three methods); `depth` the [H,W] depth render (requiring grad or
    not), `visibility_filter` the bool [P] mask of the Gaussians in view.  The options carry the trainer's names and defaults.

    Returns a dict of the UNWEIGHTED terms as 0-dim device tensors -- 'sdf_estimation_loss', 'samples_on_surface_loss',
    'sdf_better_normal_loss', each only when asked for -- plus 'n_projected' (M, int64) and 'n_samples'; the caller applies its
    factors.  `cameras_spatial_extent`: `sugar.get_cameras_spatial_extent()` (a number; that method reads the device) -- asked of
    `sugar` once when not given."""
    if use_projection_as_estimation:
        raise NotImplementedError("regulariser_terms: use_projection_as_estimation=True is not implemented")
    if not sample_only_in_gaussians_close_to_surface:
        raise NotImplementedError("regulariser_terms: sample_only_in_gaussians_close_to_surface=False is not implemented "
                                  "(the reference raises there too, coarse_sdf.py:652-653)")
    if getattr(sugar, "beta_mode", "average") not in (None, "average"):
        raise NotImplementedError(f"regulariser_terms: beta_mode {sugar.beta_mode!r} is not implemented, only 'average'")
    if sdf_estimation_mode not in MODES:
        raise ValueError(f"Unknown sdf_estimation_mode: {sdf_estimation_mode}")
    estimate = use_sdf_estimation_loss or enforce_samples_to_be_on_surface
    if not (estimate or use_sdf_better_normal_loss):
        raise ValueError("regulariser_terms: no term was asked for")
    need_gpu("regulariser_terms", points=sugar.points, depth=depth, visibility_filter=visibility_filter)
    world_to_view = fov_camera.get_world_to_view_transform().get_matrix()
    projection = fov_camera.get_projection_transform().get_matrix()
    close, std = surface_band(sugar.points, sugar.quaternions, sugar.scaling, world_to_view, fov_camera.get_camera_center(), projection,
                              depth, close_gaussian_threshold)                                                  # :610-622
    sampling_mask = visibility_filter * close                                                                   # :623
    samples, sample_idx = sugar.sample_points_in_gaussians(num_samples=n_samples_for_sdf_regularization,
                                                           sampling_scale_factor=sdf_sampling_scale_factor, mask=sampling_mask,
                                                           probabilities_proportional_to_volume=sdf_sampling_proportional_to_volume)
    fields = sugar.get_field_values(samples, sample_idx,
                                    return_sdf=estimate and sdf_estimation_mode == "sdf", density_threshold=density_threshold,
                                    density_factor=density_factor, return_sdf_grad=False, sdf_grad_max_value=10.,
                                    return_closest_gaussian_opacities=use_sdf_better_normal_loss,
                                    return_beta=estimate and sdf_estimation_mode == "density")                  # :635-642
    out = {"n_samples": samples.shape[0]}
    if estimate:
        extent = float(sugar.get_cameras_spatial_extent() if cameras_spatial_extent is None else cameras_spatial_extent)
        est, surf, M = estimation_losses(samples, depth, world_to_view, projection, fov_camera.znear, mode=sdf_estimation_mode,
                                         sdf=fields.get("sdf"), density=fields.get("density"), beta=fields.get("beta"),
                                         scale=extent / 10., std=std if normalize_by_sdf_std else None, sample_idx=sample_idx,
                                         clamp_max=10. * extent, with_estimation=use_sdf_estimation_loss,
                                         with_surface=enforce_samples_to_be_on_surface, squared_estimation=squared_sdf_estimation_loss,
                                         squared_surface=squared_samples_on_surface_loss)                       # :644-686
        if use_sdf_estimation_loss:
            out["sdf_estimation_loss"] = est
        if enforce_samples_to_be_on_surface:
            out["samples_on_surface_loss"] = surf
        out["n_projected"] = M
    if use_sdf_better_normal_loss:
        min_scaling = _plain(sugar.scaling).detach().min(dim=-1)[0]                                             # :693
        out["sdf_better_normal_loss"] = better_normal_loss(samples, sample_idx, sugar.knn_idx, sugar.get_normals(estimate_from_points=False),
                                                           sugar.points, min_scaling, fields["closest_gaussian_opacities"],
                                                           sdf_better_normal_gradient_through_normal_only)       # :688-716
    return out


def density_regulariser_terms(sugar, visibility_filter, *, sdf_estimation_mode: str = "density", use_sdf_estimation_loss: bool = True,
                              enforce_samples_to_be_on_surface: bool = False, squared_sdf_estimation_loss: bool = False,
                              squared_samples_on_surface_loss: bool = False, use_sdf_better_normal_loss: bool = True,
                              sdf_better_normal_gradient_through_normal_only: bool = True, density_factor: float = 1.0,
                              density_threshold: float = 1.0, n_samples_for_sdf_regularization: int = 1_000_000,
                              sdf_sampling_scale_factor: float = 1.5, sdf_sampling_proportional_to_volume: bool = False,
                              cameras_spatial_extent=None):
    """coarse_density.py:574-730 for one camera with `use_projection_as_estimation=True` (that trainer's default): the sampling mask
    is `visibility_filter` alone (the bool [P] `radii > 0`; no band, no depth render, no camera), then
    `sugar.sample_points_in_gaussians`, `sugar.get_field_values`, `sugar.get_normals`, `projection_estimation_losses` and
    `better_normal_loss`.  `sugar` is any object with SuGaR's attributes, as for `regulariser_terms`; the options carry the trainer's
    names and coarse_density.py's defaults (`normalize_by_sdf_std` does not exist here: the reference forces it off, :664-667).

    Returns a dict of the UNWEIGHTED terms as 0-dim device tensors -- 'sdf_estimation_loss', 'samples_on_surface_loss',
    'sdf_better_normal_loss', each only when asked for -- plus 'n_samples'; the caller applies its factors."""
    if getattr(sugar, "beta_mode", "average") not in (None, "average"):
        raise NotImplementedError(f"density_regulariser_terms: beta_mode {sugar.beta_mode!r} is not implemented, only 'average'")
    if sdf_estimation_mode not in MODES:
        raise ValueError(f"Unknown sdf_estimation_mode: {sdf_estimation_mode}")
    estimate = use_sdf_estimation_loss or enforce_samples_to_be_on_surface
    if not (estimate or use_sdf_better_normal_loss):
        raise ValueError("density_regulariser_terms: no term was asked for")
    need_gpu("density_regulariser_terms", points=sugar.points, visibility_filter=visibility_filter)
    samples, sample_idx = sugar.sample_points_in_gaussians(num_samples=n_samples_for_sdf_regularization,
                                                           sampling_scale_factor=sdf_sampling_scale_factor, mask=visibility_filter,
                                                           probabilities_proportional_to_volume=sdf_sampling_proportional_to_volume)   # :634-639
    fields = sugar.get_field_values(samples, sample_idx,
                                    return_sdf=estimate and sdf_estimation_mode == "sdf", density_threshold=density_threshold,
                                    density_factor=density_factor, return_sdf_grad=False, sdf_grad_max_value=10.,
                                    return_closest_gaussian_opacities=use_sdf_better_normal_loss,
                                    return_beta=estimate and sdf_estimation_mode == "density")                  # :642-649
    out = {"n_samples": samples.shape[0]}
    normals = sugar.get_normals(estimate_from_points=False)
    if estimate:
        extent = float(sugar.get_cameras_spatial_extent() if cameras_spatial_extent is None else cameras_spatial_extent)
        est, surf = projection_estimation_losses(samples, sample_idx, sugar.points, normals, mode=sdf_estimation_mode,
                                                 sdf=fields.get("sdf"), density=fields.get("density"), beta=fields.get("beta"),
                                                 scale=extent / 10., clamp_max=10. * extent, with_estimation=use_sdf_estimation_loss,
                                                 with_surface=enforce_samples_to_be_on_surface,
                                                 squared_estimation=squared_sdf_estimation_loss,
                                                 squared_surface=squared_samples_on_surface_loss)               # :651-700
        if use_sdf_estimation_loss:
            out["sdf_estimation_loss"] = est
        if enforce_samples_to_be_on_surface:
            out["samples_on_surface_loss"] = surf
    if use_sdf_better_normal_loss:
        min_scaling = _plain(sugar.scaling).detach().min(dim=-1)[0]                                             # :707
        out["sdf_better_normal_loss"] = better_normal_loss(samples, sample_idx, sugar.knn_idx, normals, sugar.points, min_scaling,
                                                           fields["closest_gaussian_opacities"],
                                                           sdf_better_normal_gradient_through_normal_only)       # :702-730
    return out
