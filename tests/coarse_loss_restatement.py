"""TEST INFRASTRUCTURE: the three operations of csrc/coarse_loss.hip and their composite written out as plain torch, statement by
statement after the coarse trainer (sugar_trainers/coarse_sdf.py:606-716; the 'density' branch is coarse_density.py:658-700 as well),
in whatever dtype the inputs have: float64 is the truth of the parity tests (tests/test_gpu_coarse_loss.py, the `yard_*` distances of
tests/golden/make_coarse_loss.py), float32 on the GPU is what the unmodified trainer executes today (scripts/coarse_loss_bench.py
times it).  Gradients come from autograd.  The trainer's method calls appear here as callables or as the restatements of
tests/sdf_regulariser_restatement.py (`depth_lookup` = SuGaR.get_points_depth_in_depth_map).

    surface_band        :610-622    estimation_losses   :644-686    better_normal_loss   :688-716    regulariser_terms   :606-716
"""
import torch

from tests import sdf_regulariser_restatement as rs


def view_points(world_to_view, x):
    """Transform3d.transform_points: [x 1] * M, divided by its w"""
    h = torch.cat((x, torch.ones_like(x[:, :1])), -1) @ world_to_view.reshape(4, 4).to(x.dtype)
    return h[:, :3] / h[:, 3:4]


def scalar_distance(a, b) -> float:
    """relative distance of two scalars, in float64"""
    a, b = float(torch.as_tensor(a).detach().double()), float(torch.as_tensor(b).detach().double())
    return abs(a - b) / max(abs(b), 1e-30)


def surface_band(points, quaternions, scaling, world_to_view, cam_center, projection, depth, threshold, lookup=rs.depth_lookup):
    """(close, std, map_z - z) of :610-622"""
    with torch.no_grad():
        to_camera = torch.nn.functional.normalize(cam_center.reshape(1, 3).to(points.dtype) - points, dim=-1)          # :612
        in_camera = view_points(world_to_view, points)                                                               # :613
        z = in_camera[..., 2] + 0.                                                                                   # :615
        map_z = lookup(projection, depth, in_camera)                                                                 # :616
        inverse = quaternions * quaternions.new_tensor([1.0, -1.0, -1.0, -1.0])                                      # quaternion_invert
        std = (scaling * rs.rotate(inverse, to_camera)).norm(dim=-1)                                                 # :618-620
        close = (map_z - z).abs() < threshold * std                                                                  # :622
    return close, std, map_z - z


def estimation_losses(samples, depth, world_to_view, projection, znear, *, mode="sdf", sdf=None, density=None, beta=None, scale=None,
                      std=None, sample_idx=None, clamp_max=float("inf"), with_estimation=True, with_surface=False,
                      squared_estimation=False, squared_surface=False, lookup=rs.depth_lookup):
    """(estimation, surface, M) of :644-686, with the trainer's boolean-mask compaction"""
    in_camera = view_points(world_to_view, samples)                                                                  # :646
    z = in_camera[..., 2] + 0.                                                                                       # :647
    proj_mask = z > znear                                                                                            # :648
    map_z = lookup(projection, depth, in_camera[proj_mask])                                                          # :649
    estimation = map_z - z[proj_mask]                                                                                # :650
    with torch.no_grad():
        sample_std = std.to(samples.dtype)[sample_idx][proj_mask] if std is not None else scale                      # :656-659
    est_loss = surf_loss = None
    if with_estimation:
        if mode == "sdf":
            values = sdf[proj_mask]                                                                                  # :663
            if squared_estimation:
                est_loss = ((values - estimation.abs()) / sample_std).pow(2)                                         # :665
            else:
                est_loss = (values - estimation.abs()).abs() / sample_std                                            # :667
            est_loss = est_loss.clamp(max=clamp_max).mean()                                                          # :668
        elif mode == "density":
            b, d = beta[proj_mask], density[proj_mask]                                                               # :670-671
            target = torch.exp(-0.5 * estimation.pow(2) / b.pow(2))                                                  # :672
            est_loss = ((d - target).pow(2) if squared_estimation else (d - target).abs()).mean()                    # :673-677
        else:
            raise ValueError(f"Unknown sdf_estimation_mode: {mode}")
    if with_surface:
        if squared_surface:
            surf_loss = (estimation / sample_std).pow(2)                                                             # :683
        else:
            surf_loss = estimation.abs() / sample_std                                                                # :685
        surf_loss = surf_loss.clamp(max=clamp_max).mean()                                                            # :686
    return est_loss, surf_loss, proj_mask.sum()


def better_normal_loss(samples, sample_idx, knn_idx, normals, points, min_scaling, opacities, through_normal_only=True):
    """:688-716; `normals` is get_normals(), `min_scaling` is scaling.min(-1)[0]"""
    closest = knn_idx[sample_idx]                                                                                    # :691
    closest_min_scaling = min_scaling[closest].detach().view(len(samples), -1)                                       # :693
    closest_normals = normals[closest]                                                                               # :696
    own_normals = normals[sample_idx]                                                                                # :697
    closest_normals = closest_normals * torch.sign((closest_normals * own_normals[:, None]).sum(dim=-1, keepdim=True)).detach()   # :698-700
    opac = opacities.detach()                                                                                        # :703
    weights = ((samples[:, None] - points[closest]) * closest_normals).sum(dim=-1).abs()                             # :704
    if through_normal_only:
        weights = weights.detach()                                                                                   # :705-706
    weights = opac * weights / closest_min_scaling.clamp(min=1e-6) ** 2                                              # :707
    weights_sum = weights.sum(dim=-1).detach()                                                                       # :710
    weights = weights / weights_sum.unsqueeze(-1).clamp(min=1e-6)                                                    # :711
    return (own_normals - (weights[..., None] * closest_normals).sum(dim=-2)).pow(2).sum(dim=-1).mean()             # :714-716


def regulariser_terms(sugar, fov_camera, depth, visibility_filter, *, dtype=None, sdf_estimation_mode="sdf", use_sdf_estimation_loss=True,
                      enforce_samples_to_be_on_surface=False, squared_sdf_estimation_loss=False, squared_samples_on_surface_loss=False,
                      normalize_by_sdf_std=False, close_gaussian_threshold=2.0, use_sdf_better_normal_loss=True,
                      sdf_better_normal_gradient_through_normal_only=True, density_factor=1.0 / 16.0, density_threshold=1.0,
                      n_samples_for_sdf_regularization=1_000_000, sdf_sampling_scale_factor=1.5, sdf_sampling_proportional_to_volume=False,
                      cameras_spatial_extent=None, lookup=rs.depth_lookup):
    """:606-716 for one camera.  The method calls go to `sugar` (in its own dtype); the inline statements run in `dtype` (None: the
    model's) on casts of what the methods returned, so that float64 measures the inline arithmetic alone.  The band mask is always
    formed in the model's dtype: it selects the draws."""
    cast = (lambda t: t) if dtype is None else (lambda t: t.to(dtype))
    world_to_view = fov_camera.get_world_to_view_transform().get_matrix()
    projection = fov_camera.get_projection_transform().get_matrix()
    plain = lambda t: t.as_subclass(torch.Tensor)
    close, std, _ = surface_band(plain(sugar.points), plain(sugar.quaternions), plain(sugar.scaling), world_to_view,
                                 fov_camera.get_camera_center(), projection, depth.detach(), close_gaussian_threshold, lookup=lookup)
    sampling_mask = visibility_filter * close                                                                        # :623
    samples, sample_idx = sugar.sample_points_in_gaussians(num_samples=n_samples_for_sdf_regularization,
                                                           sampling_scale_factor=sdf_sampling_scale_factor, mask=sampling_mask,
                                                           probabilities_proportional_to_volume=sdf_sampling_proportional_to_volume)
    estimate = use_sdf_estimation_loss or enforce_samples_to_be_on_surface
    fields = sugar.get_field_values(samples, sample_idx, return_sdf=estimate and sdf_estimation_mode == "sdf",
                                    density_threshold=density_threshold, density_factor=density_factor, return_sdf_grad=False,
                                    sdf_grad_max_value=10., return_closest_gaussian_opacities=use_sdf_better_normal_loss,
                                    return_beta=estimate and sdf_estimation_mode == "density")                       # :635-642
    out = {"n_samples": samples.shape[0], "close": close, "std": std, "samples": samples, "sample_idx": sample_idx}
    opt = lambda k: cast(plain(fields[k])) if k in fields else None
    if estimate:
        extent = float(sugar.get_cameras_spatial_extent() if cameras_spatial_extent is None else cameras_spatial_extent)
        est, surf, M = estimation_losses(cast(plain(samples)), cast(depth), cast(world_to_view), cast(projection), cast(fov_camera.znear),
                                         mode=sdf_estimation_mode, sdf=opt("sdf"), density=opt("density"), beta=opt("beta"),
                                         scale=extent / 10., std=cast(std) if normalize_by_sdf_std else None, sample_idx=sample_idx,
                                         clamp_max=10. * extent, with_estimation=use_sdf_estimation_loss,
                                         with_surface=enforce_samples_to_be_on_surface, squared_estimation=squared_sdf_estimation_loss,
                                         squared_surface=squared_samples_on_surface_loss, lookup=lookup)
        if use_sdf_estimation_loss:
            out["sdf_estimation_loss"] = est
        if enforce_samples_to_be_on_surface:
            out["samples_on_surface_loss"] = surf
        out["n_projected"] = M
    if use_sdf_better_normal_loss:
        min_scaling = cast(plain(sugar.scaling)).min(dim=-1)[0]
        out["sdf_better_normal_loss"] = better_normal_loss(cast(plain(samples)), sample_idx, sugar.knn_idx,
                                                           cast(plain(sugar.get_normals(estimate_from_points=False))),
                                                           cast(plain(sugar.points)), min_scaling, opt("closest_gaussian_opacities"),
                                                           sdf_better_normal_gradient_through_normal_only)
    return out
