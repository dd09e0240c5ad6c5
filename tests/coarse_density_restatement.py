"""TEST INFRASTRUCTURE: the statements of sugar_trainers/coarse_density.py:651-700 under `use_projection_as_estimation=True` (that
trainer's default) and their composite :574-730, written out as plain torch in whatever dtype the inputs have: float64 is the truth
of the parity tests (tests/test_gpu_coarse_density.py, the `yard_*` distances of tests/golden/make_coarse_density.py), float32 on
the GPU is what the unmodified trainer executes.  Gradients come from autograd.  The better-normal loss (:702-730) is
coarse_sdf.py's and is shared with tests/coarse_loss_restatement.py.

    projection_estimate   :654-656    projection_estimation_losses   :651-700    density_regulariser_terms   :574-730
"""
import torch

from tests.coarse_loss_restatement import better_normal_loss, scalar_distance  # noqa: F401  (shared with the SDF trainer's restatement)


def projection_estimate(samples, sample_idx, points, normals):
    """:655-656: the sample's offset from its own Gaussian's centre along that Gaussian's normal"""
    own_normals = normals[sample_idx]                                                                                # :655
    return ((samples - points[sample_idx]) * own_normals).sum(dim=-1)                                                # :656


def projection_estimation_losses(samples, sample_idx, points, normals, *, mode="density", sdf=None, density=None, beta=None, scale=None,
                                 clamp_max=float("inf"), with_estimation=True, with_surface=False, squared_estimation=False,
                                 squared_surface=False):
    """(estimation, surface) of :651-700; `proj_mask` is all ones (:654), so every mean is over all the samples"""
    estimation = projection_estimate(samples, sample_idx, points, normals)
    est_loss = surf_loss = None
    if with_estimation:
        if mode == "sdf":
            if squared_estimation:
                est_loss = ((sdf - estimation.abs()) / scale).pow(2)                                                 # :679
            else:
                est_loss = (sdf - estimation.abs()).abs() / scale                                                    # :681
            est_loss = est_loss.clamp(max=clamp_max).mean()                                                          # :682
        elif mode == "density":
            target = torch.exp(-0.5 * estimation.pow(2) / beta.pow(2))                                               # :686
            est_loss = ((density - target).pow(2) if squared_estimation else (density - target).abs()).mean()        # :687-691
        else:
            raise ValueError(f"Unknown sdf_estimation_mode: {mode}")
    if with_surface:
        if squared_surface:
            surf_loss = (estimation / scale).pow(2)                                                                  # :697
        else:
            surf_loss = estimation.abs() / scale                                                                     # :699
        surf_loss = surf_loss.clamp(max=clamp_max).mean()                                                            # :700
    return est_loss, surf_loss


def density_regulariser_terms(sugar, visibility_filter, *, dtype=None, sdf_estimation_mode="density", use_sdf_estimation_loss=True,
                              enforce_samples_to_be_on_surface=False, squared_sdf_estimation_loss=False,
                              squared_samples_on_surface_loss=False, use_sdf_better_normal_loss=True,
                              sdf_better_normal_gradient_through_normal_only=True, density_factor=1.0, density_threshold=1.0,
                              n_samples_for_sdf_regularization=1_000_000, sdf_sampling_scale_factor=1.5,
                              sdf_sampling_proportional_to_volume=False, cameras_spatial_extent=None):
    """:574-730 for one camera.  The method calls go to `sugar` (in its own dtype); the inline statements run in `dtype` (None: the
    model's) on casts of what the methods returned, so that float64 measures the inline arithmetic alone."""
    cast = (lambda t: t) if dtype is None else (lambda t: t.to(dtype))
    plain = lambda t: t.as_subclass(torch.Tensor)
    samples, sample_idx = sugar.sample_points_in_gaussians(num_samples=n_samples_for_sdf_regularization,
                                                           sampling_scale_factor=sdf_sampling_scale_factor, mask=visibility_filter,
                                                           probabilities_proportional_to_volume=sdf_sampling_proportional_to_volume)   # :574, :634
    estimate = use_sdf_estimation_loss or enforce_samples_to_be_on_surface
    fields = sugar.get_field_values(samples, sample_idx, return_sdf=estimate and sdf_estimation_mode == "sdf",
                                    density_threshold=density_threshold, density_factor=density_factor, return_sdf_grad=False,
                                    sdf_grad_max_value=10., return_closest_gaussian_opacities=use_sdf_better_normal_loss,
                                    return_beta=estimate and sdf_estimation_mode == "density")                       # :642-649
    out = {"n_samples": samples.shape[0], "samples": samples, "sample_idx": sample_idx}
    opt = lambda k: cast(plain(fields[k])) if k in fields else None
    normals = cast(plain(sugar.get_normals(estimate_from_points=False)))
    points = cast(plain(sugar.points))
    if estimate:
        extent = float(sugar.get_cameras_spatial_extent() if cameras_spatial_extent is None else cameras_spatial_extent)
        est, surf = projection_estimation_losses(cast(plain(samples)), sample_idx, points, normals, mode=sdf_estimation_mode,
                                                 sdf=opt("sdf"), density=opt("density"), beta=opt("beta"), scale=extent / 10.,
                                                 clamp_max=10. * extent, with_estimation=use_sdf_estimation_loss,
                                                 with_surface=enforce_samples_to_be_on_surface,
                                                 squared_estimation=squared_sdf_estimation_loss,
                                                 squared_surface=squared_samples_on_surface_loss)
        if use_sdf_estimation_loss:
            out["sdf_estimation_loss"] = est
        if enforce_samples_to_be_on_surface:
            out["samples_on_surface_loss"] = surf
    if use_sdf_better_normal_loss:
        min_scaling = cast(plain(sugar.scaling)).min(dim=-1)[0]
        out["sdf_better_normal_loss"] = better_normal_loss(cast(plain(samples)), sample_idx, sugar.knn_idx, normals, points, min_scaling,
                                                           opt("closest_gaussian_opacities"),
                                                           sdf_better_normal_gradient_through_normal_only)
    return out
