"""SuGaR's coarse stage as a loop of this package's own: the default schedule of sugar_trainers/coarse_sdf.py ("sdf") or of
sugar_trainers/coarse_density.py ("density") from a 7 000-iteration 3DGS checkpoint, over `coarse_model.CoarseModel` and the HIP
kernels --

    RGB pass      shcolor.sh_to_rgb -> colours, sugar_amd.diff_gaussian_rasterization, fused_loss.l1_ssim_loss        coarse_sdf.py:504-536
    entropy       coarse_loss.opacity_entropy over radii > 0, for 7000 < it < 9000                                    :538-551
    neighbours    knn.knn_points at 7001 and at every it % 500 == 0 from then on                                      :559-561
    prune         strengths < 0.5 at the start of 9001, the Adam moments of the kept rows carried, neighbours reset   :486-497
    SDF pass      for it > 9000: depth rendered as colour (bg = the largest depth, gradient flowing),
                  coarse_loss.regulariser_terms with the draws of coarse_draw, factors 0.2 / 0.2                      :566-716
    density pass  with regulariser='density' instead of the SDF pass: NO depth render and no band -- the draw over
                  radii > 0, coarse_loss.density_regulariser_terms (the estimate is the sample's offset along its
                  own Gaussian's normal, the target exp(-est^2 / 2 beta^2)), factors 0.2 / 0.2            coarse_density.py:570-730
    optimiser     fused_adam.FusedAdam over the reference's six groups and rates, the positions' rate on its schedule sugar_optimizer.py

as a class (`CoarseTrainer.step`) and a command:

    python -m sugar_amd.coarse_train POINT_CLOUD.ply --cameras cameras.json --images DIR --out DIR
        [--regulariser {sdf,density} --iterations 15000 --start-iteration 7000 --estimation-factor 0.2 --normal-factor 0.2 --seed 0]

which writes DIR/<iterations>.pt (the reference's checkpoint shape) and DIR/point_cloud.ply (what `sugar_amd.extract` reads) and
prints the reference's loss line every 50 iterations.  The schedule is the pure function `phase`: the two trainers share it.
`regulariser='density'` applies DENSITY_OVERRIDES, the four defaults in which coarse_density.py differs; options given by the caller
win.  Not here: densification inside this loop (the reference's defaults disable it from a trained 3DGS), mesh-bound models, beta
modes other than 'average', coarse_density.py's depth-map estimate (`use_projection_as_estimation=False` there), the projection
estimate under the "sdf" regulariser, multi-GPU.

A step reads the device once on top of what the rasterizer's plain API does: the number of Gaussians the draw could choose from,
once per SDF iteration -- with none, the regulariser is left out of that step, as the reference does (:626, :717-718)."""
from __future__ import annotations

import argparse
import math
import os
import sys
import time
from typing import NamedTuple

import torch

# the trainer's names and defaults, coarse_sdf.py:56-224 (initialize_from_trained_3dgs=True)
DEFAULTS = dict(
    num_iterations=15_000, spatial_lr_scale=None, position_lr_init=0.00016, position_lr_final=0.0000016, position_lr_delay_mult=0.01,
    position_lr_max_steps=30_000, feature_lr=0.0025, opacity_lr=0.05, scaling_lr=0.005, rotation_lr=0.001,
    dssim_factor=0.2, sh_levels=4, use_white_background=False,
    enforce_entropy_regularization=True, start_entropy_regularization_from=7000, end_entropy_regularization_at=9000,
    entropy_regularization_factor=0.1,
    regularize_sdf=True, start_sdf_regularization_from=9000, use_sdf_estimation_loss=True, enforce_samples_to_be_on_surface=False,
    sdf_estimation_mode="sdf", samples_on_surface_factor=0.2, squared_sdf_estimation_loss=False, squared_samples_on_surface_loss=False,
    normalize_by_sdf_std=False, start_sdf_estimation_from=9000, sample_only_in_gaussians_close_to_surface=True,
    close_gaussian_threshold=2., backpropagate_gradients_through_depth=True, use_sdf_better_normal_loss=True,
    start_sdf_better_normal_from=9000, sdf_better_normal_gradient_through_normal_only=True, density_factor=1. / 16.,
    density_threshold=1., n_samples_for_sdf_regularization=1_000_000, sdf_sampling_scale_factor=1.5,
    sdf_sampling_proportional_to_volume=False,
    regularity_knn=16, reset_neighbors_every=500, regularize_from=7000, start_reset_neighbors_from=7001,
    prune_when_starting_regularization=False, prune_low_opacity_gaussians_at=(9000,), prune_hard_opacity_threshold=0.5,
    estimation_factor=0.2, normal_factor=0.2, print_loss_every_n_iterations=50,
    regulariser="sdf", use_projection_as_estimation=False,
)
# what coarse_density.py:112-156 sets differently from coarse_sdf.py (`use_projection_as_estimation` turns the band off, :127-128)
DENSITY_OVERRIDES = dict(sdf_estimation_mode="density", use_projection_as_estimation=True,
                         sample_only_in_gaussians_close_to_surface=False, density_factor=1.0)
REGULARISERS = ("sdf", "density")
GROUPS = (("points", "_points"), ("sh_coordinates_dc", "_sh_coordinates_dc"), ("sh_coordinates_rest", "_sh_coordinates_rest"),
          ("all_densities", "all_densities"), ("scales", "_scales"), ("quaternions", "_quaternions"))      # sugar_optimizer.py:67-83


class Phase(NamedTuple):
    """what iteration `it` does, in the order the loop does it"""
    prune: bool               # at the start: remove the Gaussians below the hard opacity threshold ...
    reset_after_prune: bool   # ... and, when the prune happens, reset the neighbours
    entropy: bool             # add the entropy term
    reset_neighbors: bool     # reset the neighbours before the regulariser
    sdf: bool                 # draw samples and add the regulariser's terms
    sdf_estimation: bool
    sdf_better_normal: bool


def phase(iteration: int, **options) -> Phase:
    """the schedule of coarse_sdf.py:486-497, :538, :553-572, :688 as flags; `options` override DEFAULTS"""
    o = dict(DEFAULTS, **options)
    it = int(iteration)
    regularize = bool(o["regularize_sdf"])                                                                      # :178-189
    prune = (regularize and o["prune_when_starting_regularization"] and it == o["regularize_from"] + 1) or (
        (it - 1) in tuple(o["prune_low_opacity_gaussians_at"]))                                                 # :487-491
    entropy = bool(o["enforce_entropy_regularization"]) and o["start_entropy_regularization_from"] < it < o["end_entropy_regularization_at"]
    in_reg = regularize and it > o["regularize_from"]                                                           # :553-557
    reset = in_reg and it >= o["start_reset_neighbors_from"] and (it == o["regularize_from"] + 1
                                                                  or it % o["reset_neighbors_every"] == 0)      # :559
    sdf = in_reg and it > o["start_sdf_regularization_from"]                                                    # :566
    est = sdf and bool(o["use_sdf_estimation_loss"] or o["enforce_samples_to_be_on_surface"]) and it > o["start_sdf_estimation_from"]
    nrm = sdf and bool(o["use_sdf_better_normal_loss"]) and it > o["start_sdf_better_normal_from"]
    return Phase(prune=bool(prune), reset_after_prune=bool(prune and regularize and it >= o["start_reset_neighbors_from"]),
                 entropy=bool(entropy), reset_neighbors=bool(reset), sdf=bool(sdf and (est or nrm)), sdf_estimation=bool(est),
                 sdf_better_normal=bool(nrm))


def expon_lr(step, lr_init, lr_final, lr_delay_steps=0, lr_delay_mult=1.0, max_steps=1_000_000) -> float:
    """get_expon_lr_func, sugar_utils/general_utils.py:23-56: log-linear from lr_init at step 0 to lr_final at max_steps, times the
    delay factor when lr_delay_steps > 0"""
    if step < 0 or (lr_init == 0.0 and lr_final == 0.0):
        return 0.0
    if lr_delay_steps > 0:
        delay_rate = lr_delay_mult + (1 - lr_delay_mult) * math.sin(0.5 * math.pi * min(max(step / lr_delay_steps, 0.0), 1.0))
    else:
        delay_rate = 1.0
    t = min(max(step / max_steps, 0.0), 1.0)
    return delay_rate * math.exp(math.log(lr_init) * (1 - t) + math.log(lr_final) * t)


def position_lr(iteration, lr_scale, **options) -> float:
    """SuGaROptimizer.update_learning_rate (sugar_optimizer.py:87-109): the `points` group's rate at `iteration` for the spatial scale
    `lr_scale` (the cameras' extent unless the option `spatial_lr_scale` says otherwise: the caller resolves that).  The optimiser
    hands `lr_delay_mult` but no `lr_delay_steps`, so the delay factor is 1."""
    o = dict(DEFAULTS, **options)
    return expon_lr(iteration, o["position_lr_init"] * lr_scale, o["position_lr_final"] * lr_scale,
                    lr_delay_mult=o["position_lr_delay_mult"], max_steps=o["position_lr_max_steps"])


class CoarseTrainer:
    def __init__(self, model, cameras, images, **options):
        """`model`: a `CoarseModel` on a ROCm device; `cameras`: the list of `synthetic.Camera` it renders (handed to the model when
        it has none yet); `images`: one [H,W,3] or [3,H,W] float32 ground-truth image per camera; `options`: any key of DEFAULTS"""
        unknown = sorted(set(options) - set(DEFAULTS))
        if unknown:
            raise TypeError(f"CoarseTrainer: unknown options {unknown}")
        regulariser = options.get("regulariser", DEFAULTS["regulariser"])
        if regulariser not in REGULARISERS:
            raise ValueError(f"CoarseTrainer: regulariser must be one of {REGULARISERS}, got {regulariser!r}")
        self.options = o = dict(DEFAULTS, **(DENSITY_OVERRIDES if regulariser == "density" else {}))
        o.update(options)                                                        # the caller's explicit options win
        if not model._points.is_cuda:
            raise RuntimeError("CoarseTrainer: the model must be on a ROCm device; there is no CPU fallback")
        if len({o["start_sdf_regularization_from"], o["start_sdf_estimation_from"], o["start_sdf_better_normal_from"]}) != 1:
            raise NotImplementedError("CoarseTrainer: the regulariser's terms must start together (the reference's default)")
        if not o["backpropagate_gradients_through_depth"]:
            raise NotImplementedError("CoarseTrainer: backpropagate_gradients_through_depth=False is not implemented")
        if regulariser == "density":
            if not o["use_projection_as_estimation"]:
                raise NotImplementedError("CoarseTrainer: regulariser='density' with use_projection_as_estimation=False (the depth-map "
                                          "estimate of coarse_density.py) is not implemented")
            if o["sample_only_in_gaussians_close_to_surface"]:
                raise NotImplementedError("CoarseTrainer: sample_only_in_gaussians_close_to_surface=True with "
                                          "use_projection_as_estimation=True is not implemented (the reference turns the band off, "
                                          "coarse_density.py:127-128)")
            if o["normalize_by_sdf_std"]:
                raise NotImplementedError("CoarseTrainer: normalize_by_sdf_std=True with use_projection_as_estimation=True is not "
                                          "implemented (the reference forces it off, coarse_density.py:664-667)")
        elif o["use_projection_as_estimation"]:
            raise NotImplementedError("CoarseTrainer: use_projection_as_estimation=True needs regulariser='density'")
        from .fused_adam import FusedAdam
        self.model = model
        if model.cameras is None:
            model.set_cameras(cameras)
        if len(images) != len(model.cameras):
            raise ValueError("CoarseTrainer: one image per camera")
        dev = model.device
        H, W = model.image_height, model.image_width
        self.images = []
        for im in images:
            im = torch.as_tensor(im, dtype=torch.float32)
            if im.shape == (H, W, 3):
                im = im.permute(2, 0, 1)
            if im.shape != (3, H, W):
                raise ValueError(f"CoarseTrainer: an image is {tuple(im.shape)}, the cameras render {W} x {H}")
            self.images.append(im.contiguous().to(dev))
        model.knn_to_track = int(o["regularity_knn"])
        self.extent = model.get_cameras_spatial_extent()
        self.spatial_lr_scale = self.extent if o["spatial_lr_scale"] is None else float(o["spatial_lr_scale"])          # :412-414
        rates = dict(points=o["position_lr_init"] * self.spatial_lr_scale, sh_coordinates_dc=o["feature_lr"],
                     sh_coordinates_rest=o["feature_lr"] / 20.0, all_densities=o["opacity_lr"], scales=o["scaling_lr"],
                     quaternions=o["rotation_lr"])
        self.optimizer = FusedAdam([{"params": [getattr(model, attr)], "lr": rates[name], "name": name} for name, attr in GROUPS],
                                   lr=0.0, eps=1e-15)
        self.bg = torch.ones(3, device=dev) if o["use_white_background"] else None
        self.train_losses = []
        self.n_masked = None          # of the latest SDF iteration, as a Python int

    def update_learning_rate(self, iteration):
        lr = position_lr(iteration, self.spatial_lr_scale, **self.options)
        for group in self.optimizer.param_groups:
            if group["name"] == "points":
                group["lr"] = lr
        return lr

    def _density_regulariser(self, ph, visible):
        """(weighted sum or None, terms) of coarse_density.py:570-730 for one camera: no depth render, the draw over `visible`"""
        from .coarse_loss import density_regulariser_terms
        o, model = self.options, self.model
        terms = density_regulariser_terms(
            model, visible, sdf_estimation_mode=o["sdf_estimation_mode"],
            use_sdf_estimation_loss=bool(o["use_sdf_estimation_loss"]) and ph.sdf_estimation,
            enforce_samples_to_be_on_surface=bool(o["enforce_samples_to_be_on_surface"]) and ph.sdf_estimation,
            squared_sdf_estimation_loss=o["squared_sdf_estimation_loss"],
            squared_samples_on_surface_loss=o["squared_samples_on_surface_loss"], use_sdf_better_normal_loss=ph.sdf_better_normal,
            sdf_better_normal_gradient_through_normal_only=o["sdf_better_normal_gradient_through_normal_only"],
            density_factor=o["density_factor"], density_threshold=o["density_threshold"],
            n_samples_for_sdf_regularization=o["n_samples_for_sdf_regularization"],
            sdf_sampling_scale_factor=o["sdf_sampling_scale_factor"],
            sdf_sampling_proportional_to_volume=o["sdf_sampling_proportional_to_volume"], cameras_spatial_extent=self.extent)
        self.n_masked = int(model.last_draw[2])          # the step's one host read, after the terms, as in `_regulariser`
        if self.n_masked == 0:
            return None, {}                                                                                              # :632-633, :731-732
        weights = dict(sdf_estimation_loss=o["estimation_factor"], samples_on_surface_loss=o["samples_on_surface_factor"],
                       sdf_better_normal_loss=o["normal_factor"])
        return sum(weights[k] * terms[k] for k in weights if k in terms), terms

    def _regulariser(self, ph, camera_index, visible):
        """(weighted sum or None, terms) of :566-716 for one camera"""
        if self.options["regulariser"] == "density":
            return self._density_regulariser(ph, visible)
        from .coarse_loss import regulariser_terms
        o, model = self.options, self.model
        fov_camera = model.p3d_cameras[camera_index]
        point_depth = fov_camera.get_world_to_view_transform().transform_points(model.points)[..., 2:].expand(-1, 3)      # :579
        max_depth = point_depth.max()
        depth = model.render_image_gaussian_rasterizer(camera_indices=camera_index,
                                                       bg_color=max_depth + torch.zeros(3, dtype=torch.float, device=model.device),
                                                       sh_deg=0, point_colors=point_depth)[..., 0]                       # :581-590
        terms = regulariser_terms(
            model, fov_camera, depth, visible, sdf_estimation_mode=o["sdf_estimation_mode"],
            use_sdf_estimation_loss=bool(o["use_sdf_estimation_loss"]) and ph.sdf_estimation,
            enforce_samples_to_be_on_surface=bool(o["enforce_samples_to_be_on_surface"]) and ph.sdf_estimation,
            squared_sdf_estimation_loss=o["squared_sdf_estimation_loss"],
            squared_samples_on_surface_loss=o["squared_samples_on_surface_loss"], normalize_by_sdf_std=o["normalize_by_sdf_std"],
            sample_only_in_gaussians_close_to_surface=o["sample_only_in_gaussians_close_to_surface"],
            close_gaussian_threshold=o["close_gaussian_threshold"], use_sdf_better_normal_loss=ph.sdf_better_normal,
            sdf_better_normal_gradient_through_normal_only=o["sdf_better_normal_gradient_through_normal_only"],
            density_factor=o["density_factor"], density_threshold=o["density_threshold"],
            n_samples_for_sdf_regularization=o["n_samples_for_sdf_regularization"],
            sdf_sampling_scale_factor=o["sdf_sampling_scale_factor"],
            sdf_sampling_proportional_to_volume=o["sdf_sampling_proportional_to_volume"], cameras_spatial_extent=self.extent)
        # the step's one host read: how many Gaussians the draw could choose from.  It comes after the whole of `regulariser_terms`: with
        # an empty band the field, the normals and both loss forwards have run on all-zero draws (samples at Gaussian 0's centre) and are
        # thrown away here.  That is rare (no visible Gaussian within the band of the depth map) and harmless, and it keeps the common
        # iteration free of a host wait between the draw and the field kernels.
        self.n_masked = int(model.last_draw[2])
        if self.n_masked == 0:
            return None, {}                                                                                              # :626, :717-718
        weights = dict(sdf_estimation_loss=o["estimation_factor"], samples_on_surface_loss=o["samples_on_surface_factor"],
                       sdf_better_normal_loss=o["normal_factor"])
        return sum(weights[k] * terms[k] for k in weights if k in terms), terms

    def step(self, iteration, camera_index, return_grads: bool = False):
        """one iteration of the loop (coarse_sdf.py:481-758) on camera `camera_index`; returns the loss and its unweighted terms as
        0-dim device tensors (nothing is read back here), and with `return_grads` a copy of every parameter's gradient by group"""
        from .coarse_loss import opacity_entropy
        from .fused_loss import l1_ssim_loss
        o, model = self.options, self.model
        ph = phase(iteration, **o)
        self.update_learning_rate(iteration)                                                                             # :484
        if ph.prune:                                                                                                     # :486-497
            with torch.no_grad():
                prune_mask = (model.strengths < o["prune_hard_opacity_threshold"]).squeeze()
            model.prune(~prune_mask, self.optimizer)
            if ph.reset_after_prune:
                model.reset_neighbors()
        outputs = model.render_image_gaussian_rasterizer(camera_indices=camera_index, bg_color=self.bg, sh_deg=o["sh_levels"] - 1,
                                                         return_2d_radii=True, return_opacities=True)                    # :506-518
        pred_rgb = outputs["image"].transpose(-1, -2).transpose(-2, -3)                                                  # :528
        result = {"rgb_loss": l1_ssim_loss(pred_rgb, self.images[camera_index], o["dssim_factor"])}                      # :457, :536
        loss = result["rgb_loss"]
        visible = outputs["radii"] > 0                                                                                   # :543, :558
        if ph.entropy:
            result["entropy"] = opacity_entropy(outputs["opacities"], visible)
            loss = loss + o["entropy_regularization_factor"] * result["entropy"]                                         # :548-551
        if ph.reset_neighbors or (ph.sdf and model.knn_idx is None):
            model.reset_neighbors()                                                                                      # :559-561
        if ph.sdf:
            weighted, terms = self._regulariser(ph, camera_index, visible)
            result["n_masked"] = self.n_masked
            if weighted is not None:
                loss = loss + weighted
                result.update(terms)
        result["loss"] = loss
        loss.backward()                                                                                                  # :735
        if return_grads:
            result["grads"] = {name: getattr(model, attr).grad.detach().clone() for name, attr in GROUPS}
        self.optimizer.step()                                                                                            # :757-758
        self.optimizer.zero_grad(set_to_none=True)
        return result

    def save(self, path, iteration, epoch=0):
        """the reference's checkpoint, :785-790"""
        self.model.save_model(path, train_losses=self.train_losses, epoch=epoch, iteration=iteration,
                              optimizer_state_dict=self.optimizer.state_dict())

    def run(self, start_iteration, num_iterations=None, seed: int = 0, log=print):
        """the loop of :471-812 from `start_iteration` (exclusive) to `num_iterations` (inclusive): a fresh shuffle of the cameras per
        epoch, the loss line every `print_loss_every_n_iterations`; returns (iteration, epoch)"""
        o = self.options
        num_iterations = o["num_iterations"] if num_iterations is None else int(num_iterations)
        generator = torch.Generator().manual_seed(int(seed))
        iteration, epoch, t0 = int(start_iteration), 0, time.time()
        while iteration < num_iterations:
            for camera_index in torch.randperm(len(self.model.cameras), generator=generator).tolist():                   # :476
                iteration += 1
                result = self.step(iteration, camera_index)
                if iteration == 1 or iteration % o["print_loss_every_n_iterations"] == 0:                                # :761-765
                    loss = result["loss"].detach().item()
                    self.train_losses.append(loss)
                    log(f"loss: {loss:>7f}  [{iteration:>5d}/{num_iterations:>5d}]", "computed in", (time.time() - t0) / 60., "minutes.")
                    t0 = time.time()
                if iteration >= num_iterations:
                    break
            epoch += 1
        return iteration, epoch


def _find_image(directory, name):
    for suffix in ("", ".png", ".jpg", ".jpeg", ".JPG", ".PNG"):
        p = os.path.join(directory, name + suffix)
        if os.path.isfile(p):
            return p
    raise FileNotFoundError(f"no image named {name!r} (.png / .jpg / .jpeg) in {directory}")


def _parser():
    ap = argparse.ArgumentParser(prog="python -m sugar_amd.coarse_train", description="SuGaR's coarse stage with the SDF regulariser "
                                 "(coarse_sdf.py's default schedule) or the density regulariser (coarse_density.py's) from a trained "
                                 "3DGS point cloud, on the HIP kernels")
    ap.add_argument("point_cloud", help="the 3DGS checkpoint's point_cloud.ply")
    ap.add_argument("--cameras", required=True, help="cameras.json (the 3DGS format)")
    ap.add_argument("--images", required=True, help="directory of the training images, named like the cameras")
    ap.add_argument("--out", required=True, help="directory for <iterations>.pt and point_cloud.ply")
    ap.add_argument("--iterations", type=int, default=DEFAULTS["num_iterations"])
    ap.add_argument("--start-iteration", type=int, default=7000, help="the iteration the 3DGS checkpoint was written at")
    ap.add_argument("--estimation-factor", type=float, default=DEFAULTS["estimation_factor"])
    ap.add_argument("--normal-factor", type=float, default=DEFAULTS["normal_factor"])
    ap.add_argument("--samples", type=int, default=DEFAULTS["n_samples_for_sdf_regularization"], help="samples of the regulariser per iteration")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--regulariser", choices=REGULARISERS, default=DEFAULTS["regulariser"],
                    help="sdf: coarse_sdf.py's loop; density: coarse_density.py's (recommended for object-centric scenes)")
    return ap


def main(argv=None) -> int:
    a = _parser().parse_args(argv)
    import numpy as np
    from PIL import Image
    from . import io as sio
    from .coarse_model import CoarseModel
    if not torch.cuda.is_available():
        raise RuntimeError("coarse_train needs a ROCm device; there is no CPU fallback")
    dev = torch.device(a.device)
    cams, names = sio.cameras_from_json(a.cameras)
    images = []
    for cam, name in zip(cams, names):
        p = _find_image(a.images, name)
        with Image.open(p) as im:
            rgb = torch.from_numpy(np.asarray(im.convert("RGB"), dtype=np.uint8).astype(np.float32) / np.float32(255.0))
        if tuple(rgb.shape[:2]) != (int(cam.image_height), int(cam.image_width)):
            raise ValueError(f"{p}: {rgb.shape[1]}x{rgb.shape[0]}, the camera renders {cam.image_width}x{cam.image_height}")
        images.append(rgb)
    model = CoarseModel.from_gaussian_ply(a.point_cloud, cams, device=dev, seed=a.seed)
    trainer = CoarseTrainer(model, cams, images, num_iterations=a.iterations, estimation_factor=a.estimation_factor,
                            normal_factor=a.normal_factor, n_samples_for_sdf_regularization=a.samples, regulariser=a.regulariser)
    print(f"{model.n_points} Gaussians, {len(cams)} cameras, spatial extent {trainer.extent:.4g}; "
          f"iterations {a.start_iteration + 1} .. {a.iterations}")
    iteration, epoch = trainer.run(a.start_iteration, a.iterations, seed=a.seed)
    os.makedirs(a.out, exist_ok=True)
    trainer.save(os.path.join(a.out, f"{iteration}.pt"), iteration, epoch)
    model.save_ply(os.path.join(a.out, "point_cloud.ply"))
    print(f"{model.n_points} Gaussians written to {a.out} ({iteration}.pt, point_cloud.ply)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
