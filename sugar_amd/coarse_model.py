"""The free Gaussians of SuGaR's coarse stage as a model of its own, for `sugar_amd.coarse_train`: the parameters under the
reference's names (sugar_scene/sugar_model.py) and the attributes and methods that `coarse_loss.regulariser_terms` asks of `sugar`,
each one the HIP kernel this package already has for it.  A model that is not bound to a mesh, `beta_mode='average'`, K = 16
neighbours; nothing else of the reference's class is restated here.

    parameters (raw)   _points [P,3]   _scales [P,3] (log)   _quaternions [P,4]   all_densities [P,1] (logit)
                       _sh_coordinates_dc [P,1,3]   _sh_coordinates_rest [P,M-1,3]
    properties         points   scaling   quaternions (normalised)   strengths   sh_coordinates   n_points            :384-479
    reset_neighbors    knn.knn_points(points, points), self included                                                      :1026-1030
    get_normals        sdf_regulariser.smallest_axis                                                                      :930-968
    get_field_values   sdf_regulariser.sdf_field (sdf or beta asked for) / field.density_field (neither)                  :1247-1316
    sample_points_in_gaussians   coarse_draw.draw_samples + sdf_regulariser.sample_transform; weighted draws go to the
                       torch statements of sugar_patch.sample_points_in_gaussians                                         :885-928
    render_image_gaussian_rasterizer   sugar_amd.diff_gaussian_rasterization with precomputed colours                     :2084-2294
    from_gaussian_ply / model_from / save_ply / state_dict / save_model / prune

The device-side draws keep a (seed, call) pair: every draw uses the current `call` and advances it, so a run is reproducible from its
seed and no draw repeats another.  `last_draw` holds what the latest draw returned (sample_idx, noise, n_masked -- all on the
device): the trainer reads n_masked from it, once per SDF iteration.

GPU tensors only for everything that computes; construction, `state_dict`, `save_model`, `model_from`, `save_ply` and `prune` work on CPU tensors."""
from __future__ import annotations

import collections
import functools

import torch

from . import sugar_patch

PARAMETER_NAMES = ("_points", "all_densities", "_scales", "_quaternions", "_sh_coordinates_dc", "_sh_coordinates_rest")   # registration order, :222-358


class CoarseModel:
    beta_mode = "average"
    binded_to_surface_mesh = False

    def __init__(self, points, scales, quaternions, densities, sh_dc, sh_rest, cameras=None, *, seed: int = 0, knn_to_track: int = 16):
        """raw parameter tensors (copied; on whatever device `points` is on) and the training cameras: a list of
        `sugar_amd.synthetic.Camera` (what `io.cameras_from_json` returns), or None for a model that only holds parameters"""
        dev = points.device
        P = points.shape[0]
        leaf = lambda t, shape: t.detach().to(dev, torch.float32).reshape(shape).clone().contiguous().requires_grad_(True)
        self._points = leaf(points, (P, 3))
        self._scales = leaf(scales, (P, 3))
        self._quaternions = leaf(quaternions, (P, 4))
        self.all_densities = leaf(densities, (P, 1))
        self._sh_coordinates_dc = leaf(sh_dc, (P, 1, 3))
        self._sh_coordinates_rest = leaf(sh_rest, (P, -1, 3))
        self.device = dev
        self.knn_to_track = int(knn_to_track)
        self.knn_idx = self.knn_dists = None
        self.seed, self.call = int(seed), 0
        self.last_draw = None
        self.cameras, self.p3d_cameras, self._extent = None, None, None
        if cameras is not None:
            self.set_cameras(cameras)

    # ---- cameras
    def set_cameras(self, cameras):
        from .mesh_render import p3d_camera_from_gs
        cameras = list(cameras)
        on_dev = lambda c: c._replace(viewmatrix=c.viewmatrix.to(self.device), projmatrix=c.projmatrix.to(self.device),
                                      campos=c.campos.to(self.device))
        self.cameras = [on_dev(c) for c in cameras]
        self.p3d_cameras = [p3d_camera_from_gs(c, self.device) for c in cameras]
        self.image_height, self.image_width = int(cameras[0].image_height), int(cameras[0].image_width)
        centers = torch.cat([c.get_camera_center().reshape(1, 3) for c in self.p3d_cameras], dim=0)
        self._extent = spatial_extent(centers)

    def get_cameras_spatial_extent(self):
        """1.1 x the largest distance of a camera centre from their mean (:825-837), formed once when the cameras were set"""
        if self._extent is None:
            raise RuntimeError("CoarseModel: no cameras were given")
        return self._extent

    # ---- sugar_model.py:384-479 for a model that is not bound to a mesh
    points = property(lambda self: self._points)
    scaling = property(lambda self: torch.exp(self._scales))
    quaternions = property(lambda self: torch.nn.functional.normalize(self._quaternions, dim=-1))
    strengths = property(lambda self: torch.sigmoid(self.all_densities.view(-1, 1)))
    sh_coordinates = property(lambda self: torch.cat([self._sh_coordinates_dc, self._sh_coordinates_rest], dim=1))
    n_points = property(lambda self: len(self._points))

    def parameters(self):
        return [getattr(self, n) for n in PARAMETER_NAMES]

    def zero_grad(self):
        for p in self.parameters():
            p.grad = None

    def reset_neighbors(self, knn_to_track: int = None):
        """:1026-1030: the K nearest Gaussians of every Gaussian, itself included"""
        from .knn import knn_points
        if knn_to_track is not None:
            self.knn_to_track = int(knn_to_track)
        with torch.no_grad():
            knns = knn_points(self.points[None], self.points[None], K=self.knn_to_track)
            self.knn_dists, self.knn_idx = knns.dists[0], knns.idx[0]

    # ---- the methods `regulariser_terms` calls
    def get_covariance(self, return_full_matrix=False, return_sqrt=False, inverse_scales=False):
        """:729-736 for the one call the field makes: the scaled rotation (`return_sqrt=True`) of a model on the device"""
        if not (return_sqrt and self._quaternions.is_cuda):
            raise NotImplementedError("CoarseModel.get_covariance: only return_sqrt=True on a ROCm device is implemented")
        return sugar_patch.get_covariance(self, return_full_matrix=return_full_matrix, return_sqrt=True, inverse_scales=inverse_scales)

    get_smallest_axis = functools.partialmethod(sugar_patch.get_smallest_axis, _prev=None)

    def get_normals(self, estimate_from_points=False, neighborhood_size: int = 32):
        if estimate_from_points:
            raise NotImplementedError("CoarseModel.get_normals: estimate_from_points=True is not implemented")
        return self.get_smallest_axis()                                         # :967

    def get_field_values(self, x, gaussian_idx=None, closest_gaussians_idx=None, gaussian_strengths=None, gaussian_centers=None,
                         gaussian_inv_scaled_rotation=None, return_sdf=True, density_threshold=1., density_factor=1.,
                         return_sdf_grad=False, sdf_grad_max_value=10., opacity_min_clamp=1e-16,
                         return_closest_gaussian_opacities=False, return_beta=False):
        """:1247-1316 for the calls `coarse_loss.regulariser_terms` makes: the model's own Gaussians, the samples' Gaussians in
        `gaussian_idx`, no sdf gradient.  With the sdf or beta asked for it is `sdf_regulariser.sdf_field`, with neither
        `field.density_field`."""
        if return_sdf_grad:
            raise NotImplementedError("CoarseModel.get_field_values: return_sdf_grad=True is not implemented")
        if any(a is not None for a in (closest_gaussians_idx, gaussian_strengths, gaussian_centers, gaussian_inv_scaled_rotation)):
            raise NotImplementedError("CoarseModel.get_field_values: other Gaussians than the model's own are not implemented")
        if gaussian_idx is None:
            raise NotImplementedError("CoarseModel.get_field_values: gaussian_idx=None (a neighbour search per call) is not implemented")
        if not (sugar_patch._number(density_threshold) and density_threshold > 0 and sugar_patch._number(opacity_min_clamp)):
            raise NotImplementedError("CoarseModel.get_field_values: density_threshold must be a positive number")
        kw = dict(return_sdf=return_sdf, density_threshold=density_threshold, density_factor=density_factor, return_sdf_grad=False,
                  sdf_grad_max_value=sdf_grad_max_value, opacity_min_clamp=opacity_min_clamp,
                  return_closest_gaussian_opacities=return_closest_gaussian_opacities, return_beta=return_beta)
        if return_sdf or return_beta:
            return sugar_patch.get_field_values_with_sdf_tail(self, x, gaussian_idx, _prev=None, **kw)
        return sugar_patch.get_field_values(self, x, gaussian_idx, _orig=None, **kw)

    def sample_points_in_gaussians(self, num_samples, sampling_scale_factor=1., mask=None, probabilities_proportional_to_opacity=False,
                                   probabilities_proportional_to_volume=True):
        """:885-928.  The coarse stage's default call -- a mask, uniform over the masked Gaussians -- draws on the device
        (`coarse_draw.draw_samples`, no host wait); weighted draws and a call without a mask go to the torch statements."""
        from .sdf_regulariser import sample_transform
        weighted = probabilities_proportional_to_opacity or probabilities_proportional_to_volume
        if weighted or mask is None:
            n_masked = None if mask is None else mask.sum()
            if n_masked is None or int(n_masked) > 0:          # (the host read the reference makes before it samples, coarse_sdf.py:625-626)
                samples, sample_idx = sugar_patch.sample_points_in_gaussians(
                    self, num_samples, sampling_scale_factor=sampling_scale_factor, mask=mask,
                    probabilities_proportional_to_opacity=probabilities_proportional_to_opacity,
                    probabilities_proportional_to_volume=probabilities_proportional_to_volume)
                self.last_draw = None if n_masked is None else (sample_idx, None, n_masked)
                return samples, sample_idx
            sample_idx = torch.zeros(num_samples, dtype=torch.int64, device=self.device)      # nothing to choose from: as the device draw
            noise = torch.zeros(num_samples, 3, device=self.device)
        else:
            from .coarse_draw import draw_samples
            sample_idx, noise, n_masked = draw_samples(mask.reshape(-1), num_samples, self.seed, self.call)
            self.call += 1
        self.last_draw = (sample_idx, noise, n_masked)
        return sample_transform(self.points, self.quaternions, self.scaling, sample_idx, noise, float(sampling_scale_factor)), sample_idx

    # ---- rendering, :2084-2294 for precomputed colours and the covariance formed in the rasterizer
    def render_image_gaussian_rasterizer(self, camera_indices=0, bg_color=None, sh_deg=0, compute_color_in_rasterizer=False,
                                         compute_covariance_in_rasterizer=True, return_2d_radii=False, return_opacities=False,
                                         point_colors=None, **unused):
        from .diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
        from .shcolor import sh_to_rgb
        if compute_color_in_rasterizer or not compute_covariance_in_rasterizer:
            raise NotImplementedError("CoarseModel renders precomputed colours with the covariance formed in the rasterizer")
        cam, dev = self.cameras[camera_indices], self.device
        if bg_color is None:
            bg_color = torch.zeros(3, device=dev)
        st = GaussianRasterizationSettings(image_height=self.image_height, image_width=self.image_width, tanfovx=cam.tanfovx,
                                           tanfovy=cam.tanfovy, bg=bg_color, scale_modifier=1., viewmatrix=cam.viewmatrix,
                                           projmatrix=cam.projmatrix, sh_degree=sh_deg, campos=cam.campos, prefiltered=False, debug=False)
        if point_colors is None:
            point_colors = sh_to_rgb(self.sh_coordinates, sh_deg + 1, positions=self.points,
                                     camera_centers=self.p3d_cameras[camera_indices].get_camera_center())      # :2190-2193
        opacities = self.strengths.view(-1, 1)
        means2D = torch.zeros(self.n_points, 3, device=dev, requires_grad=True)
        image, radii = GaussianRasterizer(st)(means3D=self.points, means2D=means2D, shs=None, colors_precomp=point_colors,
                                              opacities=opacities, scales=self.scaling, rotations=self.quaternions, cov3D_precomp=None)
        image = image.transpose(0, 1).transpose(1, 2)
        if not (return_2d_radii or return_opacities):
            return image
        out = {"image": image, "radii": radii, "viewspace_points": means2D}
        if return_opacities:
            out["opacities"] = opacities
        return out

    # ---- I/O
    @classmethod
    def from_gaussian_ply(cls, path, cameras=None, device="cuda", **kwargs):
        """a 3DGS point cloud (`io.load_gaussian_ply`): the raw values go over as they are, as coarse_sdf.py:390-394 copies them"""
        from . import io
        g = io.load_gaussian_ply(path, device=device)
        return cls(g["xyz"], g["scaling"], g["rotation"], g["opacity"], g["features"][:, :1], g["features"][:, 1:], cameras, **kwargs)

    def state_dict(self):
        return collections.OrderedDict((n, getattr(self, n).detach()) for n in PARAMETER_NAMES)

    def save_model(self, path, **extras):
        """the reference's checkpoint shape, :2296-2301: {'state_dict': ..., **extras}"""
        checkpoint = {"state_dict": self.state_dict()}
        checkpoint.update(extras)
        torch.save(checkpoint, path)

    @classmethod
    def model_from(cls, checkpoint, cameras=None, device="cpu", **kwargs):
        """the model of a checkpoint `save_model` wrote (a path or the loaded dict)"""
        if not isinstance(checkpoint, dict):
            checkpoint = torch.load(checkpoint, map_location=device)
        s = checkpoint["state_dict"]
        to = lambda t: t.to(device)
        return cls(to(s["_points"]), to(s["_scales"]), to(s["_quaternions"]), to(s["all_densities"]), to(s["_sh_coordinates_dc"]),
                   to(s["_sh_coordinates_rest"]), cameras, **kwargs)

    def save_ply(self, path):
        """the 3DGS point cloud `sugar_amd.extract` reads"""
        from . import io
        io.save_gaussian_ply(path, self._points, self.sh_coordinates, self.all_densities, self._scales, self._quaternions)

    # ---- pruning
    @torch.no_grad()
    def prune(self, keep_mask, optimizer=None):
        """keeps the rows where `keep_mask` is set: the six parameters become new leaves and, with an optimiser, its groups point at
        them with the kept rows of both Adam moments and the step count (sugar_densifier.py's `_prune_optimizer`, which is
        gaussian_model.py:272-288).  `densify.py`'s prune path works on its own five names and a joint feature tensor, so it does not
        fit the six groups here.  The neighbours are stale afterwards: call `reset_neighbors`."""
        keep = keep_mask.reshape(-1).to(self.device, torch.bool)
        if keep.shape[0] != self.n_points:
            raise ValueError("CoarseModel.prune: the mask must have one entry per Gaussian")
        for n in PARAMETER_NAMES:
            old = getattr(self, n)
            new = old.detach()[keep].clone().contiguous().requires_grad_(True)
            setattr(self, n, new)
            if optimizer is None:
                continue
            for group in optimizer.param_groups:
                if len(group["params"]) == 1 and group["params"][0] is old:
                    state = optimizer.state.pop(old, None)
                    if state:
                        state["exp_avg"] = state["exp_avg"][keep].clone().contiguous()
                        state["exp_avg_sq"] = state["exp_avg_sq"][keep].clone().contiguous()
                        optimizer.state[new] = state
                    group["params"][0] = new
        self.knn_idx = self.knn_dists = None
        self.last_draw = None


def spatial_extent(camera_centers) -> float:
    """:829-833: 1.1 x the largest distance of a camera centre [n,3] from the mean centre"""
    c = camera_centers.detach().reshape(-1, 3).float()
    return 1.1 * torch.norm(c - c.mean(dim=0, keepdim=True), dim=-1).max().item()
