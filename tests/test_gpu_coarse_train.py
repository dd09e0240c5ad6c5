"""GPU tests of the native coarse-SDF trainer (sugar_amd.coarse_model / sugar_amd.coarse_train) on the model of
tests/golden/sugar_field.npz (P = 2 500, 120 x 88, `orbit_cameras`), with tests/sugar_regulariser_standin.make_module() -- the
stand-in SuGaR class under the package's bindings -- as the independent side.

  * the model against the stand-in: properties, neighbours, normals, the two `get_field_values` call shapes, the device draw, the
    weighted draw's torch path, the calls it refuses;
  * one entropy-phase step (it = 8000) and one SDF-phase step (it = 9500, the fixture's camera 3 and band threshold 8.0) against a
    composition written out here: the stand-in's `render_image_gaussian_rasterizer`, `train_step.train_loss(fused=False)`, the entropy
    statement (coarse_sdf.py:543-551) and tests/coarse_loss_restatement.regulariser_terms with the trainer's recorded
    (sample_idx, noise) injected into the stand-in's sampler.  The method calls are the same kernels on both sides, so the float64
    run of the inline statements measures them alone and their float32 run gives the yards: every scalar within
    max(4 x yard, 2 float32 ulp), every gradient norm-wise within max(4 x yard, 1e-7) (the bars of tests/test_gpu_coarse_loss.py);
  * after each of the two steps the parameters and both moments against `torch.optim.Adam`'s update of the same gradients in float64,
    held to the bars of tests/test_gpu_optim_elements.py (tests/optim_cases.bar_from: 4 x the worse yardstick's worst element, 2 x
    its median, floored at one rounding);
  * an empty band: nothing is added to the step -- no term, the RGB pass's loss tensor itself goes into the backward, its bits are
    the regulariser-free step's; gradients and parameters within the distance of two regulariser-free runs from each other.  The
    parameters bit for bit, a test of its own: known to fail on some runs (the blend backward's float atomics; see the test);
  * 24 iterations across 8 990 .. 9 013 with 6 000 samples: the entropy's window, the prune at 9 001 with its Adam moments, the
    neighbours, the regulariser's start, the checkpoint and the point cloud; the command for 3 iterations in a child process.
Each check prints its distance, its bar and its ratio to the yard."""
import functools
import json
import math
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from oracle import optim_reference as orf
from sugar_amd import coarse_draw, coarse_model, coarse_train, io as sio, sdf_regulariser, shims, sugar_patch, synthetic as syn
from sugar_amd import train_step
from tests import coarse_loss_restatement as cl
from tests import optim_cases as oc
from tests import sdf_regulariser_restatement as rs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
FX = np.load(os.path.join(HERE, "golden", "sugar_field.npz"))
REG_FX = np.load(os.path.join(HERE, "golden", "sdf_regulariser.npz"))
CL_FX = np.load(os.path.join(HERE, "golden", "coarse_loss.npz"))
FLOOR, TWO_ULP = 1e-7, 2.0 * 2.0 ** -23
W, H, P = int(FX["W"]), int(FX["H"]), 2500
CAM = int(REG_FX["depth_cam_idx"])
BAND = float(CL_FX["band_threshold"])
N_SAMPLES = 6000
PARAMS = ("_points", "_scales", "_quaternions", "all_densities", "_sh_coordinates_dc", "_sh_coordinates_rest")
STATE_KEYS = dict(_points="state_points", _scales="state_scales", _quaternions="state_quaternions", all_densities="stateall_densities",
                  _sh_coordinates_dc="state_sh_coordinates_dc", _sh_coordinates_rest="state_sh_coordinates_rest")


def _cams():
    return syn.orbit_cameras(W, H)


def _new_model(**kwargs):
    t = lambda k: torch.as_tensor(FX[STATE_KEYS[k]]).to(DEV)
    return coarse_model.CoarseModel(t("_points"), t("_scales"), t("_quaternions"), t("all_densities"), t("_sh_coordinates_dc"),
                                    t("_sh_coordinates_rest"), _cams(), **kwargs)


def _new_standin():
    shims.install()
    from tests.golden.make_sugar_field import p3d_cameras_like_the_reference
    from tests.sugar_regulariser_standin import make_module
    cams = _cams()
    return make_module().SuGaR(FX, DEV, cams, p3d_cameras_like_the_reference(cams).to(DEV))


@functools.lru_cache(maxsize=None)
def _renders():
    """the fixture model's own renders at the eight cameras, [3,H,W] on the CPU: the ground truth of the 24-iteration run"""
    model = _new_model()
    with torch.no_grad():
        return tuple(model.render_image_gaussian_rasterizer(camera_indices=i, sh_deg=3).permute(2, 0, 1).clamp(0, 1).cpu() for i in range(8))


@functools.lru_cache(maxsize=None)
def _targets():
    """ground truth that the fixture model does NOT reproduce (its renders mixed with a smooth pattern), so that the photometric loss
    and its gradient are not zero in the single-step comparisons"""
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    pattern = torch.stack((0.5 + 0.5 * torch.sin(x / 7.0), 0.5 + 0.5 * torch.cos(y / 5.0), 0.5 + 0.5 * torch.sin((x + y) / 11.0)))
    return tuple((0.7 * r + 0.3 * pattern).contiguous() for r in _renders())


def _check(what, got, want, yard):
    got, want = torch.as_tensor(got).detach().cpu(), torch.as_tensor(want).detach().cpu()
    scalar = want.dim() == 0
    d = cl.scalar_distance(got, want) if scalar else rs.distance(got, want)
    bar = max(4.0 * float(yard), TWO_ULP if scalar else FLOOR)
    print(f"{what:44s} distance {d:.3e}   bar {bar:.3e}   yard {float(yard):.3e}   ratio-to-yard {d / max(float(yard), 1e-30):.2f}")
    assert torch.isfinite(got).all(), what
    assert d <= bar, (what, d, bar)


# ------------------------------------------------------------------------------------------------ the model against the stand-in
def test_model_properties_neighbours_normals_and_fields_equal_the_stand_in():
    from sugar_amd.knn import knn_points
    model, standin = _new_model(), _new_standin()
    for name in ("points", "scaling", "strengths", "quaternions", "sh_coordinates"):
        assert torch.equal(getattr(model, name), getattr(standin, name)), name
    assert torch.allclose(model.quaternions.norm(dim=-1), torch.ones(P, device=DEV), atol=1e-6)
    assert model.n_points == P and (model.image_height, model.image_width) == (H, W)
    # the cameras: the same pytorch3d-style cameras as the stand-in's, and the reference's extent
    for i in range(8):
        a, b = model.p3d_cameras[i], standin.nerfmodel.training_cameras.p3d_cameras[i]
        assert torch.equal(a.get_world_to_view_transform().get_matrix(), b.get_world_to_view_transform().get_matrix())
        assert torch.equal(a.get_projection_transform().get_matrix(), b.get_projection_transform().get_matrix())
        assert torch.equal(a.get_camera_center(), b.get_camera_center())
    centers = standin.nerfmodel.training_cameras.p3d_cameras.get_camera_center()
    want = 1.1 * torch.norm(centers - centers.mean(dim=0, keepdim=True), dim=-1).max().item()                  # sugar_model.py:829-833
    assert model.get_cameras_spatial_extent() == pytest.approx(want, rel=1e-6)
    # neighbours: knn_points over the model's own points, self included
    assert model.knn_idx is None
    model.reset_neighbors()
    assert torch.equal(model.knn_idx, knn_points(model.points[None], model.points[None], K=16).idx[0])
    assert model.knn_idx.shape == (P, 16) and torch.equal(model.knn_idx[:, 0], torch.arange(P, device=DEV))
    # normals and the two call shapes of get_field_values `regulariser_terms` makes, on the fixture's samples and neighbours
    model.knn_idx = standin.knn_idx
    assert torch.equal(model.get_normals(estimate_from_points=False), standin.get_normals(estimate_from_points=False))
    x, idx = torch.as_tensor(FX["field_x"]).to(DEV), torch.as_tensor(FX["field_gaussian_idx"]).to(DEV)
    for kw in (dict(return_sdf=True, return_closest_gaussian_opacities=True, return_beta=False),
               dict(return_sdf=False, return_closest_gaussian_opacities=True, return_beta=False),
               dict(return_sdf=False, return_closest_gaussian_opacities=True, return_beta=True)):
        kw.update(density_threshold=1.0, density_factor=1.0 / 16.0, return_sdf_grad=False, sdf_grad_max_value=10.)
        got, want = model.get_field_values(x, idx, **kw), standin.get_field_values(x, idx, **kw)
        assert set(got) == set(want) and "closest_gaussian_opacities" in got and ("sdf" in got) == kw["return_sdf"]
        for k in got:
            assert torch.equal(got[k], want[k]) and got[k].requires_grad, (kw, k)
    with pytest.raises(NotImplementedError, match="not implemented"):
        model.get_field_values(x, idx, return_sdf_grad=True)
    with pytest.raises(NotImplementedError, match="not implemented"):
        model.get_field_values(x, closest_gaussians_idx=model.knn_idx[idx])
    with pytest.raises(NotImplementedError, match="not implemented"):
        model.get_field_values(x)


def test_model_draws_on_the_device_and_weighted_draws_reach_the_torch_path():
    model = _new_model(seed=41)
    mask = torch.as_tensor(REG_FX["sample_mask"]).to(DEV)
    assert model.call == 0
    samples, idx = model.sample_points_in_gaussians(N_SAMPLES, sampling_scale_factor=1.5, mask=mask, probabilities_proportional_to_volume=False)
    assert model.call == 1 and samples.shape == (N_SAMPLES, 3) and samples.requires_grad
    want_idx, want_noise, want_n = coarse_draw.draw_samples(mask, N_SAMPLES, 41, 0)
    want = sdf_regulariser.sample_transform(model.points, model.quaternions, model.scaling, want_idx, want_noise, 1.5)
    assert torch.equal(idx, want_idx) and torch.equal(samples, want) and mask[idx].all()
    assert torch.equal(model.last_draw[0], want_idx) and torch.equal(model.last_draw[1], want_noise) and int(model.last_draw[2]) == int(mask.sum())
    again, _ = model.sample_points_in_gaussians(N_SAMPLES, sampling_scale_factor=1.5, mask=mask, probabilities_proportional_to_volume=False)
    assert model.call == 2 and not torch.equal(again, samples)                  # the next call: other draws
    # weighted draws: the torch statements of sugar_patch.sample_points_in_gaussians, under torch's own generator
    for kw in (dict(probabilities_proportional_to_volume=True), dict(probabilities_proportional_to_volume=False,
                                                                    probabilities_proportional_to_opacity=True)):
        torch.manual_seed(5)
        got = model.sample_points_in_gaussians(N_SAMPLES, sampling_scale_factor=1.5, mask=mask, **kw)
        torch.manual_seed(5)
        want = sugar_patch.sample_points_in_gaussians(model, N_SAMPLES, sampling_scale_factor=1.5, mask=mask, **kw)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and model.call == 2
        assert model.last_draw[1] is None and int(model.last_draw[2]) == int(mask.sum())
    # nothing to choose from: zeros, on either path
    empty = torch.zeros(P, dtype=torch.bool, device=DEV)
    for kw in (dict(probabilities_proportional_to_volume=False), dict(probabilities_proportional_to_volume=True)):
        s, i = model.sample_points_in_gaussians(257, sampling_scale_factor=1.5, mask=empty, **kw)
        assert int(model.last_draw[2]) == 0 and not i.any() and torch.equal(s, model.points[:1].expand(257, 3))


# ------------------------------------------------------------------------------------------------------- single steps, composed
def _load(standin, state):
    with torch.no_grad():
        for name in PARAMS:
            getattr(standin, name).copy_(state[name])
    standin.zero_grad()


def _snapshot(trainer):
    model, opt = trainer.model, trainer.optimizer
    params = {n: getattr(model, n).detach().clone() for n in PARAMS}
    zeros = lambda n: torch.zeros_like(params[n])
    st = {n: opt.state.get(getattr(model, n), {}) for n in PARAMS}
    return dict(params=params, exp_avg={n: st[n]["exp_avg"].clone() if st[n] else zeros(n) for n in PARAMS},
                exp_avg_sq={n: st[n]["exp_avg_sq"].clone() if st[n] else zeros(n) for n in PARAMS},
                step={n: int(st[n]["step"]) if st[n] else 0 for n in PARAMS})


def _radii(standin, ci):
    """radii of the stand-in's render (its `render_image_gaussian_rasterizer` returns the image alone): the same boundary call"""
    from sugar_amd.diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    cam = standin.cams[ci]
    st = GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=torch.zeros(3, device=DEV),
                                       scale_modifier=1., viewmatrix=cam.viewmatrix.to(DEV), projmatrix=cam.projmatrix.to(DEV), sh_degree=0,
                                       campos=cam.campos.to(DEV), prefiltered=False, debug=False)
    with torch.no_grad():
        _, radii = GaussianRasterizer(st)(means3D=standin.points, means2D=torch.zeros(P, 3, device=DEV), shs=None,
                                          colors_precomp=torch.zeros(P, 3, device=DEV), opacities=standin.strengths.view(-1, 1),
                                          scales=standin.scaling, rotations=standin.quaternions, cov3D_precomp=None)
    return radii


def _compose(standin, state, it, ci, gt, dtype, draw=None, knn_idx=None, extent=None):
    """iteration `it` of coarse_sdf.py:504-735 on the stand-in at `state`, the inline statements in `dtype`: (loss, terms, gradients)"""
    _load(standin, state)
    ph = coarse_train.phase(it)
    fov_camera = standin.nerfmodel.training_cameras.p3d_cameras[ci]
    colors = standin.get_points_rgb(positions=standin.points, camera_centers=fov_camera.get_camera_center(), sh_levels=4)     # :2190-2193
    image = standin.render_image_gaussian_rasterizer(camera_indices=ci, bg_color=torch.zeros(3, device=DEV), sh_deg=3, point_colors=colors)
    pred_rgb = image.transpose(-1, -2).transpose(-2, -3)                                                       # coarse_sdf.py:528
    terms = {"rgb_loss": train_step.train_loss(pred_rgb.cpu().to(dtype), gt.to(dtype), 0.2, fused=False).to(DEV)}             # :457, :536
    loss = terms["rgb_loss"]
    visible = _radii(standin, ci) > 0                                                                          # :543
    if ph.entropy:
        vis_opacities = standin.strengths.view(-1, 1).to(dtype)[visible]                                       # :545
        terms["entropy"] = (- vis_opacities * torch.log(vis_opacities + 1e-10)
                            - (1 - vis_opacities) * torch.log(1 - vis_opacities + 1e-10)).mean()               # :548-551
        loss = loss + 0.1 * terms["entropy"]
    if ph.sdf:
        standin.knn_idx = knn_idx
        sample_idx, noise = draw

        def recorded_draw(num_samples, sampling_scale_factor=1., mask=None, **_):
            assert num_samples == len(sample_idx) and mask is not None and bool(mask[sample_idx].all())
            return sdf_regulariser.sample_transform(standin.points, standin.quaternions, standin.scaling, sample_idx, noise,
                                                    float(sampling_scale_factor)), sample_idx
        standin.sample_points_in_gaussians = recorded_draw
        point_depth = fov_camera.get_world_to_view_transform().transform_points(standin.points)[..., 2:].expand(-1, 3)       # :579
        max_depth = point_depth.max()
        depth = standin.render_image_gaussian_rasterizer(camera_indices=ci, bg_color=max_depth + torch.zeros(3, dtype=torch.float, device=DEV),
                                                         sh_deg=0, point_colors=point_depth)[..., 0]            # :581-590
        out = cl.regulariser_terms(standin, fov_camera, depth, visible, dtype=dtype, close_gaussian_threshold=BAND,
                                   n_samples_for_sdf_regularization=N_SAMPLES, cameras_spatial_extent=extent)
        del standin.sample_points_in_gaussians
        for k in ("sdf_estimation_loss", "sdf_better_normal_loss"):
            terms[k] = out[k]
        terms["n_projected"] = out["n_projected"]
        loss = loss + 0.2 * out["sdf_estimation_loss"] + 0.2 * out["sdf_better_normal_loss"]                   # :668, :716
    loss.backward()
    grads = {n: getattr(standin, n).grad.detach().clone() for n in PARAMS}
    return loss.detach(), {k: v.detach() for k, v in terms.items()}, grads


def _check_adam(what, trainer, before, grads, lr_by_param):
    """the parameters and both moments after the step against torch.optim.Adam's update in float64, bars as tests/test_gpu_optim_elements.py"""
    model, opt = trainer.model, trainer.optimizer
    for n in PARAMS:
        p, m, v = (before[k][n].cpu().numpy().reshape(-1) for k in ("params", "exp_avg", "exp_avg_sq"))
        g = grads[n].cpu().numpy().reshape(-1)
        lr = np.full(p.shape, np.float32(lr_by_param[n]))
        args = dict(beta1=0.9, beta2=0.999, eps=1e-15, step=before["step"][n] + 1)
        p1, m1, v1, mags = orf.adam_step(p, g, m, v, lr, **args)
        ya, yb = orf.adam_step_f32(p, g, m, v, lr, **args), orf.adam_step_torch(p, g, m, v, lr, **args)
        st = opt.state[getattr(model, n)]
        assert int(st["step"]) == before["step"][n] + 1
        got = (getattr(model, n).detach(), st["exp_avg"], st["exp_avg_sq"])
        for j, (k, ref, mag) in enumerate((("p", p1, "p"), ("m", m1, "m"), ("v", v1, "v"))):
            label = f"{what} {n} {k}'"
            oc.check(label, oc.element_err(got[j].cpu().numpy().reshape(-1), ref, mags[mag]), oc.bar_from(label, ref, mags[mag], ya[j], yb[j]))


GROUP_OF = {attr: name for name, attr in coarse_train.GROUPS}


def _rates(trainer):
    return {attr: next(g["lr"] for g in trainer.optimizer.param_groups if g["name"] == name) for name, attr in coarse_train.GROUPS}


def test_an_entropy_step_and_an_sdf_step_equal_the_composition_on_the_stand_in():
    model, standin = _new_model(seed=3), _new_standin()
    gts = _targets()
    trainer = coarse_train.CoarseTrainer(model, _cams(), gts, n_samples_for_sdf_regularization=N_SAMPLES, close_gaussian_threshold=BAND)
    assert trainer.extent == model.get_cameras_spatial_extent() == trainer.spatial_lr_scale
    for it in (8000, 9500):
        before = _snapshot(trainer)
        result = trainer.step(it, CAM, return_grads=True)
        rates = _rates(trainer)
        assert rates["_points"] == coarse_train.position_lr(it, trainer.extent)
        assert [rates[n] for n in PARAMS[1:]] == [0.005, 0.001, 0.05, 0.0025, 0.0025 / 20.0]
        if it == 8000:
            assert set(result) == {"rgb_loss", "entropy", "loss", "grads"}
            draw = knn_idx = None
        else:
            assert set(result) == {"rgb_loss", "sdf_estimation_loss", "sdf_better_normal_loss", "n_projected", "n_samples", "n_masked",
                                   "loss", "grads"}
            # not vacuous: a band with Gaussians in it, samples in front of the camera
            print(f"it {it}: n_masked {result['n_masked']}, n_projected {int(result['n_projected'])} of {N_SAMPLES}")
            assert result["n_masked"] >= 256 and int(result["n_projected"]) >= 0.9 * N_SAMPLES and result["n_samples"] == N_SAMPLES
            assert model.call == 1 and int(model.last_draw[2]) == result["n_masked"]
            draw, knn_idx = model.last_draw[:2], model.knn_idx
        runs = {dtype: _compose(standin, before["params"], it, CAM, gts[CAM], dtype, draw, knn_idx, trainer.extent)
                for dtype in (torch.float64, torch.float32)}
        (want_loss, want_terms, want_g), (f32_loss, f32_terms, f32_g) = runs[torch.float64], runs[torch.float32]
        _check(f"it {it} loss", result["loss"], want_loss, cl.scalar_distance(f32_loss, want_loss))
        for k in ("rgb_loss", "entropy", "sdf_estimation_loss", "sdf_better_normal_loss"):
            assert (k in result) == (k in want_terms), k
            if k in result:
                assert torch.isfinite(result[k]) and float(result[k].detach()) > 0, k
                _check(f"it {it} {k}", result[k], want_terms[k], cl.scalar_distance(f32_terms[k], want_terms[k]))
        if it == 9500:
            assert int(result["n_projected"]) == int(want_terms["n_projected"]) == int(f32_terms["n_projected"])
        for n in PARAMS:
            g = result["grads"][GROUP_OF[n]]
            assert g.shape == before["params"][n].shape and g.any(), n
            _check(f"it {it} grad {n}", g, want_g[n], rs.distance(f32_g[n], want_g[n]))
        _check_adam(f"it {it}", trainer, before, {n: result["grads"][GROUP_OF[n]] for n in PARAMS}, rates)
        assert all(getattr(model, n).grad is None for n in PARAMS)


@functools.lru_cache(maxsize=None)
def _empty_band_steps():
    """step 9500 on the fixture's camera by three fresh trainers: `a` with an all-False band (close_gaussian_threshold = 0), `b1` and
    `b2` with `regularize_sdf=False` -- two runs of the SAME step, whose distance is the rasterizer's run-to-run noise"""
    gts = _targets()
    make = lambda **kw: coarse_train.CoarseTrainer(_new_model(), _cams(), gts, n_samples_for_sdf_regularization=N_SAMPLES, **kw)
    trainers = make(close_gaussian_threshold=0.0), make(regularize_sdf=False), make(regularize_sdf=False)
    return trainers, tuple(t.step(9500, CAM, return_grads=True) for t in trainers)


def test_an_empty_band_adds_nothing_to_the_step():
    """what is a pure function of its inputs, bit for bit: no term is returned, the draw was made and found nothing, the tensor that is
    backpropagated IS the RGB pass's loss (the same graph as the regulariser-free step), and its bits are the regulariser-free step's.
    The gradients and parameters pass through the blend backward, whose float atomics (csrc/blend.hip) make two runs of the same
    step differ in the last bits, and Adam can turn that into +-lr for a near-zero gradient: they are held to the distance of the two
    regulariser-free runs from each other -- 3 x that noise, floored at 1e-6 of the gradient's norm / 3e-4 of the update's norm (the
    yardstick and floor of tests/test_gpu_train.py:107-112).  A contribution of the skipped terms -- the NaN of an empty mean, a
    stray factor -- would be orders above it."""
    (a, b1, b2), (ra, r1, r2) = _empty_band_steps()
    assert ra["n_masked"] == 0 and a.n_masked == 0 and "sdf_estimation_loss" not in ra and "sdf_better_normal_loss" not in ra
    assert "n_masked" not in r1 and a.model.call == 1 and b1.model.call == 0          # the draw was made, and found nothing to draw from
    assert ra["loss"] is ra["rgb_loss"] and r1["loss"] is r1["rgb_loss"]              # the same graph: the RGB pass alone
    assert torch.equal(ra["loss"], r1["loss"]) and torch.equal(r1["loss"], r2["loss"])
    for name, attr in coarse_train.GROUPS:
        start = torch.as_tensor(FX[STATE_KEYS[attr]]).to(DEV).reshape(getattr(a.model, attr).shape)
        pa, p1, p2 = (getattr(t.model, attr).detach() for t in (a, b1, b2))
        ga, g1, g2 = (r["grads"][name] for r in (ra, r1, r2))
        g_diff, g_noise, g_norm = float((ga - g1).norm()), float((g1 - g2).norm()), float(g1.norm())
        p_diff, p_noise, upd = float((pa - p1).norm()), float((p1 - p2).norm()), float((p1 - start).norm())
        print(f"{attr:22s} grad: |a - b| {g_diff:.3e}  |b - b'| {g_noise:.3e}  |b| {g_norm:.3e}   params: |a - b| {p_diff:.3e}  "
              f"|b - b'| {p_noise:.3e}  update {upd:.3e}   a == b in {int((pa == p1).sum())} of {pa.numel()}, b == b' in {int((p1 == p2).sum())}")
        assert torch.isfinite(pa).all() and torch.isfinite(ga).all(), attr
        assert upd > 0 and g_norm > 0, attr                                          # the step did move them
        assert g_diff <= max(3.0 * g_noise, 1e-6 * g_norm), (attr, g_diff, g_noise, g_norm)
        assert p_diff <= max(3.0 * p_noise, 3e-4 * upd), (attr, p_diff, p_noise, upd)


def test_an_empty_band_gives_the_step_without_the_regulariser_bit_for_bit():
    """the parameters after the empty-band step against those after the regulariser-free step, `torch.equal` on every group.

    KNOWN TO FAIL ON SOME RUNS.  The two steps submit the same work (test_an_empty_band_adds_nothing_to_the_step), but the blend
    backward sums a Gaussian's gradient over its tiles with float atomics, so two runs of the SAME step differ in the last bits of
    the gradients and, now and then, of a parameter; no loop over this rasterizer can promise equal bits here.  Recorded on an
    MI355X, six runs: two equal in every bit of every group, four not -- each time one element of the 112 500 of
    `_sh_coordinates_rest` (2.9e-11 off), once also one of the 2 500 of `all_densities` (3.7e-9 off); where it was measured, the two
    regulariser-free runs differed from each other in one element of `_sh_coordinates_rest` by the same amount (gradients 4e-12 ..
    4e-10 apart norm-wise either way, norms 7e-4 .. 3e-2)."""
    (a, b1, _), _ = _empty_band_steps()
    unequal = [attr for _, attr in coarse_train.GROUPS if not torch.equal(getattr(a.model, attr), getattr(b1.model, attr))]
    assert not unequal, unequal


# ------------------------------------------------------------------------------------------------------------ the 24 iterations
def test_twenty_four_iterations_across_the_prune_and_the_regularisers_start(tmp_path):
    model = _new_model(seed=9)
    trainer = coarse_train.CoarseTrainer(model, _cams(), _renders(), n_samples_for_sdf_regularization=N_SAMPLES, close_gaussian_threshold=BAND,
                                         num_iterations=9013)
    captured = {}
    prune = model.prune

    def spy(keep_mask, optimizer=None):
        captured["before"] = _snapshot(trainer)
        captured["strengths"] = model.strengths.detach().clone()
        prune(keep_mask, optimizer)
        captured["keep"], captured["after"] = keep_mask.clone(), _snapshot(trainer)
    model.prune = spy
    resets = []
    reset = model.reset_neighbors
    model.reset_neighbors = lambda *a, **k: (resets.append(it), reset(*a, **k))[1]
    for it in range(8990, 9014):
        result = trainer.step(it, it % 8)
        assert ("entropy" in result) == (it <= 8999), it                        # 7000 < it < 9000
        assert ("keep" in captured) == (it >= 9001), it                         # the prune: at the start of 9001
        sdf = "sdf_estimation_loss" in result and "sdf_better_normal_loss" in result
        assert sdf == (it >= 9001), (it, result.get("n_masked"))                # it > 9000 (and a band that is not empty)
        if sdf:
            assert result["n_masked"] > 0 and int(result["n_projected"]) > 0
        assert all(torch.isfinite(v).all() for k, v in result.items() if torch.is_tensor(v)), it
    assert resets == [9000, 9001]                                               # it % 500 == 0, then after the prune
    keep = captured["keep"].reshape(-1)
    P2 = int(keep.sum())
    assert torch.equal(keep, (captured["strengths"] >= 0.5).reshape(-1)) and 0 < P2 < P and model.n_points == P2
    print(f"pruned {P} -> {P2} Gaussians")
    for n in PARAMS:                                                            # the kept rows, with their Adam moments, row by row
        for k in ("params", "exp_avg", "exp_avg_sq"):
            assert torch.equal(captured["after"][k][n], captured["before"][k][n][keep]), (n, k)
        assert captured["after"]["step"][n] == captured["before"]["step"][n] == 9000 - 8990 + 1
        assert captured["before"]["exp_avg"][n].any()
        st = trainer.optimizer.state[getattr(model, n)]
        assert int(st["step"]) == 24 and st["exp_avg"].shape == getattr(model, n).shape
        assert getattr(model, n).shape[0] == P2 and torch.isfinite(getattr(model, n)).all(), n
    assert model.knn_idx.shape == (P2, 16) and int(model.knn_idx.max()) < P2 and int(model.knn_idx.min()) >= 0
    assert model.call == 9013 - 9000
    ck, ply = str(tmp_path / "9013.pt"), str(tmp_path / "point_cloud.ply")
    trainer.save(ck, 9013)
    model.save_ply(ply)
    loaded = torch.load(ck, map_location="cpu")
    assert set(loaded) == {"state_dict", "train_losses", "epoch", "iteration", "optimizer_state_dict"} and loaded["iteration"] == 9013
    assert list(loaded["state_dict"]) == list(coarse_model.PARAMETER_NAMES)
    for n in PARAMS:
        assert loaded["state_dict"][n].shape[0] == P2 and torch.equal(loaded["state_dict"][n], getattr(model, n).detach().cpu()), n
    g = sio.load_gaussian_ply(ply)
    assert g["xyz"].shape == (P2, 3) and g["features"].shape == (P2, 16, 3) and torch.equal(g["xyz"], model._points.detach().cpu())


def _camera_json(i, cam):
    w2c = cam.viewmatrix.cpu().numpy().T.astype(np.float64)
    return sio.camera_to_json(i, f"view_{i:03d}", w2c[:3, :3].T, w2c[:3, 3], 2 * math.atan(cam.tanfovx), 2 * math.atan(cam.tanfovy),
                              cam.image_width, cam.image_height)


def test_the_command_runs_three_iterations_in_a_child_process(tmp_path):
    from PIL import Image
    model = _new_model()
    model.save_ply(str(tmp_path / "in.ply"))
    cams = _cams()
    (tmp_path / "cameras.json").write_text(json.dumps([_camera_json(i, c) for i, c in enumerate(cams)]))
    os.makedirs(tmp_path / "images")
    for i, r in enumerate(_renders()):
        Image.fromarray((r.permute(1, 2, 0) * 255.0).round().to(torch.uint8).numpy()).save(str(tmp_path / "images" / f"view_{i:03d}.png"))
    out = tmp_path / "out"
    run = subprocess.run([sys.executable, "-m", "sugar_amd.coarse_train", str(tmp_path / "in.ply"), "--cameras", str(tmp_path / "cameras.json"),
                          "--images", str(tmp_path / "images"), "--out", str(out), "--start-iteration", "8999", "--iterations", "9002",
                          "--samples", str(N_SAMPLES), "--seed", "1"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(run.stdout[-2000:], run.stderr[-2000:])
    assert run.returncode == 0
    assert (out / "9002.pt").is_file() and (out / "point_cloud.ply").is_file()
    state = torch.load(str(out / "9002.pt"), map_location="cpu")["state_dict"]
    g = sio.load_gaussian_ply(str(out / "point_cloud.ply"))
    assert 0 < state["_points"].shape[0] < P and g["xyz"].shape == state["_points"].shape       # the prune at 9001 ran
