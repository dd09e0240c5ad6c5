"""GPU tests of the native density regulariser: coarse_loss.projection_estimation_losses (csrc/coarse_loss.hip, sgr_projection_loss_*),
coarse_loss.density_regulariser_terms and CoarseTrainer(regulariser='density').

  * values and all five gradients against tests/golden/coarse_density.npz, which the reference's own model wrote, and against the
    float64 restatement (tests/coarse_density_restatement.py) on the same inputs: a scalar within max(4 x yard, 2 float32 ulp), an
    array norm-wise within max(4 x yard, 1e-7) -- the bars of tests/test_gpu_coarse_loss.py; the yard is the distance of the float32
    statements from the float64 ones;
  * edge shapes against float64: N in {1, 255, 256, 257, 6000} x P in {1, 257, 2500}; all 6 000 samples in one Gaussian; Gaussians
    without a sample get exact zero rows in outputs prefilled with NaN; a negative index that wraps; indices outside [-P, P)
    contribute nothing while the divisor stays N; beta = 1e-20; est == 0 and density == target planted in chosen rows;
  * two runs are bit-identical in the value and in all five gradients, and neither synchronises with the host;
  * the composite on `CoarseModel` with the fixture's recorded draw injected: against the float64 restatement on the same model, and
    against the gradients of the model's parameters that the reference's own autograd recorded;
  * one trainer step at 9 500 with regulariser='density' against a composition written out here, and its Adam update;
  * 24 iterations across 8 990 .. 9 013 and the command in a child process.
Each check prints its distance, its bar and its ratio to the yard."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from sugar_amd import _lib, coarse_loss, coarse_model, coarse_train, io as sio, sdf_regulariser, train_step
from sugar_amd._call import call, ptr
from tests import coarse_density_restatement as cd
from tests import sdf_regulariser_restatement as rs
from tests import test_gpu_coarse_train as tct         # its helpers: the fixture model, the stand-in, the snapshot and the Adam check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
FX = np.load(os.path.join(HERE, "golden", "coarse_density.npz"))
FIELD_FX = np.load(os.path.join(HERE, "golden", "sugar_field.npz"))
FLOOR, TWO_ULP = 1e-7, 2.0 * 2.0 ** -23
EXTENT = float(FX["extent"])
CAM = int(FX["cam_idx"])
N_SAMPLES, P = 6000, 2500
PARAMS = tct.PARAMS

from tests.golden.make_coarse_density import MODEL_PARAMS, SURFACE_WEIGHT, VARIANTS  # noqa: E402

RATIOS = {}


def _t(k, fx=FX):
    return torch.as_tensor(fx[k])


def _check(what, got, want, yard, floor=None):
    """an array within max(4 yard, FLOOR) norm-wise, a scalar within max(4 yard, 2 ulp) relative"""
    got, want = torch.as_tensor(got).detach().cpu(), torch.as_tensor(want).detach().cpu()
    scalar = want.dim() == 0
    d = cd.scalar_distance(got, want) if scalar else rs.distance(got, want)
    bar = max(4.0 * float(yard), (TWO_ULP if scalar else FLOOR) if floor is None else floor)
    ratio = d / max(float(yard), 1e-30)
    print(f"{what:52s} distance {d:.3e}   bar {bar:.3e}   yard {float(yard):.3e}   ratio-to-yard {ratio:.2f}")
    assert torch.isfinite(got).all(), what
    assert d <= bar, (what, d, bar)
    return ratio


GRADS = ("grad_samples", "grad_field", "grad_beta", "grad_points", "grad_normals")


def _op(x, idx, points, normals, sdf, density, beta, opts, extent=EXTENT):
    """the operation on device copies; (est, surf, {gradients})"""
    leaves = [t.to(DEV).clone().requires_grad_(True) for t in (x, sdf, density, beta, points, normals)]
    est, surf = coarse_loss.projection_estimation_losses(leaves[0], idx.to(DEV), leaves[4], leaves[5], sdf=leaves[1], density=leaves[2],
                                                         beta=leaves[3], scale=extent / 10., clamp_max=10. * extent, **opts)
    (est + SURFACE_WEIGHT * surf if surf is not None else est).backward()
    field = leaves[1] if opts["mode"] == "sdf" else leaves[2]
    return est, surf, dict(grad_samples=leaves[0].grad, grad_field=field.grad, grad_beta=leaves[3].grad if opts["mode"] == "density" else None,
                           grad_points=leaves[4].grad, grad_normals=leaves[5].grad)


def _restated(x, idx, points, normals, sdf, density, beta, opts, dtype, extent=EXTENT):
    """the restatement on the CPU in `dtype`.  Samples whose index is outside [-P, P) are left out and the means rescaled to the
    divisor N (exact in float64: the two differ by the factor n_valid / N)"""
    Pn, N = points.shape[0], x.shape[0]
    ok = (idx >= -Pn) & (idx < Pn)
    leaves = [t.to(dtype).clone().requires_grad_(True) for t in (x, sdf, density, beta, points, normals)]
    est, surf = cd.projection_estimation_losses(leaves[0][ok], idx[ok], leaves[4], leaves[5], sdf=leaves[1][ok], density=leaves[2][ok],
                                                beta=leaves[3][ok], scale=extent / 10., clamp_max=10. * extent, **opts)
    f = float(ok.sum()) / N
    est = est * f if est is not None else None
    surf = surf * f if surf is not None else None
    (est + SURFACE_WEIGHT * surf if surf is not None else est).backward()
    zero = lambda t: t.grad if t.grad is not None else torch.zeros_like(t)
    field = leaves[1] if opts["mode"] == "sdf" else leaves[2]
    return est.detach(), None if surf is None else surf.detach(), dict(
        grad_samples=zero(leaves[0]), grad_field=zero(field), grad_beta=zero(leaves[3]) if opts["mode"] == "density" else None,
        grad_points=zero(leaves[4]), grad_normals=zero(leaves[5]))


def _fixture_inputs():
    return (_t("samples"), _t("sample_idx").to(torch.int64), _t("state_points", FIELD_FX), _t("normals"), _t("field_sdf"), _t("field_density"),
            _t("field_beta"))


# ------------------------------------------------------------------------------------------------------------------ the fixture
@pytest.mark.parametrize("tag", list(VARIANTS))
def test_values_and_gradients_match_the_fixture_and_float64(tag):
    opts = VARIANTS[tag]
    inputs = _fixture_inputs()
    est, surf, g = _op(*inputs, opts)
    est2, surf2, g2 = _op(*inputs, opts)
    want_est, want_surf, want_g = _restated(*inputs, opts, torch.float64)
    assert est.dim() == 0 and est.device.type == "cuda"
    worst = 0.0
    for want, label in ((lambda k: FX[f"{tag}_{k}"], "fixture"), (lambda k: dict(loss_est=want_est, loss_surf=want_surf, **want_g)[k], "float64")):
        worst = max(worst, _check(f"{tag} loss_est / {label}", est, want("loss_est"), FX[f"yard_{tag}_loss_est"]))
        if surf is not None:
            worst = max(worst, _check(f"{tag} loss_surf / {label}", surf, want("loss_surf"), FX[f"yard_{tag}_loss_surf"]))
        for k in GRADS:
            if g[k] is None:
                assert opts["mode"] == "sdf" and k == "grad_beta"
                continue
            worst = max(worst, _check(f"{tag} {k} / {label}", g[k], want(k), FX[f"yard_{tag}_{k}"]))
    print(f"{tag}: largest ratio to yard {worst:.2f}")
    # the Gaussians without a sample: exact zero rows; a Gaussian with one sample is touched (with several, the 'sdf' terms' gradients
    # -- multiples of 1 / (N s) -- can cancel exactly)
    counts = torch.as_tensor(np.bincount(FX["sample_idx"], minlength=P))
    for k in ("grad_points", "grad_normals"):
        assert g[k].shape == (P, 3) and not g[k][(counts == 0).to(DEV)].any() and g[k][(counts == 1).to(DEV)].any(dim=-1).all(), k
    # bit-identical from run to run
    assert torch.equal(est, est2) and (surf is None or torch.equal(surf, surf2))
    assert all(g[k] is None or torch.equal(g[k], g2[k]) for k in GRADS)


# ------------------------------------------------------------------------------------------------------------------ edge shapes
def _random_case(N, Pn, seed, one_gaussian=False):
    """points on a blob, unit normals, samples around their Gaussians, fields in the trainer's ranges.  The seed is advanced until, in
    float64, no sample lies within 1e-4 of a kink (relative to the term's median magnitude), as the fixture's maker does."""
    for s in range(seed, seed + 200):
        g = torch.Generator().manual_seed(s)
        points = 0.6 * torch.nn.functional.normalize(torch.randn(Pn, 3, generator=g), dim=-1)
        normals = torch.nn.functional.normalize(torch.randn(Pn, 3, generator=g), dim=-1)
        idx = torch.full((N,), Pn // 2, dtype=torch.int64) if one_gaussian else torch.randint(0, Pn, (N,), generator=g)
        x = points[idx] + 0.05 * torch.randn(N, 3, generator=g)
        density, beta = 0.05 + 0.9 * torch.rand(N, generator=g), 0.02 + 0.08 * torch.rand(N, generator=g)
        sdf = 0.1 * torch.rand(N, generator=g)
        est = cd.projection_estimate(x.double(), idx, points.double(), normals.double())
        d = density.double() - torch.exp(-0.5 * est.pow(2) / beta.double().pow(2))
        t = sdf.double() - est.abs()
        if min(float(d.abs().min()) / 0.3, float(est.abs().min()) / 0.03, float(t.abs().min()) / 0.05) >= 1e-4:
            return x, idx, points, normals, sdf, density, beta
    raise AssertionError("no seed keeps the samples off the kinks")


def _against_float64(what, inputs, opts, nan_to_zero=False):
    """the operation against the float64 restatement of the same inputs; the yards are the float32 restatement's distances from it.
    `nan_to_zero`: where torch's float32 autograd gives 0 * inf = NaN (a vanishing beta) the yard takes the float64 value, 0"""
    est, surf, g = _op(*inputs, opts)
    want = _restated(*inputs, opts, torch.float64)
    f32 = _restated(*inputs, opts, torch.float32)
    yard = lambda a, b: cd.scalar_distance(a, b) if b.dim() == 0 else rs.distance(torch.nan_to_num(a, nan=0.0) if nan_to_zero else a, b)
    _check(f"{what} loss_est", est, want[0], yard(f32[0], want[0]))
    if surf is not None:
        _check(f"{what} loss_surf", surf, want[1], yard(f32[1], want[1]))
    for k in GRADS:
        if g[k] is not None:
            _check(f"{what} {k}", g[k], want[2][k], yard(f32[2][k], want[2][k]))
    return est, surf, g, want


@pytest.mark.parametrize("Pn", [1, 257, 2500])
@pytest.mark.parametrize("N", [1, 255, 256, 257, 6000])
def test_shapes_against_float64(N, Pn):
    inputs = _random_case(N, Pn, 1000 * N + Pn)
    for tag, opts in VARIANTS.items():
        est, surf, g, _ = _against_float64(f"N={N} P={Pn} {tag}", inputs, opts)
        assert g["grad_samples"].shape == (N, 3) and g["grad_points"].shape == (Pn, 3) and g["grad_normals"].shape == (Pn, 3)


def test_every_sample_in_one_gaussian():
    inputs = _random_case(6000, 257, 77, one_gaussian=True)
    for tag, opts in VARIANTS.items():
        _, _, g, _ = _against_float64(f"one Gaussian {tag}", inputs, opts)
        rest = torch.arange(257) != 257 // 2
        assert not g["grad_points"][rest.to(DEV)].any() and not g["grad_normals"][rest.to(DEV)].any()
        assert g["grad_points"][257 // 2].any() and g["grad_normals"][257 // 2].any()


def test_gaussians_without_a_sample_get_exact_zero_rows_in_nan_prefilled_outputs():
    """the C entry point itself, with every output prefilled with NaN: every row of every output is written"""
    N, Pn = 257, 2500
    x, idx, points, normals, sdf, density, beta = (t.to(DEV).contiguous() for t in _random_case(N, Pn, 5))
    lib = _lib.load()
    one = torch.ones(1, device=DEV)
    for mode, flags, field in ((1, 4, density), (0, 4 | 8, sdf)):
        outs = [torch.full(shape, float("nan"), device=DEV) for shape in ((N,), (N,), (N, 3), (Pn, 3), (Pn, 3))]
        scratch = torch.empty(max(lib.sgr_projection_loss_backward_scratch_bytes(N, Pn), 256), dtype=torch.uint8, device=DEV)
        call("sgr_projection_loss_backward", torch.device(DEV), N, Pn, mode, flags, ptr(x), ptr(idx), ptr(points), ptr(normals), ptr(field),
             ptr(beta), EXTENT / 10., 10. * EXTENT, ptr(one), ptr(one), *(ptr(o) for o in outs), ptr(scratch))
        dfield, dbeta, dx, dp, dn = outs
        counts = torch.bincount(idx, minlength=Pn)
        assert torch.isfinite(dfield).all() and torch.isfinite(dx).all() and torch.isfinite(dp).all() and torch.isfinite(dn).all()
        assert torch.isfinite(dbeta).all() if mode == 1 else torch.isnan(dbeta).all()       # mode 'sdf' does not write dL_dbeta
        assert int((counts == 0).sum()) > 2000
        assert not dp[counts == 0].any() and not dn[counts == 0].any()
        if mode == 1:                                                           # (in mode 'sdf' with both upstream gradients 1 a sample's
            assert dp[counts > 0].any(dim=-1).all() and dn[counts > 0].any(dim=-1).all()      # two slopes -+1 / (N s) can cancel exactly)


def test_a_negative_index_wraps_and_an_index_out_of_range_contributes_nothing():
    N, Pn = 257, 257
    x, idx, points, normals, sdf, density, beta = _random_case(N, Pn, 9)
    wrapped = idx.clone()
    wrapped[::3] -= Pn                                                          # the same Gaussians, named from the end
    for tag, opts in VARIANTS.items():
        a = _op(x, idx, points, normals, sdf, density, beta, opts)
        b = _op(x, wrapped, points, normals, sdf, density, beta, opts)
        assert torch.equal(a[0], b[0]) and all(a[2][k] is None or torch.equal(a[2][k], b[2][k]) for k in GRADS), tag
    out = wrapped.clone()
    bad = torch.tensor([0, 5, 100, 255, 256])
    out[bad] = torch.tensor([Pn, -Pn - 1, 2 ** 40, -2 ** 40, Pn + 7])
    for tag, opts in VARIANTS.items():
        inputs = (x, out, points, normals, sdf, density, beta)
        est, surf, g, want = _against_float64(f"out of range {tag}", inputs, opts)
        # the divisor stays N: the value is the sum over the 252 valid samples / 257
        valid = torch.ones(N, dtype=torch.bool); valid[bad] = False
        sub = _restated(x[valid], wrapped[valid], points, normals, sdf[valid], density[valid], beta[valid], opts, torch.float64)
        assert cd.scalar_distance(want[0], sub[0] * (N - len(bad)) / N) < 1e-12
        for k in ("grad_samples", "grad_field", "grad_beta"):
            assert g[k] is None or not g[k][bad.to(DEV)].any(), (tag, k)


def test_a_vanishing_beta_gives_a_zero_target_and_finite_gradients():
    N, Pn = 257, 257
    x, idx, points, normals, sdf, density, beta = _random_case(N, Pn, 13)
    beta = beta.clone(); beta[::2] = 1e-20
    for tag in ("den", "den_sq"):
        est, _, g, want = _against_float64(f"beta 1e-20 {tag}", (x, idx, points, normals, sdf, density, beta), VARIANTS[tag], nan_to_zero=True)
        assert all(torch.isfinite(g[k]).all() for k in GRADS)
        assert not g["grad_beta"][::2].any() and not g["grad_samples"][::2].any()       # the target is 0 there: nothing flows through it
        assert g["grad_field"][::2].all()


def test_planted_kinks_pass_exactly_zero():
    N, Pn = 256, 257
    x, drawn, points, normals, sdf, density, beta = _random_case(N, Pn, 21)
    idx = torch.arange(N)                                                       # one sample per Gaussian: the rows can be read off
    x = points[idx] + (x - points[drawn])
    rows = torch.tensor([0, 63, 64, 255])
    x[rows] = points[rows]                                                      # est == 0 exactly
    density = density.clone(); density[rows[:2]] = 1.0                          # ... and there the target is exp(0) = 1 == density
    for tag, opts in VARIANTS.items():
        est, surf, g, want = _against_float64(f"kinks {tag}", (x, idx, points, normals, sdf, density, beta), opts)
        dev_rows = rows.to(DEV)
        for k in ("grad_samples", "grad_points", "grad_normals"):              # d|x|/dx = 0 at 0; est^2 has slope 0 at 0
            assert not g[k][dev_rows].any(), (tag, k)
        if opts["mode"] == "density":
            assert not g["grad_field"][dev_rows[:2]].any() and not g["grad_beta"][dev_rows].any()      # sign(0) = 0 / 2 * 0
            assert g["grad_field"][dev_rows[2:]].all()
        else:
            assert g["grad_field"][dev_rows].all()                              # |sdf - 0| / s: the field's own slope stays
        assert g["grad_samples"][1].any() and g["grad_points"][1].any() and g["grad_normals"][1].any()


def test_two_runs_are_bit_identical_and_neither_synchronises_with_the_host():
    inputs = [t.to(DEV) for t in _fixture_inputs()]

    def run():
        out = []
        for opts in VARIANTS.values():
            leaves = [t.clone().requires_grad_(True) for t in (inputs[0], inputs[4], inputs[5], inputs[6], inputs[2], inputs[3])]
            est, surf = coarse_loss.projection_estimation_losses(leaves[0], inputs[1], leaves[4], leaves[5], sdf=leaves[1], density=leaves[2],
                                                                 beta=leaves[3], scale=EXTENT / 10., clamp_max=10. * EXTENT, **opts)
            (est + surf if surf is not None else est).backward()
            out += [est, surf] + [t.grad for t in leaves]
        return out
    run(); torch.cuda.synchronize()                                             # (warm: code objects, the allocator)
    torch.cuda.set_sync_debug_mode("error")
    try:
        a, b = run(), run()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert len(a) == 24
    for u, v in zip(a, b):
        assert (u is None and v is None) or torch.equal(u, v)


# ------------------------------------------------------------------------------------------------------------------ the composite
def _inject(model, sample_idx, noise):
    def recorded_draw(num_samples, sampling_scale_factor=1., mask=None, **_):
        assert num_samples == len(sample_idx) and mask is not None and bool(mask[sample_idx].all())
        return sdf_regulariser.sample_transform(model.points, model.quaternions, model.scaling, sample_idx, noise,
                                                float(sampling_scale_factor)), sample_idx
    model.sample_points_in_gaussians = recorded_draw


def test_the_composite_on_the_model_equals_float64_and_the_references_parameter_gradients():
    """`density_regulariser_terms` on `CoarseModel` with the fixture's draw (sample_idx, noise) injected.  Against the float64
    restatement on the SAME model the method calls are the same kernels on both sides, so the inline yard and the bars above apply.
    Against the reference's own autograd (`model_*` of the fixture) the sampler, the field and the normals are this package's kernels
    on one side and the reference's CPU methods on the other: there the bar is floored at what tests/test_gpu_sugar_field.py and
    tests/test_gpu_sdf_regulariser.py already hold those kernels to against the same reference -- 2e-5 for a value, 1e-4 norm-wise
    for a parameter gradient."""
    model = tct._new_model()
    model.knn_idx = _t("state_knn_idx", FIELD_FX).to(DEV)
    visible = _t("sample_mask").to(DEV)
    _inject(model, _t("sample_idx").to(torch.int64).to(DEV), _t("sample_noise").to(DEV))
    kw = dict(n_samples_for_sdf_regularization=N_SAMPLES, cameras_spatial_extent=EXTENT)

    def run(fn, **more):
        model.zero_grad()
        out = fn(model, visible, **kw, **more)
        (out["sdf_estimation_loss"] + out["sdf_better_normal_loss"]).backward()
        return out, {n: getattr(model, n).grad.detach().clone() for n in MODEL_PARAMS}
    got, got_g = run(coarse_loss.density_regulariser_terms)
    again, again_g = run(coarse_loss.density_regulariser_terms)
    want, want_g = run(cd.density_regulariser_terms, dtype=torch.float64)
    f32, f32_g = run(cd.density_regulariser_terms, dtype=torch.float32)
    assert set(got) == {"sdf_estimation_loss", "sdf_better_normal_loss", "n_samples"} and got["n_samples"] == N_SAMPLES
    for k in ("sdf_estimation_loss", "sdf_better_normal_loss"):
        _check(f"composite {k}", got[k], want[k], cd.scalar_distance(f32[k], want[k]))
        assert torch.equal(got[k], again[k])
    for n in MODEL_PARAMS:
        _check(f"composite grad {n}", got_g[n], want_g[n], rs.distance(f32_g[n], want_g[n]))
        assert torch.equal(got_g[n], again_g[n]), n
    _check("samples / reference", want["samples"], FX["samples"], 0.0, floor=2e-5)
    _check("sdf_estimation_loss / reference", got["sdf_estimation_loss"], FX["model_loss_est"], FX["yard_model_loss_est"], floor=2e-5)
    _check("sdf_better_normal_loss / reference", got["sdf_better_normal_loss"], FX["model_loss_normal"], FX["yard_model_loss_normal"], floor=2e-5)
    for n in MODEL_PARAMS:
        _check(f"grad {n} / reference", got_g[n], FX["model_grad" + n], FX["yard_model_grad" + n], floor=1e-4)


# ------------------------------------------------------------------------------------------------------------------ a trainer step
def _compose(standin, state, ci, gt, dtype, draw, knn_idx, extent):
    """iteration 9500 of coarse_density.py:504-735 (default options) on the stand-in at `state`, the inline statements in `dtype`"""
    tct._load(standin, state)
    fov_camera = standin.nerfmodel.training_cameras.p3d_cameras[ci]
    colors = standin.get_points_rgb(positions=standin.points, camera_centers=fov_camera.get_camera_center(), sh_levels=4)
    image = standin.render_image_gaussian_rasterizer(camera_indices=ci, bg_color=torch.zeros(3, device=DEV), sh_deg=3, point_colors=colors)
    pred_rgb = image.transpose(-1, -2).transpose(-2, -3)
    terms = {"rgb_loss": train_step.train_loss(pred_rgb.cpu().to(dtype), gt.to(dtype), 0.2, fused=False).to(DEV)}
    visible = tct._radii(standin, ci) > 0                                                                      # coarse_density.py:562, :574
    standin.knn_idx = knn_idx
    sample_idx, noise = draw

    def recorded_draw(num_samples, sampling_scale_factor=1., mask=None, **_):
        assert num_samples == len(sample_idx) and mask is not None and bool(mask[sample_idx].all())
        return sdf_regulariser.sample_transform(standin.points, standin.quaternions, standin.scaling, sample_idx, noise,
                                                float(sampling_scale_factor)), sample_idx
    standin.sample_points_in_gaussians = recorded_draw
    out = cd.density_regulariser_terms(standin, visible, dtype=dtype, n_samples_for_sdf_regularization=N_SAMPLES, cameras_spatial_extent=extent)
    del standin.sample_points_in_gaussians
    for k in ("sdf_estimation_loss", "sdf_better_normal_loss"):
        terms[k] = out[k]
    loss = terms["rgb_loss"] + 0.2 * out["sdf_estimation_loss"] + 0.2 * out["sdf_better_normal_loss"]          # :691, :730
    loss.backward()
    grads = {n: getattr(standin, n).grad.detach().clone() for n in PARAMS}
    return loss.detach(), {k: v.detach() for k, v in terms.items()}, grads


def test_a_density_step_equals_the_composition_on_the_stand_in():
    model, standin = tct._new_model(seed=3), tct._new_standin()
    gts = tct._targets()
    trainer = coarse_train.CoarseTrainer(model, tct._cams(), gts, n_samples_for_sdf_regularization=N_SAMPLES, regulariser="density")
    o = trainer.options
    assert (o["sdf_estimation_mode"], o["density_factor"], o["use_projection_as_estimation"], o["sample_only_in_gaussians_close_to_surface"]) == (
        "density", 1.0, True, False)
    renders = []
    render = model.render_image_gaussian_rasterizer
    model.render_image_gaussian_rasterizer = lambda *a, **k: (renders.append(k), render(*a, **k))[1]
    before = tct._snapshot(trainer)
    result = trainer.step(9500, CAM, return_grads=True)
    rates = tct._rates(trainer)
    assert len(renders) == 1 and renders[0].get("point_colors") is None         # the RGB pass alone: no depth render
    assert set(result) == {"rgb_loss", "sdf_estimation_loss", "sdf_better_normal_loss", "n_samples", "n_masked", "loss", "grads"}
    print(f"n_masked {result['n_masked']} of {P}")
    assert result["n_masked"] >= 256 and result["n_samples"] == N_SAMPLES
    assert model.call == 1 and int(model.last_draw[2]) == result["n_masked"]
    draw, knn_idx = model.last_draw[:2], model.knn_idx
    runs = {dtype: _compose(standin, before["params"], CAM, gts[CAM], dtype, draw, knn_idx, trainer.extent) for dtype in (torch.float64, torch.float32)}
    (want_loss, want_terms, want_g), (f32_loss, f32_terms, f32_g) = runs[torch.float64], runs[torch.float32]
    tct._check("density step loss", result["loss"], want_loss, cd.scalar_distance(f32_loss, want_loss))
    for k in ("rgb_loss", "sdf_estimation_loss", "sdf_better_normal_loss"):
        assert torch.isfinite(result[k]) and float(result[k].detach()) > 0, k
        tct._check(f"density step {k}", result[k], want_terms[k], cd.scalar_distance(f32_terms[k], want_terms[k]))
    for n in PARAMS:
        g = result["grads"][tct.GROUP_OF[n]]
        assert g.shape == before["params"][n].shape and g.any(), n
        tct._check(f"density step grad {n}", g, want_g[n], rs.distance(f32_g[n], want_g[n]))
    tct._check_adam("density step", trainer, before, {n: result["grads"][tct.GROUP_OF[n]] for n in PARAMS}, rates)
    assert all(getattr(model, n).grad is None for n in PARAMS)


# ------------------------------------------------------------------------------------------------- the schedule and the command
def test_twenty_four_density_iterations_across_the_prune_and_the_regularisers_start(tmp_path):
    model = tct._new_model(seed=9)
    trainer = coarse_train.CoarseTrainer(model, tct._cams(), tct._renders(), n_samples_for_sdf_regularization=N_SAMPLES, num_iterations=9013,
                                         regulariser="density")
    captured, resets, renders = {}, [], []
    prune, reset, render = model.prune, model.reset_neighbors, model.render_image_gaussian_rasterizer

    def spy(keep_mask, optimizer=None):
        captured["strengths"] = model.strengths.detach().clone()
        prune(keep_mask, optimizer)
        captured["keep"] = keep_mask.clone()
    model.prune = spy
    model.reset_neighbors = lambda *a, **k: (resets.append(it), reset(*a, **k))[1]
    model.render_image_gaussian_rasterizer = lambda *a, **k: (renders.append((it, k.get("point_colors") is not None)), render(*a, **k))[1]
    for it in range(8990, 9014):
        result = trainer.step(it, it % 8)
        assert ("entropy" in result) == (it <= 8999), it
        assert ("keep" in captured) == (it >= 9001), it                         # the prune: at the start of 9001
        started = "sdf_estimation_loss" in result and "sdf_better_normal_loss" in result
        assert started == (it >= 9001), (it, result.get("n_masked"))            # the regulariser: it > 9000
        if started:
            assert result["n_masked"] > 0 and "n_projected" not in result
        assert all(torch.isfinite(v).all() for k, v in result.items() if torch.is_tensor(v)), it
    assert resets == [9000, 9001]                                               # it % 500 == 0, then after the prune
    assert renders == [(it, False) for it in range(8990, 9014)]                 # one RGB render per iteration, no depth render
    keep = captured["keep"].reshape(-1)
    P2 = int(keep.sum())
    assert torch.equal(keep, (captured["strengths"] >= 0.5).reshape(-1)) and 0 < P2 < P and model.n_points == P2
    assert model.knn_idx.shape == (P2, 16) and model.call == 9013 - 9000
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


def test_the_command_runs_three_density_iterations_in_a_child_process(tmp_path):
    from PIL import Image
    model = tct._new_model()
    model.save_ply(str(tmp_path / "in.ply"))
    cams = tct._cams()
    (tmp_path / "cameras.json").write_text(json.dumps([tct._camera_json(i, c) for i, c in enumerate(cams)]))
    os.makedirs(tmp_path / "images")
    for i, r in enumerate(tct._renders()):
        Image.fromarray((r.permute(1, 2, 0) * 255.0).round().to(torch.uint8).numpy()).save(str(tmp_path / "images" / f"view_{i:03d}.png"))
    out = tmp_path / "out"
    run = subprocess.run([sys.executable, "-m", "sugar_amd.coarse_train", str(tmp_path / "in.ply"), "--cameras", str(tmp_path / "cameras.json"),
                          "--images", str(tmp_path / "images"), "--out", str(out), "--start-iteration", "8999", "--iterations", "9002",
                          "--samples", str(N_SAMPLES), "--seed", "1", "--regulariser", "density"], cwd=ROOT, capture_output=True, text=True,
                         timeout=300)
    print(run.stdout[-2000:], run.stderr[-2000:])
    assert run.returncode == 0
    assert (out / "9002.pt").is_file() and (out / "point_cloud.ply").is_file()
    state = torch.load(str(out / "9002.pt"), map_location="cpu")["state_dict"]
    g = sio.load_gaussian_ply(str(out / "point_cloud.ply"))
    assert 0 < state["_points"].shape[0] < P and g["xyz"].shape == state["_points"].shape       # the prune at 9001 ran
