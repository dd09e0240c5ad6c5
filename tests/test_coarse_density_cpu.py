"""CPU tests of the native density regulariser (coarse_density.py's default, `use_projection_as_estimation=True`):
  * the committed fixture tests/golden/coarse_density.npz: the condition the GPU tests rely on holds when re-asserted by the maker's
    own `conditions` (no sample within 1e-4 of a kink), every `yard_*` is finite and small, and the float32 restatement of
    tests/coarse_density_restatement.py reproduces the recorded float32 values and gradients within their yards;
  * the argument validation and the CPU-tensor refusal of coarse_loss.projection_estimation_losses / density_regulariser_terms;
  * coarse_train.DENSITY_OVERRIDES are the four values in which coarse_density.py differs, the trainer applies them, explicit options
    win, and every other combination raises; `--regulariser` parses and its default leaves every other parsed value as it was;
  * the new symbols are declared in include/sugar_raster.h and listed in _lib.SIGNATURES; the ABI version is 4;
  * coarse_loss.regulariser_terms still refuses the two options."""
import inspect
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
FX = np.load(os.path.join(HERE, "golden", "coarse_density.npz"))
FIELD_FX = np.load(os.path.join(HERE, "golden", "sugar_field.npz"))

from sugar_amd import coarse_loss, coarse_train  # noqa: E402
from tests import coarse_density_restatement as cd  # noqa: E402
from tests import sdf_regulariser_restatement as rs  # noqa: E402

SYMBOLS = ("sgr_projection_loss_scratch_bytes", "sgr_projection_loss_forward", "sgr_projection_loss_backward_scratch_bytes",
           "sgr_projection_loss_backward")


def _t(k, fx=FX):
    return torch.as_tensor(fx[k])


# ------------------------------------------------------------------------------------------------------------------ the fixture
def test_the_makers_condition_holds():
    from make_coarse_density import MARGIN, conditions
    margins = conditions(FX, FIELD_FX)
    for name, m in margins.items():
        print(f"{name:32s} {m:.3e}")
        assert m >= MARGIN == 1e-4, name
    assert set(margins) == {"density == target", "est == 0", "sdf == |est|", "clamp of |sdf - |est|| / s", "clamp of |est| / s"}
    assert FX["samples"].shape == (6000, 3) and FX["sample_noise"].shape == (6000, 3) and FX["normals"].shape == (2500, 3)
    assert FX["sample_mask"][FX["sample_idx"]].all() and FX["sample_mask"].sum() >= 256
    assert os.path.getsize(os.path.join(HERE, "golden", "coarse_density.npz")) < 1 << 20


def test_yardsticks_are_finite_and_small():
    yards = [k for k in FX.files if k.startswith("yard_")]
    assert len(yards) == 6 + 6 + 6 + 6, yards                                   # den, den_sq, sdf_surf, model
    for k in yards:
        assert k[len("yard_"):] in FX.files, k
        print(f"{k:36s} {float(FX[k]):.3e}")
        assert np.isfinite(FX[k]) and 0.0 <= float(FX[k]) < 1e-4, (k, float(FX[k]))


def test_float32_restatement_reproduces_the_fixture():
    from make_coarse_density import SURFACE_WEIGHT, VARIANTS
    extent = float(FX["extent"])
    idx = _t("sample_idx").to(torch.int64)

    def same(name, got):
        d = cd.scalar_distance(got, FX[name]) if got.dim() == 0 else rs.distance(got, FX[name])
        bar = max(4.0 * float(FX["yard_" + name]), 1e-6)
        print(f"{name:36s} distance {d:.3e}  bar {bar:.3e}")
        assert d <= bar, (name, d, bar)

    for tag, opts in VARIANTS.items():
        leaves = [t.clone().requires_grad_(True) for t in (_t("samples"), _t("field_sdf"), _t("field_density"), _t("field_beta"),
                                                           _t("state_points", FIELD_FX), _t("normals"))]
        est, surf = cd.projection_estimation_losses(leaves[0], idx, leaves[4], leaves[5], sdf=leaves[1], density=leaves[2], beta=leaves[3],
                                                    scale=extent / 10., clamp_max=10. * extent, **opts)
        (est + SURFACE_WEIGHT * surf if surf is not None else est).backward()
        same(tag + "_loss_est", est.detach())
        if surf is not None:
            same(tag + "_loss_surf", surf.detach())
        same(tag + "_grad_samples", leaves[0].grad)
        same(tag + "_grad_field", (leaves[1] if opts["mode"] == "sdf" else leaves[2]).grad)
        if opts["mode"] == "density":
            same(tag + "_grad_beta", leaves[3].grad)
        else:
            assert leaves[3].grad is None
        same(tag + "_grad_points", leaves[4].grad); same(tag + "_grad_normals", leaves[5].grad)
        counts = np.bincount(FX["sample_idx"], minlength=2500)
        assert not leaves[4].grad[counts == 0].any() and not leaves[5].grad[counts == 0].any()


# ------------------------------------------------------------------------------------------------------------ argument validation
def test_cpu_tensors_raise():
    P, N = 5, 7
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        coarse_loss.projection_estimation_losses(torch.zeros(N, 3), torch.zeros(N, dtype=torch.int64), torch.zeros(P, 3), torch.ones(P, 3),
                                                 density=torch.zeros(N), beta=torch.ones(N))
    sugar = types.SimpleNamespace(beta_mode="average", points=torch.zeros(P, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        coarse_loss.density_regulariser_terms(sugar, torch.ones(P, dtype=torch.bool))


def test_projection_estimation_losses_checks_its_options():
    x, i, p, n = torch.zeros(3, 3), torch.zeros(3, dtype=torch.int64), torch.zeros(5, 3), torch.ones(5, 3)
    f = coarse_loss.projection_estimation_losses
    with pytest.raises(ValueError, match="Unknown sdf_estimation_mode"):
        f(x, i, p, n, mode="tsdf", sdf=torch.zeros(3), scale=1.0)
    with pytest.raises(ValueError, match="neither term"):
        f(x, i, p, n, density=torch.zeros(3), beta=torch.ones(3), with_estimation=False)
    with pytest.raises(ValueError, match="needs density= and beta="):
        f(x, i, p, n, density=torch.zeros(3))
    with pytest.raises(ValueError, match="needs sdf="):
        f(x, i, p, n, mode="sdf", scale=1.0)
    with pytest.raises(ValueError, match="scale="):
        f(x, i, p, n, mode="sdf", sdf=torch.zeros(3))
    with pytest.raises(ValueError, match="scale="):
        f(x, i, p, n, density=torch.zeros(3), beta=torch.ones(3), with_surface=True)
    d = {k: q.default for k, q in inspect.signature(f).parameters.items()}
    assert (d["mode"], d["clamp_max"], d["with_estimation"], d["with_surface"], d["squared_estimation"], d["squared_surface"]) == (
        "density", float("inf"), True, False, False, False)


def test_density_regulariser_terms_checks_its_options_and_has_the_trainers_defaults():
    sugar = types.SimpleNamespace(beta_mode="average")
    with pytest.raises(ValueError, match="Unknown sdf_estimation_mode"):
        coarse_loss.density_regulariser_terms(sugar, None, sdf_estimation_mode="tsdf")
    with pytest.raises(ValueError, match="no term"):
        coarse_loss.density_regulariser_terms(sugar, None, use_sdf_estimation_loss=False, use_sdf_better_normal_loss=False)
    for beta_mode in ("learnable", "weighted_average"):
        with pytest.raises(NotImplementedError, match="beta_mode"):
            coarse_loss.density_regulariser_terms(types.SimpleNamespace(beta_mode=beta_mode), None)
    params = inspect.signature(coarse_loss.density_regulariser_terms).parameters
    assert list(params)[:2] == ["sugar", "visibility_filter"] and "fov_camera" not in params and "depth" not in params
    d = {k: p.default for k, p in params.items()}
    assert (d["sdf_estimation_mode"], d["density_factor"], d["density_threshold"]) == ("density", 1.0, 1.0)        # coarse_density.py:124, :156, :155
    assert (d["n_samples_for_sdf_regularization"], d["sdf_sampling_scale_factor"], d["sdf_sampling_proportional_to_volume"]) == (1_000_000, 1.5, False)
    assert (d["use_sdf_estimation_loss"], d["enforce_samples_to_be_on_surface"], d["use_sdf_better_normal_loss"]) == (True, False, True)
    assert (d["squared_sdf_estimation_loss"], d["squared_samples_on_surface_loss"], d["sdf_better_normal_gradient_through_normal_only"]) == (
        False, False, True)


@pytest.mark.parametrize("option,value", [("use_projection_as_estimation", True), ("sample_only_in_gaussians_close_to_surface", False)])
def test_regulariser_terms_still_refuses_the_two_options(option, value):
    with pytest.raises(NotImplementedError, match=option):
        coarse_loss.regulariser_terms(types.SimpleNamespace(beta_mode="average"), None, None, None, **{option: value})


# ----------------------------------------------------------------------------------------------------- the trainer and the command
def test_density_overrides_are_the_references_four_values():
    assert coarse_train.DENSITY_OVERRIDES == dict(sdf_estimation_mode="density", use_projection_as_estimation=True,
                                                  sample_only_in_gaussians_close_to_surface=False, density_factor=1.0)
    d = coarse_train.DEFAULTS
    assert (d["regulariser"], d["use_projection_as_estimation"]) == ("sdf", False)
    assert (d["sdf_estimation_mode"], d["sample_only_in_gaussians_close_to_surface"], d["density_factor"]) == ("sdf", True, 1.0 / 16.0)
    ref = "/root/reference/sugar_trainers/coarse_density.py"
    if os.path.exists(ref):                                                     # the reference's own assignments, where the tree exists
        src = open(ref).read()
        assert re.search(r"^\s*sdf_estimation_mode = 'density'", src, re.M) and re.search(r"^\s*density_factor = 1\.\s", src, re.M)
        assert re.search(r"^\s*use_projection_as_estimation = True", src, re.M)
        assert re.search(r"if use_projection_as_estimation:\s*\n\s*sample_only_in_gaussians_close_to_surface = False", src)
    for it in (7001, 8999, 9000, 9001, 9500):                                   # the two schedules are the same
        assert coarse_train.phase(it, **coarse_train.DENSITY_OVERRIDES, regulariser="density") == coarse_train.phase(it)


def _options_of(**options):
    """the options CoarseTrainer resolves, read off the exception-free part of its constructor through a stub model"""
    seen = {}

    class Stop(Exception):
        pass

    class Points:
        is_cuda = True

    class Model:
        _points = Points()
        cameras = None

        def set_cameras(self, cameras):
            raise Stop

    t = coarse_train.CoarseTrainer.__new__(coarse_train.CoarseTrainer)
    try:
        t.__init__(Model(), [], [], **options)
    except Stop:
        seen.update(t.options)
    return seen


def test_the_trainer_applies_the_overrides_and_explicit_options_win():
    assert _options_of() == coarse_train.DEFAULTS
    o = _options_of(regulariser="density")
    assert o == dict(coarse_train.DEFAULTS, regulariser="density", **coarse_train.DENSITY_OVERRIDES)
    o = _options_of(regulariser="density", density_factor=0.5, sdf_estimation_mode="sdf", enforce_samples_to_be_on_surface=True)
    assert (o["density_factor"], o["sdf_estimation_mode"], o["enforce_samples_to_be_on_surface"]) == (0.5, "sdf", True)
    assert o["use_projection_as_estimation"] is True and o["sample_only_in_gaussians_close_to_surface"] is False


@pytest.mark.parametrize("options,match", [
    (dict(regulariser="density", use_projection_as_estimation=False), "use_projection_as_estimation"),
    (dict(regulariser="density", sample_only_in_gaussians_close_to_surface=True), "sample_only_in_gaussians_close_to_surface"),
    (dict(regulariser="density", normalize_by_sdf_std=True), "normalize_by_sdf_std"),
    (dict(regulariser="density", backpropagate_gradients_through_depth=False), "backpropagate_gradients_through_depth"),
    (dict(use_projection_as_estimation=True), "use_projection_as_estimation"),
    (dict(regulariser="sdf", use_projection_as_estimation=True, backpropagate_gradients_through_depth=False), "backpropagate_gradients_through_depth"),
])
def test_every_other_combination_raises_naming_the_option(options, match):
    with pytest.raises(NotImplementedError, match=match):
        _options_of(**options)


def test_an_unknown_regulariser_raises():
    with pytest.raises(ValueError, match="regulariser"):
        _options_of(regulariser="tsdf")


def test_the_command_switch_parses_and_its_default_changes_nothing_else():
    ap = coarse_train._parser()
    base = ["pc.ply", "--cameras", "c.json", "--images", "im", "--out", "o"]
    a, b = ap.parse_args(base), ap.parse_args(base + ["--regulariser", "density"])
    assert a.regulariser == "sdf" and b.regulariser == "density"
    assert {k: v for k, v in vars(a).items() if k != "regulariser"} == {k: v for k, v in vars(b).items() if k != "regulariser"}
    assert vars(a) == dict(point_cloud="pc.ply", cameras="c.json", images="im", out="o", iterations=15000, start_iteration=7000,
                           estimation_factor=0.2, normal_factor=0.2, samples=1_000_000, seed=0, device="cuda:0", regulariser="sdf")
    with pytest.raises(SystemExit):
        ap.parse_args(base + ["--regulariser", "tsdf"])


# --------------------------------------------------------------------------------------------------------------------- the ABI
def test_the_new_symbols_are_declared_and_listed():
    from sugar_amd import _lib
    header = open(os.path.join(ROOT, "include", "sugar_raster.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\b(int|size_t)\s+" + name + r"\s*\(", code), name
        assert name in _lib.SIGNATURES, name
    fwd, bwd = _lib.SIGNATURES["sgr_projection_loss_forward"][1], _lib.SIGNATURES["sgr_projection_loss_backward"][1]
    assert len(fwd) == 16 and len(bwd) == 21                                    # (the stream last)
    assert re.search(r"#define\s+SGR_ABI_VERSION\s+4\b", header) and "#define SGR_ABI_VERSION 4 " in header
    source = open(os.path.join(ROOT, "sugar_amd", "csrc", "coarse_loss.hip")).read()
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", source), name
    for word in ("printf", "assert(", "atomicAdd"):
        assert word not in source[source.index("struct ProjArgs"):source.index("bool proj_args_ok")], word
