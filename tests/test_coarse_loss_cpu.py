"""CPU tests of the coarse trainers' inline loss terms (sugar_amd.coarse_loss over csrc/coarse_loss.hip):
  * the committed fixture tests/golden/coarse_loss.npz: the conditions the GPU tests rely on hold (re-asserted by the maker's own
    `conditions`), every `yard_*` is finite and below 1e-4, and the float32 restatement of tests/coarse_loss_restatement.py
    reproduces the recorded float32 arrays;
  * the argument validation of coarse_loss.py: CPU tensors raise (there is no CPU fallback), each unsupported option raises;
  * the new symbols are declared in include/sugar_raster.h, listed in _lib.SIGNATURES, and the translation unit is in build.SOURCES;
  * the scratch layouts (csrc/coarse_loss_layout.h): tests/host/coarse_loss_layout_main.cpp, a host program of its own, is compiled and
    run (the same file is what runs under -fsanitize=address,undefined, see its header);
  * where the reference tree exists, the maker reproduces the committed fixture."""
import os
import re
import shutil
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
FX = np.load(os.path.join(HERE, "golden", "coarse_loss.npz"))
FIELD_FX = np.load(os.path.join(HERE, "golden", "sugar_field.npz"))
REG_FX = np.load(os.path.join(HERE, "golden", "sdf_regulariser.npz"))

from sugar_amd import coarse_loss  # noqa: E402
from tests import coarse_loss_restatement as cl  # noqa: E402
from tests import sdf_regulariser_restatement as rs  # noqa: E402

SYMBOLS = ("sgr_surface_band", "sgr_estimation_loss_scratch_bytes", "sgr_estimation_loss_forward", "sgr_estimation_loss_backward",
           "sgr_better_normal_forward_scratch_bytes", "sgr_better_normal_forward", "sgr_better_normal_backward_scratch_bytes",
           "sgr_better_normal_backward")


def _t(k, fx=FX):
    return torch.as_tensor(fx[k])


def test_the_makers_conditions_hold():
    from make_coarse_loss import conditions
    conditions(FX, FIELD_FX, REG_FX)
    assert FX["samples"].shape == (6000, 3) and FX["field_opacities"].shape == (6000, 16) and FX["est_band"].shape == (1000, 3)
    assert REG_FX["depth_map"].shape == (int(FIELD_FX["H"]), int(FIELD_FX["W"])) == (88, 120)
    assert FX["sample_mask"][FX["sample_idx"]].all()
    assert all(int(FX[k]) == 6000 for k in FX.files if k.endswith("_M"))


def test_yardsticks_are_finite_and_small():
    yards = [k for k in FX.files if k.startswith("yard_")]
    assert len(yards) == 28
    for k in yards:
        assert k[len("yard_"):] in FX.files, k
        print(f"{k:36s} {float(FX[k]):.3e}")
        assert np.isfinite(FX[k]) and 0.0 <= float(FX[k]) < 1e-4, (k, float(FX[k]))


def test_float32_restatement_reproduces_the_fixture():
    """the restatement with its own lookup (tests/sdf_regulariser_restatement.depth_lookup) in place of the reference's method: the
    recorded float32 results within their own yard of float64 (a float32 evaluation of the same formulas), M and the mask exactly"""
    from make_coarse_loss import EST_VARIANTS, SURFACE_WEIGHT, estimation_inputs
    V, Pm, dmap = _t("cam_world_to_view"), _t("depth_projection", REG_FX), _t("depth_map", REG_FX)
    pts, sc = _t("state_points", FIELD_FX), torch.exp(_t("state_scales", FIELD_FX))
    q = torch.nn.functional.normalize(_t("state_quaternions", FIELD_FX), dim=-1)
    extent = float(FX["extent"])

    def same(name, got):
        d = cl.scalar_distance(got, FX[name]) if got.dim() == 0 else rs.distance(got, FX[name])
        bar = max(4.0 * float(FX["yard_" + name]), 1e-6)
        print(f"{name:36s} distance {d:.3e}  bar {bar:.3e}")
        assert d <= bar, (name, d, bar)

    close, std, diff = cl.surface_band(pts, q, sc, V, _t("cam_center"), Pm, dmap, float(FX["band_threshold"]))
    assert torch.equal(close, _t("band_close"))
    same("band_std", std); same("band_diff", diff)
    x, idx, sdf, density, beta = estimation_inputs(FX)
    for tag, opts in EST_VARIANTS.items():
        opts = dict(opts)
        by_std = opts.pop("by_std", False)
        image = dmap[..., None].repeat(1, 1, 3).contiguous().requires_grad_(True)
        leaves = [t.clone().requires_grad_(True) for t in (x, sdf, density, beta)]
        est, surf, M = cl.estimation_losses(leaves[0], image[..., 0], V, Pm, _t("znear"), sdf=leaves[1], density=leaves[2], beta=leaves[3],
                                            scale=None if by_std else extent / 10., std=_t("band_std") if by_std else None, sample_idx=idx,
                                            clamp_max=10. * extent, **opts)
        (est + SURFACE_WEIGHT * surf if surf is not None else est).backward()
        assert int(M) == int(FX[tag + "_M"])
        same(tag + "_loss_est", est.detach())
        if surf is not None:
            same(tag + "_loss_surf", surf.detach())
        same(tag + "_grad_samples", leaves[0].grad); same(tag + "_grad_depth", image.grad[..., 0])
        same(tag + "_grad_field", (leaves[1] if opts["mode"] == "sdf" else leaves[2]).grad)
        if opts["mode"] == "density":
            same(tag + "_grad_beta", leaves[3].grad)
    normals, knn = _t("normals_out", REG_FX), _t("state_knn_idx", FIELD_FX)
    for tag, only in (("normal_only", True), ("normal_full", False)):
        leaves = [t.clone().requires_grad_(True) for t in (_t("samples"), normals, pts)]
        loss = cl.better_normal_loss(leaves[0], idx[:6000], knn, leaves[1], leaves[2], sc.min(dim=-1)[0], _t("field_opacities"), only)
        loss.backward()
        same(tag + "_loss", loss.detach()); same(tag + "_grad_normals", leaves[1].grad)
        if only:
            assert leaves[0].grad is None and leaves[2].grad is None
        else:
            same(tag + "_grad_points", leaves[2].grad); same(tag + "_grad_samples", leaves[0].grad)


# ------------------------------------------------------------------------------------------------------------ argument validation
def test_cpu_tensors_raise():
    P, N, K = 5, 7, 16
    eye = torch.eye(4)[None]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        coarse_loss.surface_band(torch.zeros(P, 3), torch.ones(P, 4), torch.ones(P, 3), eye, torch.zeros(1, 3), eye, torch.ones(4, 6))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        coarse_loss.estimation_losses(torch.zeros(N, 3), torch.ones(4, 6), eye, eye, 0.1, sdf=torch.zeros(N), scale=1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        coarse_loss.better_normal_loss(torch.zeros(N, 3), torch.zeros(N, dtype=torch.int64), torch.zeros(P, K, dtype=torch.int64),
                                       torch.ones(P, 3), torch.zeros(P, 3), torch.ones(P), torch.ones(N, K))


def test_estimation_losses_checks_its_options():
    x, d, eye = torch.zeros(3, 3), torch.ones(4, 6), torch.eye(4)
    with pytest.raises(ValueError, match="Unknown sdf_estimation_mode"):
        coarse_loss.estimation_losses(x, d, eye, eye, 0.1, mode="tsdf", sdf=torch.zeros(3), scale=1.0)
    with pytest.raises(ValueError, match="neither term"):
        coarse_loss.estimation_losses(x, d, eye, eye, 0.1, sdf=torch.zeros(3), scale=1.0, with_estimation=False)
    with pytest.raises(ValueError, match="needs density= and beta="):
        coarse_loss.estimation_losses(x, d, eye, eye, 0.1, mode="density", density=torch.zeros(3), scale=1.0)
    with pytest.raises(ValueError, match="scale="):
        coarse_loss.estimation_losses(x, d, eye, eye, 0.1, sdf=torch.zeros(3))
    with pytest.raises(ValueError, match="needs sample_idx="):
        coarse_loss.estimation_losses(x, d, eye, eye, 0.1, sdf=torch.zeros(3), std=torch.ones(5))


@pytest.mark.parametrize("option,value,error", [
    ("use_projection_as_estimation", True, NotImplementedError),
    ("sample_only_in_gaussians_close_to_surface", False, NotImplementedError),
    ("sdf_estimation_mode", "tsdf", ValueError),
])
def test_each_unsupported_option_raises(option, value, error):
    sugar = types.SimpleNamespace(beta_mode="average")
    with pytest.raises(error, match=option if error is NotImplementedError else "Unknown sdf_estimation_mode"):
        coarse_loss.regulariser_terms(sugar, None, None, None, **{option: value})


@pytest.mark.parametrize("beta_mode", ["learnable", "weighted_average"])
def test_the_other_beta_modes_raise(beta_mode):
    with pytest.raises(NotImplementedError, match="beta_mode"):
        coarse_loss.regulariser_terms(types.SimpleNamespace(beta_mode=beta_mode), None, None, None)


def test_the_composite_has_the_trainers_defaults():
    import inspect
    d = {k: p.default for k, p in inspect.signature(coarse_loss.regulariser_terms).parameters.items()}
    assert (d["sdf_estimation_mode"], d["use_sdf_estimation_loss"], d["enforce_samples_to_be_on_surface"]) == ("sdf", True, False)   # coarse_sdf.py:121-124
    assert (d["squared_sdf_estimation_loss"], d["squared_samples_on_surface_loss"], d["normalize_by_sdf_std"]) == (False, False, False)  # :128-131
    assert (d["sample_only_in_gaussians_close_to_surface"], d["close_gaussian_threshold"]) == (True, 2.0)                           # :135-136
    assert (d["use_sdf_better_normal_loss"], d["sdf_better_normal_gradient_through_normal_only"]) == (True, True)                   # :140-144
    assert (d["density_factor"], d["density_threshold"]) == (1.0 / 16.0, 1.0)                                                       # :146-149
    assert (d["n_samples_for_sdf_regularization"], d["sdf_sampling_scale_factor"], d["sdf_sampling_proportional_to_volume"]) == (1_000_000, 1.5, False)


# --------------------------------------------------------------------------------------------------------------------- the ABI
def test_the_new_symbols_are_declared_listed_and_built():
    from sugar_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "sugar_raster.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\b(int|size_t)\s+" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES, name
    for flag, value in (("SGR_CL_SQUARED_EST", 1), ("SGR_CL_SQUARED_SURFACE", 2), ("SGR_CL_WITH_EST", 4), ("SGR_CL_WITH_SURFACE", 8)):
        assert re.search(rf"#define {flag} {value}\b", header), flag
    assert (coarse_loss._SQUARED_EST, coarse_loss._SQUARED_SURFACE, coarse_loss._WITH_EST, coarse_loss._WITH_SURFACE) == (1, 2, 4, 8)
    assert "coarse_loss.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "coarse_loss.hip"))
    assert "float atomics" in header[header.index("sgr_estimation_loss_*"):header.index("sgr_better_normal_*")]     # the depth gradient's caveat
    assert "#define SGR_ABI_VERSION 4 " in header                                                                    # additive: no bump


# ----------------------------------------------------------------------------------------------------------- the scratch layouts
def test_scratch_layouts_in_a_host_program(tmp_path):
    """csrc/coarse_loss_layout.h is plain host C++: a program of its own (tests/host/coarse_loss_layout_main.cpp) carves the layouts
    into heap blocks of exactly the reported sizes, writes every part end to end and checks alignment, order and the 2^32 entry limit.
    (Its header gives the command that runs the same file under AddressSanitizer and UBSan; nothing loaded into Python is sanitized.)"""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler"
    exe = tmp_path / "coarse_loss_layout"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "sugar_amd", "csrc"),
           os.path.join(HERE, "host", "coarse_loss_layout_main.cpp"), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert built.returncode == 0, built.stderr[-3000:]
    ran = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert ran.returncode == 0, (ran.stdout[-2000:], ran.stderr[-3000:])
    assert "layouts ok" in ran.stdout


@pytest.mark.skipif(not os.path.isdir("/root/reference"), reason="the reference tree is only present in the build container")
def test_committed_fixture_is_what_the_maker_writes():
    import make_coarse_loss as maker
    out = maker.run()
    assert set(out) == set(FX.files)
    for k in FX.files:
        a, b = np.asarray(out[k]), FX[k]
        assert a.shape == b.shape and a.dtype == b.dtype, k
        if k.startswith("yard_") and "_grad_" in k:
            assert abs(float(a) - float(b)) <= 0.5 * float(b), k
        elif "_grad_" in k:                    # torch's CPU scatter backwards add in thread order: equal up to the order of the adds
            assert (rs.distance(a, b) if a.ndim else cl.scalar_distance(a, b)) <= 1e-6, k
        else:
            assert np.array_equal(a, b), k     # same machine code, same seeds, CPU float32: the same bytes
