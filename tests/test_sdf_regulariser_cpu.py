"""CPU tests of the SDF regulariser bindings (sugar_amd.sugar_patch.install_regulariser, csrc/sdf_regulariser.hip underneath):
  * the committed fixture tests/golden/sdf_regulariser.npz: every `yard_*` -- the distance between the reference method's float32
    result and the float64 restatement of tests/sdf_regulariser_restatement.py -- is within the project's bars for these quantities
    (2e-5 for values, 1e-4 for gradients: tests/test_gpu_sugar_field.py), and the conditions the GPU tests rely on hold;
  * the host logic of install_regulariser / uninstall_regulariser / shims.install(patch_regulariser=...) / launch --patch-regulariser
    on a fake class: exactly the four names are bound, signatures are kept, the originals come back, CPU tensors reach the original,
    in every order with the other bindings of sugar_patch;
  * where the reference tree exists, the maker reproduces the committed fixture."""
import inspect
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
FX = np.load(os.path.join(HERE, "golden", "sdf_regulariser.npz"))
FIELD_FX = np.load(os.path.join(HERE, "golden", "sugar_field.npz"))

from sugar_amd import shims, sugar_patch  # noqa: E402

FOUR = ("sample_points_in_gaussians", "get_smallest_axis", "get_points_depth_in_depth_map", "get_field_values")


def test_yardsticks_are_within_the_projects_bars():
    yards = [k for k in FX.files if k.startswith("yard_")]
    assert len(yards) == 10
    for k in yards:
        assert k[len("yard_"):] in FX.files, k
        bar = 1e-4 if "_grad_" in k else 2e-5
        print(f"{k:32s} {float(FX[k]):.3e}  (bar {bar:g})")
        assert 0.0 <= float(FX[k]) < bar, (k, float(FX[k]))


def test_the_makers_conditions_hold():
    from make_sdf_regulariser import conditions
    conditions(FX, FIELD_FX)
    assert FX["depth_map"].shape == (int(FIELD_FX["H"]), int(FIELD_FX["W"]))
    assert np.array_equal(FX["sample_out"], FIELD_FX["field_x"]) and np.array_equal(FX["sample_idx"], FIELD_FX["field_gaussian_idx"])
    assert FX["sample_mask"][FX["sample_idx"]].all()
    assert np.array_equal(FX["normals_out"], FX["axis_out"])


# ---------------------------------------------------------------------------------------------------------------- a fake class
def _fake_module():
    """a module with a `SuGaR` class that has the reference's signatures for every method sugar_patch binds; each method says who it is"""
    class SuGaR:
        beta_mode = "average"
        binded_to_surface_mesh = False
        image_height, image_width = 4, 6
        device = torch.device("cpu")

        def __init__(self):
            self._p, self._s, self._q = torch.zeros(5, 3), torch.ones(5, 3), torch.ones(5, 4)

        points = property(lambda self: self._p)
        scaling = property(lambda self: self._s)
        quaternions = property(lambda self: self._q)
        n_points = property(lambda self: 5)

        def sample_points_in_gaussians(self, num_samples, sampling_scale_factor=1., mask=None,
                                       probabilities_proportional_to_opacity=False, probabilities_proportional_to_volume=True,):
            """the reference's sampler"""
            return ("reference", "sample_points_in_gaussians", num_samples, sampling_scale_factor)

        def get_smallest_axis(self, return_idx=False):
            return ("reference", "get_smallest_axis", return_idx)

        def get_normals(self, estimate_from_points=False, neighborhood_size: int = 32):
            return self.get_smallest_axis()

        def get_points_depth_in_depth_map(self, fov_camera, depth, points_in_camera_space):
            return ("reference", "get_points_depth_in_depth_map")

        def get_field_values(self, x, gaussian_idx=None, closest_gaussians_idx=None, gaussian_strengths=None, gaussian_centers=None,
                             gaussian_inv_scaled_rotation=None, return_sdf=True, density_threshold=1., density_factor=1.,
                             return_sdf_grad=False, sdf_grad_max_value=10., opacity_min_clamp=1e-16,
                             return_closest_gaussian_opacities=False, return_beta=False,):
            return ("reference", "get_field_values", return_sdf, return_beta)

        def get_points_rgb(self, positions=None, camera_centers=None, directions=None, sh_levels=None, sh_coordinates=None):
            return ("reference", "get_points_rgb")

        def get_covariance(self, return_full_matrix=False, return_sqrt=False, inverse_scales=False):
            return ("reference", "get_covariance")

        def compute_level_surface_points_from_camera_fast(self, nerf_cameras=None, cam_idx=0, rasterizer=None, **kw):
            return ("reference", "compute_level_surface_points_from_camera_fast")
    return types.SimpleNamespace(SuGaR=SuGaR)


def _calls(model):
    cam = types.SimpleNamespace(get_projection_transform=lambda: types.SimpleNamespace(get_matrix=lambda: torch.eye(4)[None]))
    return {"sample_points_in_gaussians": model.sample_points_in_gaussians(7, sampling_scale_factor=2.),
            "get_smallest_axis": model.get_smallest_axis(return_idx=True),
            "get_points_depth_in_depth_map": model.get_points_depth_in_depth_map(cam, torch.zeros(4, 6), torch.zeros(3, 3)),
            "get_field_values": model.get_field_values(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64), return_beta=True)}


def test_install_binds_exactly_the_four_methods_and_uninstall_restores_them():
    assert sugar_patch.REGULARISER_PATCHED == FOUR
    assert sugar_patch.PATCHED == ("get_points_rgb", "get_covariance", "get_field_values", "compute_level_surface_points_from_camera_fast")
    mod = _fake_module()
    cls = mod.SuGaR
    before = dict(cls.__dict__)
    signatures = {n: inspect.signature(getattr(cls, n)) for n in FOUR}
    assert sugar_patch.install_regulariser(mod) == list(FOUR)
    assert sugar_patch.install_regulariser(mod) == list(FOUR)          # idempotent
    changed = sorted(k for k in cls.__dict__ if cls.__dict__[k] is not before.get(k))
    assert changed == sorted(FOUR + ("_sugar_amd_regulariser_original",))
    for n in FOUR:
        assert inspect.signature(getattr(cls, n)) == signatures[n], n
        assert getattr(cls, n).__name__ == n
        assert cls._sugar_amd_regulariser_original[n] is before[n]       # the originals stay reachable
    assert cls.sample_points_in_gaussians.__doc__ == "the reference's sampler"
    # CPU tensors reach the original, arguments intact
    got = _calls(cls())
    assert got["sample_points_in_gaussians"] == ("reference", "sample_points_in_gaussians", 7, 2.)
    assert got["get_smallest_axis"] == ("reference", "get_smallest_axis", True)
    assert got["get_points_depth_in_depth_map"] == ("reference", "get_points_depth_in_depth_map")
    assert got["get_field_values"] == ("reference", "get_field_values", True, True)
    assert cls().get_normals() == ("reference", "get_smallest_axis", False)
    sugar_patch.uninstall_regulariser(mod)
    sugar_patch.uninstall_regulariser(mod)                               # idempotent
    assert dict(cls.__dict__) == before


@pytest.mark.parametrize("order", ["regulariser_first", "regulariser_last"])
def test_the_bindings_compose_with_the_others_in_any_order(order):
    mod = _fake_module()
    cls = mod.SuGaR
    before = dict(cls.__dict__)
    others = lambda: (sugar_patch.install(mod), sugar_patch.install_row_gathers(mod), sugar_patch.install_binding(mod))
    if order == "regulariser_first":
        sugar_patch.install_regulariser(mod)
        others()
    else:
        others()
        sugar_patch.install_regulariser(mod)
    assert sorted(cls._sugar_amd_regulariser_original) == sorted(FOUR) and sorted(cls._sugar_amd_original) == sorted(sugar_patch.PATCHED)
    got = _calls(cls())                                                  # CPU tensors: through both layers to the reference's method
    assert all(v[0] == "reference" and v[1] == k for k, v in got.items()), got
    if order == "regulariser_first":     # take ours out from underneath `install`'s binding, which stays
        sugar_patch.uninstall_regulariser(mod)
        assert "_sugar_amd_regulariser_original" not in cls.__dict__
        assert cls._sugar_amd_original["get_field_values"] is before["get_field_values"]
        assert cls().get_field_values(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64)) == ("reference", "get_field_values", True, False)
        assert cls.__dict__["sample_points_in_gaussians"] is before["sample_points_in_gaussians"]
    sugar_patch.uninstall(mod)                                           # everything off, in one call
    for n in FOUR + sugar_patch.PATCHED + ("points", "scaling", "quaternions", "get_normals"):
        assert cls.__dict__[n] is before[n], n
    assert "_sugar_amd_regulariser_original" not in cls.__dict__


def test_shims_install_takes_the_flag_and_leaves_the_default_alone():
    mod = _fake_module()
    before = dict(mod.SuGaR.__dict__)
    shims.install()
    assert dict(mod.SuGaR.__dict__) == before
    assert inspect.signature(shims.install).parameters["patch_regulariser"].default is False
    shims.install(patch_regulariser=mod)
    assert sorted(mod.SuGaR._sugar_amd_regulariser_original) == sorted(FOUR) and "_sugar_amd_original" not in mod.SuGaR.__dict__
    sugar_patch.uninstall_regulariser(mod)
    assert dict(mod.SuGaR.__dict__) == before


def test_launch_binds_the_regulariser_only_when_asked(tmp_path):
    """`python -m sugar_amd.launch --patch-regulariser script.py`: a fake `sugar_scene.sugar_model` next to the script stands in for
    the reference's"""
    pkg = tmp_path / "sugar_scene"
    pkg.mkdir()
    (pkg / "__init__.py").write_text("")
    (pkg / "sugar_model.py").write_text(
        "class SuGaR:\n"
        "    points = scaling = quaternions = property(lambda self: None)\n"
        "    def get_normals(self, estimate_from_points=False, neighborhood_size=32): pass\n"
        + "".join(f"    def {n}(self, *a, **k): pass\n" for n in FOUR + sugar_patch.PATCHED[:2] + sugar_patch.PATCHED[3:])
        + "def extract_texture_image_and_uv_from_gaussians(*a, **k): pass\n")
    script = tmp_path / "train.py"
    script.write_text(
        "import json, sugar_scene.sugar_model as sm\n"
        "print(json.dumps({'regulariser': sorted(sm.SuGaR.__dict__.get('_sugar_amd_regulariser_original', {})),\n"
        "                  'sugar': sorted(sm.SuGaR.__dict__.get('_sugar_amd_original', {}))}))\n")
    env = dict(os.environ, PYTHONPATH="")
    res = {}
    for flags in ((), ("--patch-regulariser",)):
        out = subprocess.run([sys.executable, "-m", "sugar_amd.launch", "--quiet", *flags, str(script)], cwd=ROOT, env=env,
                             capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        res[flags] = json.loads(out.stdout.strip().splitlines()[-1])
    assert res[()]["regulariser"] == [] and res[()]["sugar"] == sorted(sugar_patch.PATCHED)          # the defaults are unchanged
    assert res[("--patch-regulariser",)] == {"regulariser": sorted(FOUR), "sugar": sorted(sugar_patch.PATCHED)}


@pytest.mark.skipif(not os.path.isdir("/root/reference"), reason="the reference tree is only present in the build container")
def test_committed_fixture_is_what_the_reference_returns():
    import make_sdf_regulariser as maker
    out = maker.run()
    assert set(out) == set(FX.files)
    for k in FX.files:
        a, b = np.asarray(out[k]), FX[k]
        assert a.shape == b.shape and a.dtype == b.dtype, k
        assert np.array_equal(a, b), k         # same machine code, same seeds, CPU float32: the same bytes
