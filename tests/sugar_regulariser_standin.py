"""TEST INFRASTRUCTURE: stand-in `SuGaR` classes for the GPU tests of the SDF regulariser bindings (the reference tree does not exist on
the GPU box).  `make_module()` returns a module-like namespace whose `SuGaR` is a fresh subclass of tests/sugar_standin.StandInSuGaR
with the properties and `get_normals` in its own dict -- what `sugar_patch.install_row_gathers` rebinds -- and, in place of the
reference's own `sample_points_in_gaussians` / `get_smallest_axis` / `get_points_depth_in_depth_map`, methods that fail loudly: on the
GPU the bindings of `sugar_patch.install_regulariser` must answer every call themselves.  (`get_field_values` underneath is the
binding of `sugar_patch.install`, as StandInSuGaR has it.)  The bindings are then installed on it exactly as on the real class."""
import types

from sugar_amd import sugar_patch
from tests.sugar_standin import StandInSuGaR


def _not_reached(name):
    def method(self, *args, **kwargs):
        raise AssertionError(f"{name}: the previous binding was reached with GPU tensors")
    method.__name__ = name
    return method


def _get_normals(self, estimate_from_points=False, neighborhood_size: int = 32):
    assert not estimate_from_points
    return self.get_smallest_axis()                                   # sugar_model.py:967 (a model that is not mesh-bound)


def make_module(patch_sugar=False, patch_gathers=False, regulariser_first=False):
    body = dict(points=StandInSuGaR.points, scaling=StandInSuGaR.scaling, quaternions=StandInSuGaR.quaternions,
                get_normals=_get_normals, binded_to_surface_mesh=False)
    for name in sugar_patch.REGULARISER_PATCHED[:3]:
        body[name] = _not_reached(name)
    module = types.SimpleNamespace(SuGaR=type("SuGaR", (StandInSuGaR,), body))
    if regulariser_first:
        sugar_patch.install_regulariser(module)
    if patch_sugar:
        sugar_patch.install(module)
    if patch_gathers:
        sugar_patch.install_row_gathers(module)
    if not regulariser_first:
        sugar_patch.install_regulariser(module)
    return module
