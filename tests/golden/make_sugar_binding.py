#!/usr/bin/env python
"""Golden fixture for the refine stage's mesh binding, written by the reference's OWN class on the CPU: the properties

  SuGaR.points / SuGaR.scaling / SuGaR.quaternions        sugar_scene/sugar_model.py:383-479

of a SuGaR model bound to a surface mesh (the construction of make_sugar_callsite.py `run_bound`, with its `_bumpy_sphere` at 144 triangles and its
test-only substitutions), for n = 1, 3, 4 and 6 Gaussians per triangle, in a
mid-refinement state (`_points`, `_scales`, `_quaternions` perturbed with a seeded generator).  `Meshes`, `matrix_to_quaternion` are the
stand-ins of sugar_amd.shims.

Per n (prefix `n{n}_`):
  inputs            _points, faces, bary (surface_triangle_bary_coords, [n,3]), _scales, _quaternions, thickness
  out_<prop>        the three properties as the reference returns them (float32)
  cot_<prop>        a seeded cotangent for each
  grad_<prop>_<param>   what autograd puts on _points / _scales / _quaternions for sum(property * cotangent), one backward per property
  grad_all_<param>      ... and for the sum of the three
  ..._f64           the same quantities with the model's tensors cast to double (same input values)
  nc_value_f64, nc_grad_f64   the stand-in `pytorch3d.loss.mesh_normal_consistency(model.surface_mesh)` and its vertex gradient in
                    float64.  PARITY-UNPINNED against pytorch3d, which is not installed: the stand-in is this project's definition.

Asserted here so that the arg-max of matrix_to_quaternion (and with it the quaternion's sign) cannot flip between float32 and float64:
for EVERY Gaussian the largest and second-largest of the four q_abs values differ by more than 1e-3, and every face has an area above
1e-6.  The tests exclude no element.

The GPU test (tests/test_gpu_mesh_bind.py) replays this file through the HIP kernels; it never imports the reference.

    python tests/golden/make_sugar_binding.py      -> tests/golden/sugar_binding.npz
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import make_sugar_callsite as mk  # noqa: E402

W, H = 200, 152
N_LAT, N_LON = 7, 12          # 144 triangles, 86 vertices: keeps the file near half a megabyte
CASES = ((1, 101), (3, 103), (4, 104), (6, 126))     # (Gaussians per triangle, seed: the first that meets the conditions below)
PROPS = ("points", "scaling", "quaternions")
PARAMS = ("_points", "_scales", "_quaternions")
DEPENDS = {"points": ("_points",), "scaling": ("_scales",), "quaternions": ("_points", "_quaternions"), "all": PARAMS}


def build_model(sm, n_per_triangle, seed):
    from sugar_amd import synthetic as syn
    cams = syn.orbit_cameras(W, H)
    nerf = types.SimpleNamespace(device=torch.device("cpu"), training_cameras=mk._Cameras(cams))
    mesh = mk._bumpy_sphere(n_lat=N_LAT, n_lon=N_LON)
    g = torch.Generator().manual_seed(seed)
    model = sm.SuGaR(nerfmodel=nerf, points=None, colors=None, initialize=False, sh_levels=4, keep_track_of_knn=False,
                     surface_mesh_to_bind=mesh, n_gaussians_per_surface_triangle=n_per_triangle, learn_surface_mesh_positions=True,
                     learn_surface_mesh_opacity=True, learn_surface_mesh_scales=True)
    P = model._n_points
    assert model.binded_to_surface_mesh and not model.editable and P == n_per_triangle * len(mesh.triangles)
    with torch.no_grad():   # a mid-refinement state
        model._points += 0.01 * torch.randn(model._points.shape, generator=g)
        model._scales += 0.3 * torch.randn(P, 2, generator=g) + 0.5
        model._quaternions += 0.7 * torch.randn(P, 2, generator=g)
    cots = {"points": torch.randn(P, 3, generator=g), "scaling": torch.randn(P, 3, generator=g),
            "quaternions": torch.randn(P, 4, generator=g)}
    return model, cots


def to_double(model):
    for name in PARAMS:
        setattr(model, name, torch.nn.Parameter(getattr(model, name).detach().double()))
    model.surface_triangle_bary_coords = model.surface_triangle_bary_coords.double()
    model.surface_mesh_thickness = torch.nn.Parameter(model.surface_mesh_thickness.detach().double(), requires_grad=False)


def evaluate(model, cots, suffix):
    """outputs and gradients of the three properties under `cots` (cast to the model's dtype)"""
    out = {}
    dtype = model._points.dtype
    for which in PROPS + ("all",):
        for p in PARAMS:
            getattr(model, p).grad = None
        props = PROPS if which == "all" else (which,)
        loss = 0.0
        for prop in props:
            val = getattr(model, prop)
            if which != "all":
                out[f"out_{prop}{suffix}"] = val.detach().numpy().copy()
            loss = loss + (val * cots[prop].to(dtype)).sum()
        loss.backward()
        for p in DEPENDS[which]:
            out[f"grad_{which}{p}{suffix}"] = getattr(model, p).grad.detach().numpy().copy()
    return out


def check_conditions(model):
    """on the float64 model: the arg-max margin of matrix_to_quaternion and the face areas"""
    from pytorch3d.transforms import quaternion_to_matrix
    with torch.no_grad():
        m = quaternion_to_matrix(model.quaternions)
        d = torch.diagonal(m, dim1=-2, dim2=-1)
        t = torch.stack([1 + d[:, 0] + d[:, 1] + d[:, 2], 1 + d[:, 0] - d[:, 1] - d[:, 2], 1 - d[:, 0] + d[:, 1] - d[:, 2],
                         1 - d[:, 0] - d[:, 1] + d[:, 2]], dim=-1)
        q_abs = t.clamp_min(0).sqrt().sort(dim=-1, descending=True).values
        margin = float((q_abs[:, 0] - q_abs[:, 1]).min())
        tri = model._points[model._surface_mesh_faces]
        area = 0.5 * torch.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], dim=-1).norm(dim=-1)
    assert margin > 1e-3, f"arg-max margin {margin}: choose another seed"
    assert float(area.min()) > 1e-6, f"smallest face area {float(area.min())}"
    return margin, float(area.min())


def run_case(sm, n, seed):
    from pytorch3d.loss import mesh_normal_consistency
    model, cots = build_model(sm, n, seed)
    out = {"_points": model._points.detach().numpy().copy(), "faces": model._surface_mesh_faces.detach().numpy().astype(np.int64),
           "bary": model.surface_triangle_bary_coords[..., 0].numpy().copy(), "_scales": model._scales.detach().numpy().copy(),
           "_quaternions": model._quaternions.detach().numpy().copy(),
           "thickness": model.surface_mesh_thickness.detach().numpy().astype(np.float32).reshape(1)}
    for k, v in cots.items():
        out["cot_" + k] = v.numpy().copy()
    out.update(evaluate(model, cots, ""))
    to_double(model)
    out.update(evaluate(model, cots, "_f64"))
    check_conditions(model)
    model._points.grad = None
    loss = mesh_normal_consistency(model.surface_mesh)
    loss.backward()
    out["nc_value_f64"] = loss.detach().numpy().reshape(1).copy()
    out["nc_grad_f64"] = model._points.grad.detach().numpy().copy()
    return out


def run():
    """returns {name: np.ndarray}"""
    sm = mk._import_reference_model()
    assert not getattr(sm, "use_old_method", False)
    real_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    sm.knn_points = mk._scipy_knn_points
    try:
        out = {}
        for n, seed in CASES:
            for k, v in run_case(sm, n, seed).items():
                out[f"n{n}_{k}"] = v
        return out
    finally:
        torch.Tensor.cuda = real_cuda


def main():
    out = run()
    path = os.path.join(HERE, "sugar_binding.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", len(out), "arrays")


if __name__ == "__main__":
    sys.exit(main())
