"""CPU tests of the yardstick of the point-surface route (tests/point_surface_restatement.py) and of the pieces of the route that need no
GPU: the float32 and float64 restatements agree on what is defined; after the spurious-face rule the sphere and the torus are closed
surfaces of the right genus wound outwards, the hemisphere is open with one boundary loop; the compaction, the outlier rule and the
command-line parser."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import mc_restatement as mcr  # noqa: E402
import point_surface_restatement as psr  # noqa: E402


@functools.lru_cache(maxsize=None)
def _mesh(name):
    """the restatement's pipeline on one case with exact neighbours: volumes in both precisions, the mesh before and after the drop"""
    c = psr.case(name)
    grid = psr.grid_points(*c["axes"])
    idx = psr.exact_knn(grid, c["points"], psr.K)
    shape = tuple(a.size for a in c["axes"])
    v32 = psr.implicit(grid, c["points"], c["normals"], idx, c["radius"], np.float32)[0].reshape(shape)
    v64 = psr.implicit(grid, c["points"], c["normals"], idx, c["radius"], np.float64)[0].reshape(shape)
    verts, faces, _ = mcr.marching_cubes(v32, 0.0)
    kept_v, kept_f = psr.drop_spurious(verts, faces, v32)
    return dict(case=c, v32=v32, v64=v64, verts=verts, faces=faces, kept_verts=kept_v, kept_faces=kept_f)


@pytest.mark.parametrize("name", ["A", "A'", "B", "C"])
def test_float32_and_float64_restatements_define_the_same_points(name):
    m = _mesh(name)
    assert np.array_equal(np.isnan(m["v32"]), np.isnan(m["v64"]))
    defined = np.isfinite(m["v32"])
    assert defined.any() and not defined.all()
    diff = np.abs(m["v32"][defined].astype(np.float64) - m["v64"][defined]).max()
    print(f"{name}: largest |float32 - float64| = {diff:.3g} ({diff / float(m['case']['radius']):.3g} of the radius)")
    assert diff < 1e-6 * float(m["case"]["radius"])      # float32: a few 2^-24 of values below the radius


@pytest.mark.parametrize("name", ["A", "A'", "B"])
def test_closed_shapes_are_closed_after_the_face_drop(name):
    m = _mesh(name)
    c = m["case"]
    v, f = m["kept_verts"], m["kept_faces"]
    assert 0 < f.shape[0] < m["faces"].shape[0]                                 # the walls at undefined points were there, and went
    closed, boundary, no_repeat = mcr.edge_report(f, v.shape[0])
    assert closed and no_repeat and boundary.shape[0] == 0
    assert mcr.euler_characteristic(f, v.shape[0]) == c["chi"]
    world = psr.grid_to_world(v, *c["axes"])
    volume, _ = mcr.signed_volume_and_area(world, f)
    assert volume > 0                                                           # wound outwards
    assert not psr.spurious_vertices(v, m["v32"]).any()
    assert c["distance"](world).max() < 0.25 * c["spacing"]                     # (a wall or a flipped sign is off by half a cell or more)


def test_hemisphere_stays_open():
    m = _mesh("C")
    v, f = m["kept_verts"], m["kept_faces"]
    closed, boundary, no_repeat = mcr.edge_report(f, v.shape[0])
    assert not closed and no_repeat and boundary.shape[0] > 0
    assert mcr.euler_characteristic(f, v.shape[0]) == 1                         # a disc: one boundary loop
    assert not psr.spurious_vertices(v, m["v32"])[f].any()
    assert np.array_equal(np.unique(f.reshape(-1)), np.arange(v.shape[0]))      # no unreferenced vertex is left


def test_spurious_rule_is_exact_on_the_restatement():
    """a vertex is spurious iff the edge it lies on has a non-finite end: checked through marching cubes' own edge records"""
    m = _mesh("C")
    _, _, aux = mcr.marching_cubes(m["v32"], 0.0)
    flat = m["v32"].reshape(-1)
    strides = (m["v32"].shape[1] * m["v32"].shape[2], m["v32"].shape[2], 1)
    other = aux["owner"] + np.array(strides)[aux["axis"]]
    expect = ~(np.isfinite(flat[aux["owner"]]) & np.isfinite(flat[other]))
    assert np.array_equal(psr.spurious_vertices(m["verts"], m["v32"]), expect)
    assert (aux["t"][expect] == 0.5).all()


def test_remove_vertices_by_mask_semantics():
    """five vertices, three faces; vertex 1 goes: faces 0 and 1 go with it, vertex 0 loses its last face"""
    verts = np.arange(15, dtype=np.float32).reshape(5, 3)
    faces = np.array([[0, 1, 2], [1, 3, 2], [2, 3, 4]])
    attr = np.array([10, 11, 12, 13, 14])
    mask = np.array([False, True, False, False, False])
    v, f, a = psr.remove_vertices_by_mask(verts, faces, mask, attr)
    assert np.array_equal(v, verts[[0, 2, 3, 4]]) and np.array_equal(f, [[1, 2, 3]]) and np.array_equal(a, [10, 12, 13, 14])
    v, f, a = psr.remove_vertices_by_mask(verts, faces, mask, attr, unreferenced=True)
    assert np.array_equal(v, verts[[2, 3, 4]]) and np.array_equal(f, [[0, 1, 2]]) and np.array_equal(a, [12, 13, 14])
    v, f = psr.remove_vertices_by_mask(verts, faces, np.zeros(5, bool))
    assert np.array_equal(v, verts) and np.array_equal(f, faces)
    v, f = psr.remove_vertices_by_mask(verts, faces, np.array([False, False, True, False, False]), unreferenced=True)
    assert v.shape == (0, 3) and f.shape == (0, 3)


def test_remove_vertices_by_mask_refuses_cpu_tensors():
    from sugar_amd.decimate import remove_vertices_by_mask
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        remove_vertices_by_mask(torch.zeros(5, 3), torch.zeros(3, 3, dtype=torch.int64), torch.zeros(5, dtype=torch.bool))


def test_outlier_rule_on_a_cloud_with_one_far_point():
    from sugar_amd.point_surface import outlier_rule, statistical_outlier_mask
    g = np.random.default_rng(3)
    cloud = np.concatenate([g.uniform(-1, 1, (400, 3)), [[300.0, 0.0, 0.0]]])
    d = np.sqrt(((cloud[:, None, :] - cloud[None, :, :]) ** 2).sum(axis=2))
    mean20 = np.sort(d, axis=1)[:, :20].mean(axis=1)                            # self included: the first of the 20 is 0
    keep = psr.outlier_keep(mean20, 5.0)
    assert keep[:400].all() and not keep[400]
    assert psr.outlier_keep(mean20, 20.0).sum() >= 400                          # the reference's ratio: a far weaker filter
    assert np.array_equal(outlier_rule(torch.from_numpy(mean20), 5.0).numpy(), keep)
    assert psr.outlier_keep(np.array([1.0]), 20.0).all() and bool(outlier_rule(torch.tensor([1.0]), 20.0).all())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        statistical_outlier_mask(torch.from_numpy(cloud).float())


def test_module_refuses_cpu_tensors():
    from sugar_amd import point_surface as ps
    pts, nrm = (torch.from_numpy(a) for a in psr.fibonacci_sphere(100, 0.6))
    X = torch.linspace(-1, 1, 9)
    for fn in (lambda: ps.implicit_at(pts, pts, nrm, 0.1), lambda: ps.implicit_grid(X, X, X, pts, nrm, 0.1),
               lambda: ps.mesh_from_oriented_points(pts, nrm, X, X, X)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn()


def test_command_line_parser():
    from sugar_amd import extract
    a = extract._parser().parse_args(["model.ply", "--out", "mesh.ply"])
    assert a.route == "marching-cubes" and a.cameras is None and a.sweep == "dense" and a.level == 0.3 and a.resolution == 512
    a = extract._parser().parse_args(["model.ply", "--route", "levelset", "--cameras", "cameras.json", "--out", "mesh.ply", "--surface-level",
                                      "0.5", "--n-points", "1000", "--radius-cells", "2", "--weight-quantile", "0.1", "--resolution", "64",
                                      "--decimate", "500", "--no-clean", "--no-background"])
    assert (a.route, a.cameras, a.surface_level, a.n_points, a.radius_cells, a.weight_quantile) == ("levelset", "cameras.json", 0.5, 1000, 2.0, 0.1)
    assert a.resolution == 64 and a.decimate == 500 and a.no_clean and a.no_background
    with pytest.raises(SystemExit) as e:                                        # before anything is read: the PLY does not exist
        extract.main(["model.ply", "--route", "levelset", "--out", "mesh.ply"])
    assert e.value.code == 2
    with pytest.raises(SystemExit):
        extract._parser().parse_args(["model.ply", "--route", "poisson", "--out", "mesh.ply"])
