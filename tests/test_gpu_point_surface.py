"""GPU tests of the point-surface route (csrc/point_surface.hip, sugar_amd.point_surface, sugar_amd.extract.extract_mesh_level_sets)
against the numpy restatement tests/point_surface_restatement.py:

  1. the volume: the NaN pattern equals the float32 restatement's exactly, the defined values lie within 4 x the largest
     |float32 restatement - float64 restatement| of the float64 restatement (the yardstick sets the bar, on the device's own neighbour
     lists), and `implicit_at` gives the same bits as `implicit_grid`;
  2. the brick sandwich: (bricks holding a defined point) <= flags <= (the box rule in float64 at radius (1 + 1e-5));
  3. the face drop, bit for bit against mc_restatement.marching_cubes + the numpy drop rule on the device's volume;
  4. topology and accuracy of the device mesh; 5. invariances and errors; 6. the quantile trim and the colours; 7. the route end to end.

Cases (the smallest with partial edge bricks, inactive bricks and both k-NN paths): A a 20 000-point sphere on 37^3 (grid k-NN), A' the
same with 3 000 points (exhaustive k-NN), B a torus on 37 x 37 x 19, C the upper hemisphere of A (an open surface)."""
import functools
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import mc_restatement as mcr  # noqa: E402
import point_surface_restatement as psr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = ["A", "A'", "B", "C"]
RUNS = [(n, 16) for n in CASES] + [("A", 8)]
RUN_IDS = [f"{n}-K{k}" for n, k in RUNS]


def _dev(*arrays):
    out = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]
    return out if len(out) > 1 else out[0]


@functools.lru_cache(maxsize=None)
def _case(name):
    c = psr.case(name)
    c["d_points"], c["d_normals"] = _dev(c["points"], c["normals"])
    c["d_axes"] = tuple(_dev(*c["axes"]))
    c["shape"] = tuple(a.size for a in c["axes"])
    return c


@functools.lru_cache(maxsize=None)
def _volume(name, K):
    """the device volume and brick mask, and both restatements on the DEVICE's neighbour lists; computed once, never written to"""
    from sugar_amd.knn import knn_points
    from sugar_amd.point_surface import implicit_grid
    c = _case(name)
    vol, mask = implicit_grid(*c["d_axes"], c["d_points"], c["d_normals"], float(c["radius"]), K=K, return_active=True)
    grid = psr.grid_points(*c["axes"])
    idx = knn_points(_dev(grid)[None], c["d_points"][None], K=K).idx[0].cpu().numpy()
    r32 = psr.implicit(grid, c["points"], c["normals"], idx, c["radius"], np.float32)
    r64 = psr.implicit(grid, c["points"], c["normals"], idx, c["radius"], np.float64)
    return dict(vol=vol, mask=mask, grid=grid, r32=r32, r64=r64)


@functools.lru_cache(maxsize=None)
def _mesh(name, K=16):
    """the device mesh in index coordinates and in world coordinates, and the restatement's mesh from the device volume"""
    from sugar_amd import point_surface as ps
    c = _case(name)
    args = (c["d_points"], c["d_normals"], *c["d_axes"])
    vi, fi, _ = ps._index_mesh(*c["d_axes"], c["d_points"], c["d_normals"], float(c["radius"]), K, 2_000_000)
    mesh = ps.mesh_from_oriented_points(*args, radius=float(c["radius"]), K=K)
    vol = _volume(name, K)["vol"].cpu().numpy()
    rv, rf, _ = mcr.marching_cubes(vol, 0.0)
    kv, kf = psr.drop_spurious(rv, rf, vol)
    return dict(index_verts=vi, index_faces=fi, mesh=mesh, vol=vol, mc_faces=rf.shape[0], ref_verts=kv, ref_faces=kf)


# ------------------------------------------------------------------------------------------------ 1. the volume
@pytest.mark.parametrize("name,K", RUNS, ids=RUN_IDS)
def test_volume_against_the_restatements(name, K):
    from sugar_amd.point_surface import implicit_at
    c, v = _case(name), _volume(name, K)
    got = v["vol"].cpu().numpy().reshape(-1)
    r32, r64 = v["r32"][0], v["r64"][0]
    assert v["vol"].dtype == torch.float32 and tuple(v["vol"].shape) == c["shape"]
    assert np.array_equal(np.isnan(r32), np.isnan(r64))
    assert np.array_equal(np.isnan(got), np.isnan(r32)), "the defined / undefined pattern differs from the float32 restatement"
    defined = ~np.isnan(r32)
    assert defined.any() and not defined.all() and np.isfinite(got[defined]).all()
    yardstick = np.abs(r32[defined].astype(np.float64) - r64[defined]).max()
    err = np.abs(got[defined].astype(np.float64) - r64[defined]).max()
    print(f"{name} K={K}: {int(defined.sum())} defined points; |device - float64| = {err:.3g}, |float32 - float64| = {yardstick:.3g} "
          f"({yardstick / float(c['radius']):.3g} of the radius); tolerance {4 * yardstick:.3g}")
    assert yardstick > 0 and err <= 4 * yardstick
    value, weight = implicit_at(_dev(v["grid"]), c["d_points"], c["d_normals"], float(c["radius"]), K=K)
    assert torch.equal(value.view(torch.int32), v["vol"].reshape(-1).view(torch.int32)), "implicit_at and implicit_grid differ"
    w = weight.cpu().numpy()
    assert (w[~defined] == 0).all() and (w[defined] > 0).all()
    w64 = v["r64"][1]
    w_yard = np.abs(v["r32"][1][defined].astype(np.float64) - w64[defined]).max()
    assert np.abs(w[defined].astype(np.float64) - w64[defined]).max() <= 4 * w_yard


# ------------------------------------------------------------------------------------------------ 2. the brick sandwich
@pytest.mark.parametrize("name,K", RUNS, ids=RUN_IDS)
def test_brick_sandwich(name, K):
    c, v = _case(name), _volume(name, K)
    got = v["mask"].cpu().numpy()
    lower = psr.bricks_with_defined_point(v["r32"][0].reshape(c["shape"]))
    upper = psr.brick_box_rule(*c["axes"], c["points"], float(c["radius"]) * (1 + 1e-5))
    assert got.shape == lower.shape == upper.shape and got.dtype == bool
    assert not (lower & ~got).any(), "a brick holding a defined point is not active"
    assert not (got & ~upper).any(), "a brick beyond the box rule at radius (1 + 1e-5) is active"
    assert not got.all() and got.any()
    print(f"{name}: {int(got.sum())} of {got.size} bricks active; {int(lower.sum())} hold a defined point; box rule {int(upper.sum())}")


# ------------------------------------------------------------------------------------------------ 3. the face drop
@pytest.mark.parametrize("name", CASES)
def test_face_drop_is_exact(name):
    from sugar_amd.extract import grid_to_world
    c, m = _case(name), _mesh(name)
    assert m["index_verts"].dtype == torch.float32 and m["index_faces"].dtype == torch.int64
    assert 0 < m["ref_faces"].shape[0] < m["mc_faces"]
    assert np.array_equal(m["index_verts"].cpu().numpy().view(np.int32), m["ref_verts"].view(np.int32))
    assert np.array_equal(m["index_faces"].cpu().numpy(), m["ref_faces"])
    mesh = m["mesh"]
    assert sorted(mesh) == ["faces", "normals", "verts", "weights"]
    assert torch.equal(mesh["faces"], m["index_faces"]) and torch.equal(mesh["verts"], grid_to_world(m["index_verts"], *c["d_axes"]))
    assert np.array_equal(mesh["verts"].cpu().numpy(), psr.grid_to_world(m["ref_verts"], *c["axes"]))
    print(f"{name}: {m['mc_faces'] - m['ref_faces'].shape[0]} of {m['mc_faces']} faces dropped")


# ------------------------------------------------------------------------------------------------ 4. topology and accuracy
@pytest.mark.parametrize("name", CASES)
def test_topology_and_accuracy(name):
    c, m = _case(name), _mesh(name)
    verts, faces = m["mesh"]["verts"].cpu().numpy(), m["mesh"]["faces"].cpu().numpy()
    closed, boundary, no_repeat = mcr.edge_report(faces, verts.shape[0])
    assert no_repeat and closed == c["closed"]
    assert mcr.euler_characteristic(faces, verts.shape[0]) == c["chi"]
    ref_world = psr.grid_to_world(m["ref_verts"], *c["axes"])
    vol_dev, vol_ref = mcr.signed_volume_and_area(verts, faces)[0], mcr.signed_volume_and_area(ref_world, m["ref_faces"])[0]
    assert vol_dev > 0 and abs(vol_dev - vol_ref) <= 1e-3 * abs(vol_ref)
    worst, ref_worst = c["distance"](verts).max(), c["distance"](ref_world).max()
    print(f"{name}: worst vertex {worst / c['spacing']:.4f} cells off the surface (restatement {ref_worst / c['spacing']:.4f}); "
          f"{boundary.shape[0]} boundary edges")
    assert worst <= ref_worst + 0.01 * c["spacing"]
    if not c["closed"]:
        assert boundary.shape[0] > 0
        nearest = psr.exact_knn(verts, c["points"], 1)[:, 0]
        reach = np.linalg.norm(verts.astype(np.float64) - c["points"][nearest].astype(np.float64), axis=1).max()
        print(f"{name}: farthest vertex {reach / float(c['radius']):.3f} radii from a cloud point")
        assert reach <= float(c["radius"]) + c["spacing"]
    n = m["mesh"]["normals"].cpu().numpy()
    assert np.allclose(np.linalg.norm(n, axis=1), 1.0, atol=1e-5)
    outward = verts / np.linalg.norm(verts, axis=1, keepdims=True)
    if name != "B":
        assert (np.einsum("ij,ij->i", n, outward) > 0).all()                  # a sphere's normals point away from its centre


# ------------------------------------------------------------------------------------------------ 5. invariances
def _same_mesh(a, b):
    return all(torch.equal(a[k].view(torch.int32) if a[k].dtype == torch.float32 else a[k],
                           b[k].view(torch.int32) if b[k].dtype == torch.float32 else b[k]) for k in a) and sorted(a) == sorted(b)


def test_points_per_pass_and_repeatability():
    from sugar_amd import point_surface as ps
    c = _case("B")
    args = (*c["d_axes"], c["d_points"], c["d_normals"], float(c["radius"]))
    ref, ref_mask = _volume("B", 16)["vol"], _volume("B", 16)["mask"]
    for ppp in (2_000_000, 1024):
        vol, mask = ps.implicit_grid(*args, points_per_pass=ppp, return_active=True)
        assert torch.equal(vol.view(torch.int32), ref.view(torch.int32)) and torch.equal(mask, ref_mask), ppp
    m_args = (c["d_points"], c["d_normals"], *c["d_axes"])
    small = ps.mesh_from_oriented_points(*m_args, radius=float(c["radius"]), points_per_pass=1024)
    again = ps.mesh_from_oriented_points(*m_args, radius=float(c["radius"]))
    assert _same_mesh(small, _mesh("B")["mesh"]) and _same_mesh(again, _mesh("B")["mesh"])
    default_radius = ps.mesh_from_oriented_points(*m_args)                     # radius=None: 3 x the largest spacing
    assert _same_mesh(default_radius, _mesh("B")["mesh"])


def test_cloud_outside_the_grid_gives_an_empty_mesh(monkeypatch):
    from sugar_amd import point_surface as ps
    c = _case("A'")
    far = c["d_points"] + torch.tensor([5.0, 0.0, 0.0], device=DEV)
    names = []
    real_call, real_knn = ps.call, ps.knn_points
    monkeypatch.setattr(ps, "call", lambda name, *a: (names.append(name), real_call(name, *a))[1])
    monkeypatch.setattr(ps, "knn_points", lambda *a, **k: (names.append("knn_points"), real_knn(*a, **k))[1])
    mesh = ps.mesh_from_oriented_points(far, c["d_normals"], *c["d_axes"], radius=float(c["radius"]), colors=c["d_normals"])
    assert names == ["sgr_point_surface_mark", "sgr_sparse_sweep_compact"]
    assert mesh["verts"].shape == (0, 3) and mesh["faces"].shape == (0, 3) and mesh["faces"].dtype == torch.int64
    assert mesh["normals"].shape == (0, 3) and mesh["weights"].shape == (0,) and mesh["colors"].shape == (0, 3)
    vol, mask = ps.implicit_grid(*c["d_axes"], far, c["d_normals"], float(c["radius"]), return_active=True)
    assert bool(torch.isnan(vol).all()) and not bool(mask.any())


def test_bad_arguments_raise():
    from sugar_amd import point_surface as ps
    c = _case("A'")
    X, Y, Z = c["d_axes"]
    few = c["d_points"][:10], c["d_normals"][:10]
    with pytest.raises(ValueError, match="exceeds"):
        ps.implicit_grid(X, Y, Z, *few, 0.1, K=16)
    with pytest.raises(ValueError, match="exceeds"):
        ps.implicit_at(c["d_points"], *few, 0.1, K=16)
    with pytest.raises(ValueError, match=r"K must be in \[1, 32\]"):
        ps.implicit_grid(X, Y, Z, c["d_points"], c["d_normals"], 0.1, K=33)
    bad = Y.clone(); bad[20] = bad[19]
    with pytest.raises(ValueError, match="strictly ascending"):
        ps.implicit_grid(X, bad, Z, c["d_points"], c["d_normals"], 0.1)
    with pytest.raises(ValueError, match="strictly ascending"):
        ps.implicit_grid(X, bad.cpu(), Z, c["d_points"], c["d_normals"], 0.1)
    with pytest.raises(ValueError, match="radius"):
        ps.implicit_grid(X, Y, Z, c["d_points"], c["d_normals"], 0.0)
    cpu = c["d_points"].cpu(), c["d_normals"].cpu()
    for fn in (lambda: ps.implicit_grid(X, Y, Z, *cpu, 0.1), lambda: ps.implicit_at(c["d_points"].cpu(), *cpu, 0.1),
               lambda: ps.mesh_from_oriented_points(*cpu, X, Y, Z), lambda: ps.statistical_outlier_mask(cpu[0])):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn()


def test_remove_vertices_by_mask_on_the_device():
    from sugar_amd.decimate import remove_vertices_by_mask
    verts = np.arange(15, dtype=np.float32).reshape(5, 3)
    faces = np.array([[0, 1, 2], [1, 3, 2], [2, 3, 4]])
    attr = np.array([10, 11, 12, 13, 14])
    for mask in ([0, 1, 0, 0, 0], [0, 0, 0, 0, 0], [0, 0, 1, 0, 0], [1, 0, 0, 0, 1]):
        for unref in (False, True):
            want = psr.remove_vertices_by_mask(verts, faces, np.array(mask, bool), attr, unreferenced=unref)
            got = remove_vertices_by_mask(*_dev(verts, faces, np.array(mask, bool), attr), unreferenced=unref)
            assert got[1].dtype == torch.int64
            for g, w in zip(got, want):
                assert np.array_equal(g.cpu().numpy(), w), (mask, unref)


def test_outlier_mask_on_the_device():
    from sugar_amd.point_surface import statistical_outlier_mask
    g = np.random.default_rng(3)
    cloud = np.concatenate([g.uniform(-1, 1, (4200, 3)), [[300.0, 0.0, 0.0]]]).astype(np.float32)
    d = np.sqrt(((cloud[:, None, :].astype(np.float64) - cloud[None, :, :]) ** 2).sum(axis=2))
    mean20 = np.partition(d, 19, axis=1)[:, :20].mean(axis=1)
    for n, ratio in ((4201, 5.0), (4201, 80.0), (401, 5.0)):                    # the grid and the exhaustive k-NN path
        keep = statistical_outlier_mask(_dev(cloud[-n:]), 20, ratio).cpu().numpy()
        sub = np.partition(d[-n:, -n:], 19, axis=1)[:, :20].mean(axis=1) if n != 4201 else mean20
        want = psr.outlier_keep(sub, ratio)
        margin = np.abs(sub - (sub.mean() + ratio * sub.std(ddof=1))) > 1e-4     # (float32 distances: skip a point on the threshold)
        assert np.array_equal(keep[margin], want[margin]) and keep.dtype == bool
        assert keep[-1] == (ratio > 50)


# ------------------------------------------------------------------------------------------------ 6. trim and colours
def test_weight_quantile_trim():
    from sugar_amd import point_surface as ps
    c, full = _case("C"), _mesh("C")["mesh"]
    colors = torch.rand(c["d_points"].shape[0], 3, device=DEV)
    m_args = (c["d_points"], c["d_normals"], *c["d_axes"])
    trimmed = ps.mesh_from_oriented_points(*m_args, radius=float(c["radius"]), colors=colors, weight_quantile=0.25)
    w = full["weights"].cpu().numpy().astype(np.float64)
    assert (w > 0).all()
    below = w < np.quantile(w, 0.25)
    assert 0 < below.sum() < w.size
    want_v, want_f, want_w = psr.remove_vertices_by_mask(full["verts"].cpu().numpy(), full["faces"].cpu().numpy(), below,
                                                         full["weights"].cpu().numpy())
    assert np.array_equal(trimmed["verts"].cpu().numpy(), want_v) and np.array_equal(trimmed["faces"].cpu().numpy(), want_f)
    assert np.array_equal(trimmed["weights"].cpu().numpy(), want_w)
    assert trimmed["verts"].shape[0] == w.size - below.sum()
    nearest = psr.exact_knn(want_v, c["points"], 1)[:, 0]
    assert np.array_equal(trimmed["colors"].cpu().numpy(), colors.cpu().numpy()[nearest])
    assert trimmed["normals"].shape == trimmed["verts"].shape


def test_colors_follow_the_nearest_cloud_point():
    from sugar_amd import point_surface as ps
    c, full = _case("A"), _mesh("A")["mesh"]
    colors = torch.rand(c["d_points"].shape[0], 3, device=DEV)
    mesh = ps.mesh_from_oriented_points(c["d_points"], c["d_normals"], *c["d_axes"], radius=float(c["radius"]), colors=colors)
    assert torch.equal(mesh["verts"], full["verts"]) and torch.equal(mesh["faces"], full["faces"])
    verts = mesh["verts"].cpu().numpy().astype(np.float64)
    two = psr.exact_knn(verts, c["points"], 2)
    d = np.linalg.norm(verts[:, None, :] - c["points"][two].astype(np.float64), axis=2)
    clear = d[:, 1] - d[:, 0] > 1e-6                                             # (float32 k-NN: skip a vertex between two points)
    assert clear.mean() > 0.99
    assert np.array_equal(mesh["colors"].cpu().numpy()[clear], colors.cpu().numpy()[two[clear, 0]])
    w, value = mesh["weights"], ps.implicit_at(mesh["verts"], c["d_points"], c["d_normals"], float(c["radius"]))
    assert torch.equal(w, value[1]) and float(value[0].abs().max()) < 0.05 * c["spacing"]     # the vertices sit on the zero set


# ------------------------------------------------------------------------------------------------ 7. the route
ROUTE = dict(n_total_points=12_000, resolution=48, background=False)
EXTENT = 1.1


@functools.lru_cache(maxsize=None)
def _model():
    from sugar_amd import synthetic as syn
    sc = syn.make_bound_scene(20_000, 7, opaque=True).scene
    return dict(points=sc.means3D.to(DEV), scales=sc.scales.to(DEV), quats=sc.rotations.to(DEV), opacities=sc.opacities.to(DEV),
                sh_dc=sc.shs[:, 0, :].contiguous().to(DEV), shs=sc.shs.to(DEV))


def _route(model, cams, **kw):
    from sugar_amd.extract import extract_mesh_level_sets
    return extract_mesh_level_sets(model["points"], model["scales"], model["quats"], model["opacities"], model["sh_dc"], cams, EXTENT,
                                   **ROUTE, **kw)


def test_route_end_to_end():
    from sugar_amd import synthetic as syn
    from sugar_amd.extract import SH_C0
    m = _model()
    cams = syn.orbit_cameras(160, 120, n=6)
    mesh = _route(m, cams, return_cloud=True)
    V, F_ = mesh["verts"].shape[0], mesh["faces"].shape[0]
    cloud = mesh["cloud_points"]
    print(f"route: {cloud.shape[0]} sampled points -> {V} vertices, {F_} faces")
    assert cloud.shape[0] >= 16 and V > 0 and F_ > 0                            # (the sampler finds few crossings on these paper-thin Gaussians)
    assert mesh["normals"].shape == (V, 3) and mesh["colors"].shape == (V, 3) and mesh["weights"].shape == (V,)
    assert int(mesh["faces"].min()) == 0 and int(mesh["faces"].max()) == V - 1
    spacing = 2 * EXTENT / (ROUTE["resolution"] - 1)
    verts = mesh["verts"].cpu().numpy()
    nearest = psr.exact_knn(verts, cloud.cpu().numpy(), 1)[:, 0]
    reach = np.linalg.norm(verts.astype(np.float64) - cloud.cpu().numpy()[nearest].astype(np.float64), axis=1).max()
    assert reach <= float(np.float32(3.0 * spacing)) + spacing                  # both ends of a vertex's edge are within the radius of a point
    assert bool((mesh["cloud_points"].abs().max(dim=1).values < EXTENT).all())
    again = _route(m, cams, return_cloud=True)
    assert _same_mesh(mesh, again)
    g_idx = psr.exact_knn(verts, m["points"].cpu().numpy(), 2)
    d = np.linalg.norm(verts[:, None, :].astype(np.float64) - m["points"].cpu().numpy()[g_idx].astype(np.float64), axis=2)
    clear = d[:, 1] - d[:, 0] > 1e-6
    want = 0.5 + SH_C0 * m["sh_dc"].cpu().numpy()[g_idx[:, 0]]
    assert np.allclose(mesh["colors"].cpu().numpy()[clear], want[clear], atol=1e-6)


def _camera_json(i, cam):
    from sugar_amd import io
    w2c = cam.viewmatrix.cpu().numpy().T.astype(np.float64)
    fov_x, fov_y = 2 * math.atan(cam.tanfovx), 2 * math.atan(cam.tanfovy)
    return io.camera_to_json(i, f"view_{i:03d}", w2c[:3, :3].T, w2c[:3, 3], fov_x, fov_y, cam.image_width, cam.image_height)


def test_command_line(tmp_path, capsys):
    from sugar_amd import extract, io, synthetic as syn
    from sugar_amd.extract import extract_mesh_marching_cubes
    m = _model()
    P = m["points"].shape[0]
    cloud = str(tmp_path / "point_cloud.ply")
    io.save_gaussian_ply(cloud, m["points"], m["shs"], torch.logit(m["opacities"]).reshape(P, 1), torch.log(m["scales"]), m["quats"])
    cam_path = str(tmp_path / "cameras.json")
    with open(cam_path, "w") as f:
        json.dump([_camera_json(i, c) for i, c in enumerate(syn.orbit_cameras(160, 120, n=6))], f)
    g = io.load_gaussian_ply(cloud, device=DEV)
    loaded = dict(points=g["xyz"], scales=torch.exp(g["scaling"]), quats=g["rotation"], opacities=torch.sigmoid(g["opacity"]),
                  sh_dc=g["features"][:, 0, :])
    cams, _ = io.cameras_from_json(cam_path, device=DEV)
    assert len(cams) == 6 and (cams[0].image_width, cams[0].image_height) == (160, 120)
    want = _route(loaded, cams)
    out = str(tmp_path / "levelset.ply")
    assert extract.main([cloud, "--route", "levelset", "--cameras", cam_path, "--out", out, "--n-points", "12000", "--resolution", "48",
                         "--extent", str(EXTENT), "--no-background"]) == 0
    assert "not Poisson" in capsys.readouterr().out
    got = io.load_mesh_ply(out)
    assert want["verts"].shape[0] > 0
    assert np.array_equal(got["verts"].numpy(), want["verts"].cpu().numpy()) and np.array_equal(got["faces"].numpy(), want["faces"].cpu().numpy())
    assert np.array_equal(got["normals"].numpy(), want["normals"].cpu().numpy())
    rgb = np.rint(np.clip(want["colors"].cpu().numpy().astype(np.float64), 0.0, 1.0) * 255.0).astype(np.uint8)
    assert np.array_equal(got["colors"].numpy(), rgb) and rgb.std() > 10
    # the default route is what it was: the marching-cubes command writes what extract_mesh_marching_cubes returns
    out_mc = str(tmp_path / "mc.ply")
    assert extract.main([cloud, "--out", out_mc, "--resolution", "48", "--extent", str(EXTENT), "--no-background"]) == 0
    mc = extract_mesh_marching_cubes(loaded["points"], loaded["scales"], loaded["quats"], loaded["opacities"], loaded["sh_dc"], EXTENT,
                                     resolution=48, background=False)
    got = io.load_mesh_ply(out_mc)
    assert np.array_equal(got["verts"].numpy(), mc["verts"].cpu().numpy()) and np.array_equal(got["faces"].numpy(), mc["faces"].cpu().numpy())
    assert np.array_equal(got["normals"].numpy(), mc["normals"].cpu().numpy())
