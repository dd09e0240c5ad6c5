"""GPU tests of the marching-cubes extraction (csrc/marching_cubes.hip, sugar_amd.marching_cubes, sugar_amd.extract):

  * the kernels against the serial restatement tests/mc_restatement.py, bit for bit (vertices, faces, counts), on the analytic fields of
    tests/test_marching_cubes_cpu.py, a smooth random field, empty / full volumes and a volume with NaN and +-inf entries;
  * `density_grid` against the fixture the reference's own `compute_density` wrote (tests/golden/sugar_mcgrid.npz), and its slab sweep;
  * full size (512^3 over a 1M-Gaussian bound scene, a 512 x 384 x 640 torus): run-to-run identity, closedness, vertices on grid edges,
    normals, colours, peak memory;
  * no host synchronisation outside the one documented read of (V, F);
  * end to end into the refine stage's topology and normal-consistency kernels."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import mc_restatement as mcr  # noqa: E402
import test_marching_cubes_cpu as cpu  # noqa: E402

pytestmark = pytest.mark.gpu
LEVEL = cpu.LEVEL
DEV = "cuda:0"


def _hip(vol_np, level=LEVEL):
    from sugar_amd.marching_cubes import marching_cubes
    verts, faces = marching_cubes(torch.from_numpy(np.ascontiguousarray(vol_np)).to(DEV), level)
    assert verts.dtype == torch.float32 and faces.dtype == torch.int64 and verts.shape[1:] == (3,) and faces.shape[1:] == (3,)
    return verts.cpu().numpy(), faces.cpu().numpy()


def _assert_identical(vol_np, level=LEVEL):
    rv, rf, _ = mcr.marching_cubes(vol_np, level)
    hv, hf = _hip(vol_np, level)
    assert hv.shape == rv.shape and hf.shape == rf.shape, (hv.shape, rv.shape, hf.shape, rf.shape)
    assert np.array_equal(hv.view(np.uint32), rv.view(np.uint32))
    assert np.array_equal(hf, rf)
    return hv, hf


# ------------------------------------------------------------------------------------------------ restatement parity
@pytest.mark.parametrize("name", ["sphere", "torus", "two_spheres", "cut_sphere"])
def test_kernels_match_the_restatement_on_analytic_fields(name):
    hv, hf = _assert_identical(cpu.field(name, (64, 64, 64)))
    assert len(hv) and len(hf)


def test_kernels_match_the_restatement_on_a_rectangular_grid():
    _assert_identical(cpu.rect_sphere())


def test_kernels_match_the_restatement_on_a_smooth_random_field():
    hv, hf = _assert_identical(cpu.smooth_random(96))
    assert len(hf) > 10000


@pytest.mark.parametrize("name", ["empty", "full"])
def test_empty_and_full_volumes_give_no_mesh(name):
    hv, hf = _hip(cpu.field(name, (64, 64, 64)))
    assert hv.shape == (0, 3) and hf.shape == (0, 3)


def test_small_and_degenerate_shapes():
    for shape in ((1, 1, 1), (1, 7, 9), (2, 2, 2), (3, 17, 5), (9, 8, 33)):
        g = np.random.default_rng(sum(shape))
        _assert_identical((LEVEL + g.standard_normal(shape)).astype(np.float32))


def test_non_finite_values_count_as_outside_and_never_give_a_nan_vertex():
    """the stated rule: NaN, +inf and -inf corners are outside; an edge whose outside end is not finite puts its vertex at t = 0.5.
    (Finite ends whose difference overflows give t = 0; t = inf / inf -> 0.5 needs iso - a to overflow too, which no level near 0.3 can.)"""
    vol = cpu.field("sphere", (64, 64, 64))
    g = np.random.default_rng(0)
    idx = g.integers(0, 64, size=(600, 3))
    for k, (i, j, l) in enumerate(idx):
        vol[i, j, l] = (np.nan, np.inf, -np.inf)[k % 3]
    vol[10:14, 10:14, 10:14] = np.nan
    vol[40, 40, 40] = 3.0e38; vol[40, 40, 41] = -3.0e38      # b - a overflows to +inf: t = finite / inf = 0, the vertex sits on the outside grid point
    hv, hf = _assert_identical(vol)
    assert np.isfinite(hv).all() and hf.min() >= 0 and hf.max() < len(hv)
    _, _, aux = mcr.marching_cubes(vol, LEVEL)
    assert (aux["t"] == 0.5).sum() > 100


def test_grids_of_2_to_31_points_are_refused(hip_lib):
    from sugar_amd.marching_cubes import marching_cubes
    from sugar_amd.extract import density_grid
    huge = torch.zeros(1, device=DEV).expand(2048, 1024, 1024)      # 2^31 points, one float of storage
    with pytest.raises(ValueError, match="refused"):
        marching_cubes(huge, 0.5)
    with pytest.raises(ValueError, match="refused"):
        density_grid(torch.zeros(2048), torch.zeros(1024), torch.zeros(1024), torch.zeros(8, 3, device=DEV),
                     torch.zeros(8, 3, 3, device=DEV), torch.zeros(8, device=DEV))
    assert hip_lib.sgr_marching_cubes_count(2048, 1024, 1024, None, 0.5, None, None, None) == -1
    assert hip_lib.sgr_marching_cubes_scratch_bytes(2048, 1024, 1024) == 0


def test_mcubes_stand_in_returns_numpy_arrays():
    from sugar_amd import shims
    shims.install()
    import mcubes
    if not os.path.abspath(mcubes.__file__).startswith(os.path.join(os.path.dirname(HERE), "sugar_amd", "shims")):
        pytest.skip("a real PyMCubes is installed and wins")
    vol = cpu.field("torus", (48, 48, 48))
    v, f = mcubes.marching_cubes(vol, LEVEL)
    rv, rf, _ = mcr.marching_cubes(vol, LEVEL)
    assert isinstance(v, np.ndarray) and isinstance(f, np.ndarray) and v.dtype == np.float64
    assert np.array_equal(v.astype(np.float32), rv) and np.array_equal(f, rf)


# ------------------------------------------------------------------------------------------------ density_grid
def _rel(a, b):
    a = torch.as_tensor(a).detach().cpu().double(); b = torch.as_tensor(b).double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def test_density_grid_replays_the_reference_fixture():
    from sugar_amd.extract import density_grid
    from sugar_amd.knn import knn_points
    FX = np.load(os.path.join(HERE, "golden", "sugar_mcgrid.npz"))
    t = lambda k: torch.from_numpy(FX[k]).to(DEV)
    pts, B, st = t("points"), t("inv_scaled_rot"), t("strengths")
    # the neighbour choice of reset_neighbors(16) is the exact k-NN's: the HIP k-NN agrees with the recorded table (first column: itself).
    # Not compared for equality because of near-ties: the table was written by a float64 k-d tree, the HIP k-NN ranks float32 squared
    # distances, and two neighbours whose distances differ in the last float32 bits may swap places (or the 16th with the 17th).
    idx = knn_points(pts[None], pts[None], K=16).idx[0]
    assert (idx.cpu().numpy() == FX["knn_idx"]).mean() > 0.999
    vol = density_grid(t("X"), t("Y"), t("Z"), pts, B, st, K=16)
    assert vol.shape == (40, 40, 40) and vol.dtype == torch.float32
    rel = _rel(vol, FX["density"])
    print("density_grid vs the reference's compute_density: rel", rel)
    assert rel < 2e-5
    # several slabs (a slab size that divides nothing): bit-identical to the single pass
    for ppp in (7001, 64000 - 1, 1000):
        assert torch.equal(density_grid(t("X"), t("Y"), t("Z"), pts, B, st, K=16, points_per_pass=ppp), vol)
    # the background pass's blanking: strictly inside the box -> 0, everything else untouched
    z = density_grid(t("X"), t("Y"), t("Z"), pts, B, st, K=16, zero_inside=(-0.5, 0.5))
    X = FX["X"]
    m = (X > -0.5) & (X < 0.5)
    box = torch.from_numpy(m[:, None, None] & m[None, :, None] & m[None, None, :]).to(DEV)
    assert (z[box] == 0).all() and torch.equal(z[~box], vol[~box]) and 0 < int(box.sum()) < 64000


# ------------------------------------------------------------------------------------------------ full size
def _edge_check(faces, n_verts):
    """(no directed edge repeats, boundary vertex ids): boundary = ends of the directed edges whose reverse is absent"""
    f = faces
    e = torch.cat([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    key = e[:, 0] * n_verts + e[:, 1]
    rkey = e[:, 1] * n_verts + e[:, 0]
    skey = torch.sort(key).values
    no_repeat = bool((skey[1:] != skey[:-1]).all())
    pos = torch.searchsorted(skey, rkey).clamp_max(skey.numel() - 1)
    has_rev = skey[pos] == rkey
    return no_repeat, e[~has_rev].reshape(-1)


def _check_vertices(vol, level, verts):
    """every vertex lies on a grid edge; recomputing t = (level - a) / (b - a) from the volume with the same float32 operations gives
    the vertex back bit for bit, and a + t (b - a) equals the level within 4 ulp of max(|a|, |b|, |level|) (reasoning: see
    tests/test_marching_cubes_cpu.py:check_vertices_on_edges)"""
    nx, ny, nz = vol.shape
    fl = verts.floor()
    frac = verts != fl
    assert int(frac.sum(dim=1).max()) <= 1
    # a vertex whose i + t rounds to a whole number (t within 2^-15 of an end at i ~ 256) names no axis: rare, and only bounds-checked
    at_point = ~frac.any(dim=1)
    assert float(at_point.float().mean()) < 1e-3
    hi = torch.tensor([nx - 1, ny - 1, nz - 1], device=vol.device, dtype=torch.float32)
    assert (verts >= 0).all() and (verts <= hi).all()
    v, f0 = verts[~at_point], fl[~at_point].long()
    axis = frac[~at_point].float().argmax(dim=1)
    step = torch.nn.functional.one_hot(axis, 3)
    f1 = f0 + step
    assert (f0 >= 0).all() and (f1[:, 0] < nx).all() and (f1[:, 1] < ny).all() and (f1[:, 2] < nz).all()
    a, b = vol[f0[:, 0], f0[:, 1], f0[:, 2]], vol[f1[:, 0], f1[:, 1], f1[:, 2]]
    lv = torch.tensor(level, dtype=torch.float32, device=vol.device)
    ins = lambda x: torch.isfinite(x) & (x >= lv)
    lo_in = ins(a)
    assert (lo_in != ins(b)).all()
    out_v, in_v = torch.where(lo_in, b, a), torch.where(lo_in, a, b)
    t = (lv - out_v) / (in_v - out_v)
    t = torch.where(torch.isfinite(out_v) & torch.isfinite(t), t, torch.full_like(t, 0.5))
    i = f0.gather(1, axis[:, None])[:, 0].float()
    coord = torch.where(lo_in, (i + 1.0) - t, i + t)
    assert torch.equal(coord, v.gather(1, axis[:, None])[:, 0])
    ok = torch.isfinite(out_v)
    interp = out_v[ok].double() + t[ok].double() * (in_v[ok].double() - out_v[ok].double())
    scale = torch.maximum(torch.maximum(out_v[ok].abs(), in_v[ok].abs()), lv.abs())
    ulp = torch.nextafter(scale, torch.full_like(scale, float("inf"))) - scale
    err = (interp - lv.double()).abs()
    assert (err <= 4 * ulp.double()).all(), float((err / ulp.double()).max())


def _full_size_checks(vol, level, record_property, tag):
    from sugar_amd.marching_cubes import marching_cubes, vertex_normals
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    verts, faces = marching_cubes(vol, level)
    peak = torch.cuda.max_memory_allocated() - base
    v2, f2 = marching_cubes(vol, level)
    assert torch.equal(verts.view(torch.int32), v2.view(torch.int32)) and torch.equal(faces, f2)
    del v2, f2
    V, F_ = verts.shape[0], faces.shape[0]
    print(f"{tag}: {V} vertices, {F_} faces, peak extra memory in marching_cubes {peak / 2 ** 20:.0f} MiB (volume {vol.numel() * 4 / 2 ** 20:.0f} MiB)")
    record_property(tag + "_vertices", V); record_property(tag + "_faces", F_); record_property(tag + "_peak_mib", peak / 2 ** 20)
    assert torch.isfinite(verts).all()
    if F_:
        assert int(faces.min()) >= 0 and int(faces.max()) < V
        no_repeat, boundary = _edge_check(faces, V)
        assert no_repeat
        hi = torch.tensor(vol.shape, device=vol.device, dtype=torch.float32) - 1
        bv = verts[boundary]
        assert (((bv == 0) | (bv == hi)).any(dim=1)).all()     # the mesh is closed away from the volume's faces
        _check_vertices(vol, level, verts)
        n = vertex_normals(verts, faces)
        assert torch.equal(n, vertex_normals(verts, faces))
        length = n.norm(dim=1)
        assert (((length - 1).abs() < 1e-5) | (length == 0)).all()
    return verts, faces


def test_full_size_torus(record_property):
    nx, ny, nz = 512, 384, 640
    h = 1.0 / 639
    ax = [torch.arange(n, dtype=torch.float64, device=DEV) * h for n in (nx, ny, nz)]
    # the volume spans [0, 0.8] x [0, 0.6] x [0, 1]: the torus (outer radius R + r = 0.271 around the z axis through c) lies inside it
    c = torch.tensor([0.4 + np.sqrt(2.0) / 100, 0.29 + np.sqrt(3.0) / 100, 0.5 + np.pi / 1000], dtype=torch.float64)
    R, r = 0.19 + np.sqrt(5.0) / 100, 0.05 + np.sqrt(7.0) / 300
    q = torch.sqrt((ax[0][:, None] - c[0]) ** 2 + (ax[1][None, :] - c[1]) ** 2) - R          # [nx, ny]
    vol = torch.empty(nx, ny, nz, dtype=torch.float32, device=DEV)
    for i0 in range(0, nx, 64):                                                                # float64 -> float32 in slabs
        vol[i0:i0 + 64] = (LEVEL + r - torch.sqrt(q[i0:i0 + 64, :, None] ** 2 + (ax[2][None, None, :] - c[2]) ** 2)).float()
    verts, faces = _full_size_checks(vol, LEVEL, record_property, "torus_512x384x640")
    assert faces.shape[0] > 100000
    no_repeat, boundary = _edge_check(faces, verts.shape[0])
    assert boundary.numel() == 0                                                               # the torus lies inside the volume: closed
    und = torch.unique(torch.minimum(faces[:, [0, 1, 2]], faces[:, [1, 2, 0]]) * verts.shape[0] + torch.maximum(faces[:, [0, 1, 2]], faces[:, [1, 2, 0]]))
    assert verts.shape[0] - und.numel() + faces.shape[0] == 0                                  # Euler characteristic of a torus


def test_full_size_bound_scene(record_property):
    """make_bound_scene(1M, opaque=True): the density grid at 512^3 over the scene's extent, then the mesh.  The scene's Gaussians are
    3.3e-6 thick against a grid spacing of 0.013, so hardly any grid point sees a density above the level: the mesh is ~1 485 isolated
    octahedra (8 904 vertices, 11 880 faces), one around each lone inside point.  This case is the full-size SWEEP and run-to-run
    identity; the connected full-size surface is test_full_size_torus."""
    from sugar_amd import field, synthetic as syn
    from sugar_amd.extract import density_grid, grid_to_world, nearest_gaussian_colors, SH_C0
    from sugar_amd.knn import knn_points
    bs = syn.make_bound_scene(1_000_000, 7, opaque=True)
    sc = bs.scene
    pts = sc.means3D.to(DEV).contiguous()
    B = field.scaled_rotation(sc.rotations.to(DEV), sc.scales.to(DEV), True)
    st = sc.opacities.to(DEV).reshape(-1)
    dc = sc.shs[:, 0, :].to(DEV).contiguous()
    extent = float(pts.abs().max()) * 1.05
    X = torch.linspace(-1, 1, 512, device=DEV) * extent
    torch.cuda.reset_peak_memory_stats()
    t0 = torch.cuda.Event(enable_timing=True); t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    vol = density_grid(X, X, X, pts, B, st, K=16)
    t1.record(); torch.cuda.synchronize()
    print(f"density_grid 512^3 over {pts.shape[0]} Gaussians: {t0.elapsed_time(t1):.0f} ms, peak {torch.cuda.max_memory_allocated() / 2 ** 20:.0f} MiB")
    record_property("density_grid_ms", t0.elapsed_time(t1))
    assert torch.isfinite(vol).all()
    verts, faces = _full_size_checks(vol, LEVEL, record_property, "bound_scene_512")
    world = grid_to_world(verts, X, X, X)
    colors, idx = nearest_gaussian_colors(world, pts, dc)
    if verts.shape[0]:
        ref_idx = knn_points(world[None].contiguous(), pts[None], K=1).idx[0, :, 0]
        assert torch.equal(idx, ref_idx) and torch.equal(colors, 0.5 + SH_C0 * dc[ref_idx])


# ------------------------------------------------------------------------------------------------ synchronisation
def test_no_host_synchronisation_outside_the_one_read_back():
    from sugar_amd.extract import density_grid
    from sugar_amd.marching_cubes import mc_count, mc_emit, vertex_normals
    FX = np.load(os.path.join(HERE, "golden", "sugar_mcgrid.npz"))
    t = lambda k: torch.from_numpy(FX[k]).to(DEV)
    args = (t("X"), t("Y"), t("Z"), t("points"), t("inv_scaled_rot"), t("strengths"))
    density_grid(*args, points_per_pass=9000); torch.cuda.synchronize()      # (warm: code objects, the allocator)
    torch.cuda.set_sync_debug_mode("error")
    try:
        vol = density_grid(*args, points_per_pass=9000, zero_inside=(-0.1, 0.1))
        state, counts = mc_count(vol, LEVEL)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    n_verts, n_faces = counts.tolist()                                        # the one documented read-back
    assert n_verts > 0 and n_faces > 0
    torch.cuda.set_sync_debug_mode("error")
    try:
        verts, faces = mc_emit(state, n_verts, n_faces)
        normals = vertex_normals(verts, faces)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    rv, rf, _ = mcr.marching_cubes(vol.cpu().numpy(), LEVEL)
    assert np.array_equal(verts.cpu().numpy().view(np.uint32), rv.view(np.uint32)) and np.array_equal(faces.cpu().numpy(), rf)
    assert torch.isfinite(normals).all()


# ------------------------------------------------------------------------------------------------ end to end
def test_extracted_mesh_feeds_the_refine_stage(tmp_path):
    from sugar_amd import io
    from sugar_amd.extract import extract_mesh_marching_cubes
    from sugar_amd.mesh_bind import MeshTopology, normal_consistency
    g = torch.Generator().manual_seed(5)
    P = 20000
    d = torch.nn.functional.normalize(torch.randn(P, 3, generator=g), dim=-1)
    pts = (d * (0.55 + 0.1 * torch.sin(3 * d[:, :1]))).to(DEV)
    far = (torch.nn.functional.normalize(torch.randn(P // 4, 3, generator=g), dim=-1) * 2.5).to(DEV)     # a shell for the background pass
    pts = torch.cat([pts, far])
    n = pts.shape[0]
    scales = torch.cat([torch.full((P, 3), 0.03), torch.full((P // 4, 3), 0.12)]).to(DEV)
    quats = torch.randn(n, 4, generator=g).to(DEV)
    opac = torch.full((n,), 0.9, device=DEV)
    dc = (torch.rand(n, 1, 3, generator=g).to(DEV) - 0.5) / 0.28209479177387814
    mesh = extract_mesh_marching_cubes(pts, scales, quats, opac, dc, extent=1.0, resolution=96, level=LEVEL, background=True,
                                       points_per_pass=300_000)
    V, F_ = mesh["verts"].shape[0], mesh["faces"].shape[0]
    fg_only = extract_mesh_marching_cubes(pts, scales, quats, opac, dc, extent=1.0, resolution=96, level=LEVEL, background=False)
    assert 0 < fg_only["verts"].shape[0] < V and torch.equal(mesh["verts"][:fg_only["verts"].shape[0]], fg_only["verts"])
    assert (mesh["verts"][:fg_only["verts"].shape[0]].abs() <= 1.0).all() and float(mesh["verts"].abs().max()) > 1.5
    assert mesh["normals"].shape == (V, 3) and mesh["colors"].shape == (V, 3) and int(mesh["faces"].max()) < V
    path = str(tmp_path / "mesh.ply")
    io.save_mesh_ply(path, mesh["verts"], mesh["faces"], normals=mesh["normals"], colors=mesh["colors"])
    back = io.load_mesh_ply(path, device=DEV)
    assert torch.equal(back["verts"], mesh["verts"]) and torch.equal(back["faces"], mesh["faces"]) and torch.equal(back["normals"], mesh["normals"])
    assert torch.equal(back["colors"].float(), torch.round(mesh["colors"].clamp(0, 1).double() * 255).float())
    topo = MeshTopology.get(back["faces"], V)
    assert topo.n_faces == F_ and topo.n_pairs > 0
    loss = normal_consistency(back["verts"], back["faces"])
    assert torch.isfinite(loss) and 0 <= float(loss) < 1


def test_command_line(tmp_path):
    from sugar_amd import extract, io
    g = torch.Generator().manual_seed(2)
    P = 5000
    d = torch.nn.functional.normalize(torch.randn(P, 3, generator=g), dim=-1)
    feats = torch.zeros(P, 16, 3); feats[:, 0] = torch.rand(P, 3, generator=g)
    cloud = str(tmp_path / "point_cloud.ply")
    io.save_gaussian_ply(cloud, d * 0.5, feats, torch.full((P, 1), 3.0), torch.full((P, 3), float(np.log(0.04))), torch.randn(P, 4, generator=g))
    out = str(tmp_path / "mesh.ply")
    assert extract.main([cloud, "--out", out, "--resolution", "64", "--level", "0.3", "--extent", "0.8", "--no-background"]) == 0
    m = io.load_mesh_ply(out)
    assert m["verts"].shape[0] > 100 and m["faces"].shape[0] > 100 and float(m["verts"].abs().max()) <= 0.8
