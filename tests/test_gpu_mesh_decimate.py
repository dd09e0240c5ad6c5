"""GPU tests of the mesh decimation and cleaning (csrc/mesh_decimate.hip, sugar_amd.decimate, sugar_amd.extract):

  * the kernels against the serial restatement tests/decimate_restatement.py -- identical faces, bit-identical vertices -- on the four
    analytic fields at 64^3 (cut_sphere has a boundary), a smooth random field at 96^3 (it meets the volume's faces: boundary too) and
    the tetrahedron that cannot be decimated;
  * the cleaning passes against their restatement on the hand-built meshes and on a 64^3 mesh with 1 % of its faces duplicated and
    1 % made degenerate;
  * full size: the 512 x 384 x 640 torus of tests/test_gpu_marching_cubes.py (586 284 faces) to 200 000 faces: run-to-run identity,
    the face-count window, closedness, Euler characteristic, accuracy against a direct mesh of the same budget, one host read per round;
  * end to end through extract_mesh_marching_cubes(..., decimation_target=T, clean=True) into the refine stage's topology."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import decimate_restatement as dr  # noqa: E402
import mc_restatement as mcr  # noqa: E402
import test_marching_cubes_cpu as cpu  # noqa: E402
import test_mesh_decimate_cpu as dcpu  # noqa: E402

pytestmark = pytest.mark.gpu
LEVEL = cpu.LEVEL
DEV = "cuda:0"


def _hip_decimate(v, f, target, **kw):
    from sugar_amd.decimate import decimate
    hv, hf, info = decimate(torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV), target, **kw)
    assert hv.dtype == torch.float32 and hf.dtype == torch.int64 and hv.shape[1:] == (3,) and hf.shape[1:] == (3,)
    return hv.cpu().numpy(), hf.cpu().numpy(), info


def _assert_identical(v, f, target, **kw):
    rv, rf, rinfo = dr.decimate(v, f, target, **kw)
    hv, hf, hinfo = _hip_decimate(v, f, target, **kw)
    print("restatement", rinfo, "kernels", hinfo)
    assert hinfo == rinfo
    assert hf.shape == rf.shape and np.array_equal(hf, rf)
    assert hv.shape == rv.shape and np.array_equal(hv.view(np.uint32), rv.view(np.uint32))
    return hv, hf, hinfo


# ------------------------------------------------------------------------------------------------ restatement parity
@pytest.mark.parametrize("name", dcpu.FIELDS)
def test_kernels_match_the_restatement_on_analytic_fields(name):
    v, f = dcpu.mc_mesh(name, 64)
    target = dcpu.FACES[32][name]
    hv, hf, info = _assert_identical(v, f, target)
    assert target - 2 < len(hf) <= target and info["target_met"] and info["rounds"] <= info["round_limit"]


def test_kernels_match_the_restatement_with_another_boundary_weight():
    v, f = dcpu.mc_mesh("cut_sphere", 64)
    a = _assert_identical(v, f, 1672, boundary_weight=8.0)
    b = dcpu.decimated("cut_sphere")
    assert not np.array_equal(a[1], b[1])                                    # the weight matters


def test_kernels_match_the_restatement_on_a_smooth_random_field():
    rv, rf, _ = mcr.marching_cubes(cpu.smooth_random(96), LEVEL)
    v = (rv / np.float32(95)).astype(np.float32)
    assert len(rf) > 10000
    target = len(rf) // 4
    hv, hf, info = _assert_identical(v, rf, target)
    assert target - 2 < len(hf) <= target


def test_small_cases():
    v, f = dcpu.tetrahedron()
    hv, hf, info = _assert_identical(v, f, 0)
    assert not info["target_met"] and info["faces"] == 4 and info["rounds"] == 1
    v, f = dcpu.mc_mesh("sphere", 32)
    hv, hf, info = _hip_decimate(v, f, len(f))
    assert info["rounds"] == 0 and np.array_equal(hv.view(np.uint32), v.view(np.uint32)) and np.array_equal(hf, f)
    from sugar_amd.decimate import decimate
    with pytest.raises(ValueError, match="outside"):
        decimate(torch.from_numpy(v).to(DEV), torch.from_numpy(f + len(v)).to(DEV), 100)


# ------------------------------------------------------------------------------------------------ cleaning
def _assert_clean_identical(v, f, **kw):
    from sugar_amd.decimate import clean
    rv, rf, rmap = dr.clean(v, f, **kw)
    hv, hf, hmap = clean(torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV), **kw)
    assert hv.dtype == torch.float32 and hf.dtype == torch.int64 and hmap.dtype == torch.int64
    assert np.array_equal(hf.cpu().numpy().reshape(-1, 3), rf.reshape(-1, 3))
    assert np.array_equal(hv.cpu().numpy().view(np.uint32), rv.view(np.uint32))
    assert np.array_equal(hmap.cpu().numpy(), rmap)
    return rv, rf


def test_cleaning_matches_the_restatement_on_hand_built_meshes():
    for name, (v, f) in dcpu.hand_built_meshes().items():
        _assert_clean_identical(v, f)
        for off in ("degenerate", "duplicated_triangles", "duplicated_vertices", "non_manifold_edges"):
            _assert_clean_identical(v, f, **{off: False})


def test_cleaning_matches_the_restatement_on_a_damaged_mesh():
    v, f = dcpu.mc_mesh("sphere", 64)
    g = np.random.default_rng(11)
    n = len(f) // 100
    pick = g.choice(len(f), size=2 * n, replace=False)
    f = f.copy()
    f[pick[:n], 2] = f[pick[:n], 1]                                          # 1 % degenerate
    dup = np.roll(f[pick[n:]], 1, axis=1)                                    # 1 % duplicated, in a rotated vertex order
    where = np.sort(g.choice(len(f), size=n, replace=False))
    f = np.insert(f, where, dup, axis=0)
    twins = g.choice(len(v), size=50, replace=False)                         # 50 vertices get a bit-equal twin that some faces use
    v = np.concatenate([v, v[twins]])
    for k, t in enumerate(twins):
        rows = np.nonzero((f == t).any(axis=1))[0][:2]
        f[rows] = np.where(f[rows] == t, len(v) - 50 + k, f[rows])
    rv, rf = _assert_clean_identical(v, f)
    assert dcpu.FACES[64]["sphere"] - 2 * n - 100 <= len(rf) <= dcpu.FACES[64]["sphere"] - n and len(rv) <= len(v) - 50
    _assert_clean_identical(v, f, duplicated_vertices=False)
    v0, f0 = dcpu.mc_mesh("torus", 64)
    cv, cf = _assert_clean_identical(v0, f0)
    assert np.array_equal(cf, f0) and np.array_equal(cv.view(np.uint32), v0.view(np.uint32))      # the identity on a clean mesh


# ------------------------------------------------------------------------------------------------ full size
def _torus_volume(nx, ny, nz):
    """the torus of tests/test_gpu_marching_cubes.py::test_full_size_torus on an nx x ny x nz grid of spacing 1 / (nz - 1)"""
    h = 1.0 / (nz - 1)
    ax = [torch.arange(n, dtype=torch.float64, device=DEV) * h for n in (nx, ny, nz)]
    c = torch.tensor([0.4 + np.sqrt(2.0) / 100, 0.29 + np.sqrt(3.0) / 100, 0.5 + np.pi / 1000], dtype=torch.float64)
    R, r = 0.19 + np.sqrt(5.0) / 100, 0.05 + np.sqrt(7.0) / 300
    q = torch.sqrt((ax[0][:, None] - c[0]) ** 2 + (ax[1][None, :] - c[1]) ** 2) - R
    vol = torch.empty(nx, ny, nz, dtype=torch.float32, device=DEV)
    for i0 in range(0, nx, 64):
        vol[i0:i0 + 64] = (LEVEL + r - torch.sqrt(q[i0:i0 + 64, :, None] ** 2 + (ax[2][None, None, :] - c[2]) ** 2)).float()
    return vol, h, (c, R, r)


def _torus_error(verts, faces, params):
    c, R, r = params
    c = c.to(verts.device)

    def dist(p):
        q = torch.sqrt((p[:, 0] - c[0]) ** 2 + (p[:, 1] - c[1]) ** 2) - R
        return (r - torch.sqrt(q * q + (p[:, 2] - c[2]) ** 2)).abs().max()
    v = verts.double()
    cen = (v[faces[:, 0]] + v[faces[:, 1]] + v[faces[:, 2]]) / 3.0
    return float(torch.maximum(dist(v), dist(cen)))


def _edge_counts(faces, n_verts):
    e = torch.cat([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    key = torch.minimum(e[:, 0], e[:, 1]) * n_verts + torch.maximum(e[:, 0], e[:, 1])
    return torch.unique(key, return_counts=True)


def test_full_size_torus_to_200k_faces(record_property):
    from sugar_amd.decimate import decimate, round_limit
    from sugar_amd.marching_cubes import marching_cubes
    TARGET = 200_000
    vol, h, params = _torus_volume(512, 384, 640)
    vi, faces = marching_cubes(vol, LEVEL)
    del vol
    verts = vi * h
    F0 = faces.shape[0]
    assert F0 > 500_000
    decimate(verts[:0].new_tensor(dcpu.tetrahedron()[0]), torch.from_numpy(dcpu.tetrahedron()[1]).to(DEV), 0)      # (warm: code objects)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    v1, f1, info = decimate(verts, faces, TARGET)
    t1.record(); torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    ms = t0.elapsed_time(t1)
    print(f"torus {F0} -> {f1.shape[0]} faces: {info}, {ms:.0f} ms, {ms / max(info['rounds'], 1):.1f} ms per round, peak extra {peak / 2 ** 20:.0f} MiB")
    for k, val in (("faces_in", F0), ("faces_out", f1.shape[0]), ("rounds", info["rounds"]), ("ms", ms), ("peak_mib", peak / 2 ** 20)):
        record_property("decimate_torus_" + k, val)
    # the second run, with every host synchronisation reported: one read before the first round and one per round
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            v2, f2, info2 = decimate(verts, faces, TARGET)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    reads = [w for w in caught if "synchroniz" in str(w.message).lower()]
    print("host reads:", len(reads), "rounds:", info2["rounds"])
    assert 1 <= len(reads) <= info2["rounds"] + 1
    assert info2 == info and torch.equal(v1.view(torch.int32), v2.view(torch.int32)) and torch.equal(f1, f2)
    assert TARGET - 2 < f1.shape[0] <= TARGET and info["target_met"]
    assert info["rounds"] <= info["round_limit"] == round_limit(F0, TARGET)
    V1 = v1.shape[0]
    assert torch.isfinite(v1).all() and int(f1.min()) == 0 and int(f1.max()) == V1 - 1
    und, counts = _edge_counts(f1, V1)
    assert bool((counts == 2).all())                                         # closed: every edge has exactly two faces
    assert V1 - und.numel() + f1.shape[0] == 0                               # Euler characteristic of a torus
    # accuracy: the direct marching-cubes mesh of the same budget -- the finest grid of the same proportions with at most TARGET faces
    yard = None
    for nz in range(320, 200, -8):
        vol_c, hc, _ = _torus_volume(int(round(nz * 0.8)), int(round(nz * 0.6)), nz)
        cv, cf = marching_cubes(vol_c, LEVEL)
        if cf.shape[0] <= TARGET:
            yard = (nz, cf.shape[0], _torus_error(cv * hc, cf, params))
            break
    assert yard is not None
    e_dec = _torus_error(v1, f1, params)
    ratio = e_dec / yard[2]
    print(f"E(decimated) {e_dec:.4e}; E(direct, nz = {yard[0]}, {yard[1]} faces) {yard[2]:.4e}; ratio {ratio:.3f}")
    record_property("decimate_torus_error_ratio", ratio)
    assert ratio <= max(1.0, 1.25 * dcpu.MEASURED_RATIO["torus"])


# ------------------------------------------------------------------------------------------------ end to end
def test_decimated_extraction_feeds_the_refine_stage():
    from sugar_amd.extract import extract_mesh_marching_cubes
    from sugar_amd.mesh_bind import MeshTopology, normal_consistency
    g = torch.Generator().manual_seed(5)
    P = 20000
    d = torch.nn.functional.normalize(torch.randn(P, 3, generator=g), dim=-1)
    pts = (d * (0.55 + 0.1 * torch.sin(3 * d[:, :1]))).to(DEV)
    far = (torch.nn.functional.normalize(torch.randn(P // 4, 3, generator=g), dim=-1) * 2.5).to(DEV)
    pts = torch.cat([pts, far])
    n = pts.shape[0]
    scales = torch.cat([torch.full((P, 3), 0.03), torch.full((P // 4, 3), 0.12)]).to(DEV)
    quats = torch.randn(n, 4, generator=g).to(DEV)
    opac = torch.full((n,), 0.9, device=DEV)
    dc = (torch.rand(n, 1, 3, generator=g).to(DEV) - 0.5) / 0.28209479177387814
    kw = dict(extent=1.0, resolution=96, level=LEVEL, background=True, points_per_pass=300_000)
    full = extract_mesh_marching_cubes(pts, scales, quats, opac, dc, **kw)
    same = extract_mesh_marching_cubes(pts, scales, quats, opac, dc, decimation_target=None, clean=False, **kw)
    for k in ("verts", "faces", "normals", "colors"):
        assert torch.equal(full[k], same[k]), k                              # the defaults change nothing
    fg_full = extract_mesh_marching_cubes(pts, scales, quats, opac, dc, **dict(kw, background=False))
    T = 3000
    assert fg_full["faces"].shape[0] > T and full["faces"].shape[0] - fg_full["faces"].shape[0] > T
    mesh = extract_mesh_marching_cubes(pts, scales, quats, opac, dc, decimation_target=T, clean=True, **kw)
    fg = extract_mesh_marching_cubes(pts, scales, quats, opac, dc, decimation_target=T, clean=True, **dict(kw, background=False))
    V, F_ = mesh["verts"].shape[0], mesh["faces"].shape[0]
    n_fg = fg["faces"].shape[0]
    assert 0 < n_fg <= T and 0 < F_ - n_fg <= T                              # at most T faces per part
    assert torch.equal(mesh["faces"][:n_fg], fg["faces"]) and torch.equal(mesh["verts"][:fg["verts"].shape[0]], fg["verts"])
    assert mesh["normals"].shape == (V, 3) and mesh["colors"].shape == (V, 3) and int(mesh["faces"].max()) == V - 1
    assert torch.isfinite(mesh["verts"]).all() and torch.isfinite(mesh["normals"]).all()
    topo = MeshTopology.get(mesh["faces"], V)
    assert topo.n_faces == F_ and topo.n_pairs > 0
    loss = normal_consistency(mesh["verts"], mesh["faces"])
    assert torch.isfinite(loss) and 0 <= float(loss) < 1
