"""GPU tests of the refined-mesh postprocess (csrc/mesh_postprocess.hip via sugar_amd.mesh_postprocess), the 2-D `knn_points` and the
command `python -m sugar_amd.refined_mesh`, against the numpy restatement of tests/mesh_postprocess_restatement.py (whose rule
tests/test_mesh_postprocess_cpu.py pins) and against the reference's own k-NN formulation run on the device.  The reference is never
imported here."""
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
import mesh_postprocess_restatement as mpr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ITERATIONS = (0, 1, 2, 5, 9)

# the smallest shapes at which the kernels can go wrong
PEEL_CASES = {
    "sheet7x5+extras": lambda: mpr.with_extras(mpr.sheet(7, 5)),       # 74 faces: below one wave; reaches its fixed point (the pair)
    "sheet41x30+extras": lambda: mpr.with_extras(mpr.sheet(41, 30)),   # 2 464 faces: no multiple of 64 or 256, several workgroups
    "sheet300x251": lambda: mpr.sheet_fast(300, 251),                  # 150 600 faces, 226 451 edges, several iterations deep
    "octahedron": lambda: mpr.octahedron(2)[1],                        # closed: loses nothing
    "sheet7x5": lambda: mpr.sheet(7, 5),                               # empty from iteration 5 on, run to 9
}


@functools.lru_cache(maxsize=None)
def _faces(name):
    return PEEL_CASES[name]()


@functools.lru_cache(maxsize=None)
def _expected(name, masked):
    """the restatement's masks after 0 .. 9 steps, computed once per case (the large sheet with the numpy counting, which the CPU
    tests hold against the serial loop)"""
    faces = _faces(name)
    return mpr.peel_steps(faces, max(ITERATIONS), mpr.initial_mask(len(faces)) if masked else None, serial=len(faces) < 10_000)


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


@pytest.mark.parametrize("it", ITERATIONS)
@pytest.mark.parametrize("name", list(PEEL_CASES))
def test_peel_is_the_restatement_byte_for_byte(hip_lib, name, it):
    from sugar_amd.mesh_postprocess import PeelTopology, peel_border_faces
    faces = _faces(name)
    f64, f32 = _dev(faces), _dev(faces, torch.int32)
    want = _expected(name, False)[it]
    got = peel_border_faces(f64, it)
    assert got.dtype == torch.bool and got.shape == (len(faces),)
    assert np.array_equal(got.cpu().numpy(), want), (name, it, int(got.sum()), int(want.sum()))
    assert torch.equal(peel_border_faces(f32, it), got)                              # int32 faces
    assert torch.equal(peel_border_faces(f64, it), got)                              # a second run
    topo = PeelTopology(f64, int(faces.max()) + 5)                                   # unreferenced vertices change nothing
    assert torch.equal(peel_border_faces(f64, it, topology=topo), got)
    m0 = mpr.initial_mask(len(faces))
    got_m = peel_border_faces(f64, it, face_mask=_dev(m0))
    assert np.array_equal(got_m.cpu().numpy(), _expected(name, True)[it]), (name, it, "masked")
    assert torch.equal(peel_border_faces(f32, it, face_mask=_dev(m0), topology=topo), got_m)


def test_peel_fixed_points(hip_lib):
    from sugar_amd.mesh_postprocess import peel_border_faces
    assert peel_border_faces(_dev(_faces("octahedron")), 9).all()
    assert peel_border_faces(_dev(_faces("sheet7x5+extras")), 9).nonzero().reshape(-1).tolist() == [71, 72]
    empty = peel_border_faces(_dev(_faces("sheet7x5")), 5)
    assert not empty.any()
    assert not peel_border_faces(_dev(_faces("sheet7x5")), 4, face_mask=empty).any()      # an empty set stays empty
    none = torch.zeros(0, 3, dtype=torch.int64, device=DEV)
    assert peel_border_faces(none, 3).shape == (0,)                                        # no face: nothing is launched


@pytest.mark.parametrize("name", ["sheet7x5+extras", "sheet41x30+extras"])
def test_peel_equals_the_reference_formulation_on_the_device(hip_lib, name):
    """refined_mesh.py:133-147 as written, through the 2-D `knn_points`: 222 points take the exhaustive kernel, 7 392 the grid"""
    from sugar_amd.knn import GRID_THRESHOLD, knn_points
    from sugar_amd.mesh_postprocess import peel_border_faces
    new_faces = _dev(_faces(name))
    assert (3 * len(new_faces) >= GRID_THRESHOLD) == (name == "sheet41x30+extras")
    edges0 = new_faces[..., None, (0, 1)].sort(dim=-1)[0]
    edges1 = new_faces[..., None, (1, 2)].sort(dim=-1)[0]
    edges2 = new_faces[..., None, (2, 0)].sort(dim=-1)[0]
    all_edges = torch.cat([edges0, edges1, edges2], dim=-2)
    face_mask = torch.ones(len(new_faces), dtype=torch.bool, device=DEV)
    for i in range(5):
        pts = all_edges[face_mask].view(1, -1, 2).float()
        edges_neighbors = knn_points(pts, pts, K=2)
        is_inside = (edges_neighbors.dists[0][..., 1].view(-1, 3) < 0.01).all(-1)
        face_mask[face_mask.clone()] = is_inside
        assert face_mask.any()
        assert torch.equal(face_mask, peel_border_faces(new_faces, i + 1)), (name, i)


def _brute_knn(p, K):
    p64 = p.astype(np.float64)
    d = ((p64[:, None, :] - p64[None, :, :]) ** 2).sum(-1)
    idx = np.argsort(d, axis=1, kind="stable")[:, :K]
    return np.take_along_axis(d, idx, 1), idx, d


@pytest.mark.parametrize("N", [5000, 3000])
def test_knn_points_2d(hip_lib, N):
    """N = 5 000 takes the grid kernels (>= GRID_THRESHOLD), 3 000 the exhaustive one.  Distances: a float32 (dx dx + dy dy) + 0 of
    float32 differences carries at most 4 roundings, 4 * 2^-24 < 1e-6 relative.  Indices equal the float64 brute force's wherever
    float64 tells the candidates apart; where two candidates lie within that rounding of each other either is right."""
    from sugar_amd.knn import GRID_THRESHOLD, knn_points
    assert (N >= GRID_THRESHOLD) == (N == 5000)
    p = np.random.default_rng(N).uniform(0, 1, (N, 2)).astype(np.float32)
    ref_d, ref_i, full = _brute_knn(p, 16)
    t = _dev(p)[None]
    for K in (1, 2, 16):
        out = knn_points(t, t, K=K, return_nn=True)
        d, i = out.dists[0].cpu().numpy(), out.idx[0].cpu().numpy()
        assert d.shape == (N, K) and i.shape == (N, K) and i.dtype == np.int64
        assert np.allclose(d, ref_d[:, :K], rtol=1e-6, atol=0)
        same = i == ref_i[:, :K]
        assert same.mean() >= 0.999
        assert np.allclose(np.take_along_axis(full, i, 1)[~same], ref_d[:, :K][~same], rtol=1e-6, atol=0)
        assert out.knn.shape == (1, N, K, 2) and torch.equal(out.knn[0], t[0][out.idx[0]])
    other = _dev(np.random.default_rng(1).uniform(0, 1, (70, 2)).astype(np.float32))[None]      # p1 is not p2
    o = knn_points(other, t, K=3)
    od = ((other[0].cpu().numpy().astype(np.float64)[:, None] - p.astype(np.float64)[None]) ** 2).sum(-1)
    assert np.allclose(o.dists[0].cpu().numpy(), np.sort(od, 1)[:, :3], rtol=1e-6, atol=0)
    with pytest.raises(RuntimeError, match="expected"):
        knn_points(torch.zeros(1, N, 4, device=DEV), torch.zeros(1, N, 4, device=DEV), K=1)
    with pytest.raises(RuntimeError, match="expected"):
        knn_points(t, torch.zeros(1, N, 3, device=DEV), K=1)                                    # mixed dimensions


def test_readd_equals_the_restatement(hip_lib):
    """the case tests/test_mesh_postprocess_cpu.py shows to be decidable in float32 (every dead face's density is 1e-3 off the threshold)"""
    from sugar_amd.mesh_postprocess import readd_dense_faces
    c = mpr.readd_case()
    dens = mpr.face_density(c["verts"], c["faces"], c["points"], c["scaling"], c["quaternions"], c["strengths"])
    want = mpr.readd(c["mask"], dens, c["threshold"])
    args = [_dev(c[k]) for k in ("verts", "faces", "mask", "points", "scaling", "quaternions", "strengths")]
    got = readd_dense_faces(*args, c["threshold"])
    assert np.array_equal(got.cpu().numpy(), want)
    assert (want & ~c["mask"]).any() and (~want).any()
    assert np.array_equal(args[2].cpu().numpy(), c["mask"])                          # the mask handed in is not written
    # no dead face: the mask comes back unchanged
    full = torch.ones(len(c["faces"]), dtype=torch.bool, device=DEV)
    assert torch.equal(readd_dense_faces(args[0], args[1], full, *args[3:], c["threshold"]), full)


def _bound_gaussians(sd, n):
    """the Gaussians of a bound model in plain torch on the host (sugar_amd.synthetic.bound_gaussians, not the HIP binding)"""
    from sugar_amd import synthetic as syn
    t = lambda k: torch.from_numpy(np.asarray(sd[k]))
    means, scaling, quats = syn.bound_gaussians(t("_points"), t("_surface_mesh_faces"), torch.exp(t("_scales")), t("_quaternions"),
                                                float(sd["surface_mesh_thickness"]), n)
    strengths = 1.0 / (1.0 + np.exp(-sd["all_densities"].reshape(-1).astype(np.float64)))
    return means.numpy(), scaling.numpy(), quats.numpy(), strengths


def _restated_postprocess(sd, n, iterations=5, threshold=0.1):
    faces = sd["_surface_mesh_faces"]
    means, scaling, quats, strengths = _bound_gaussians(sd, n)
    dens = mpr.face_density(sd["_points"], faces, means, scaling, quats, strengths)
    mask = mpr.peel(faces, iterations)
    assert mpr.margin_ok(mask, dens, threshold)                  # the case is decidable in float32, no face exempted
    out = mpr.readd(mask, dens, threshold)
    assert (out & ~mask).any() and (~out).any()                  # some border faces come back, some stay out
    return out


@pytest.mark.parametrize("n", [1, 6])
def test_postprocess_bound_mesh(hip_lib, n):
    from sugar_amd.mesh_postprocess import postprocess_bound_mesh
    sd = mpr.bound_case(12, 9, n, seed=3)
    want = _restated_postprocess(sd, n)
    d = {k: _dev(v) for k, v in sd.items()}
    verts_before = d["_points"].clone()
    r = postprocess_bound_mesh(d["_points"], d["_surface_mesh_faces"], n, d["_scales"], d["_quaternions"], d["all_densities"],
                               d["surface_mesh_thickness"], d["_sh_coordinates_dc"], d["_sh_coordinates_rest"])
    assert np.array_equal(r.face_mask.cpu().numpy(), want)
    assert np.array_equal(r.faces.cpu().numpy(), sd["_surface_mesh_faces"][want])
    assert len(r.per_gaussian) == 5
    for got, key in zip(r.per_gaussian, ("_scales", "_quaternions", "all_densities", "_sh_coordinates_dc", "_sh_coordinates_rest")):
        assert np.array_equal(got.cpu().numpy(), mpr.compact_rows(sd[key], want, n)), key
    assert torch.equal(d["_points"], verts_before)


def _camera_json(i, cam):
    from sugar_amd import io
    w2c = cam.viewmatrix.cpu().numpy().T.astype(np.float64)
    fov_x, fov_y = 2 * math.atan(cam.tanfovx), 2 * math.atan(cam.tanfovy)
    return io.camera_to_json(i, f"view_{i:03d}", w2c[:3, :3].T, w2c[:3, 3], fov_x, fov_y, cam.image_width, cam.image_height)


def test_command_line_end_to_end(hip_lib, tmp_path, capsys):
    """a synthetic checkpoint in the reference's layout (a 12 x 9 sheet, n = 1), two 64 x 48 cameras that see it, square size 4:
    without and with --postprocess"""
    from sugar_amd import synthetic as syn
    from sugar_amd import texture
    from sugar_amd.mesh_render import load_textured_obj
    from sugar_amd.refined_mesh import main
    sd = mpr.bound_case(12, 9, 1, seed=3)
    kept = _restated_postprocess(sd, 1)
    faces = sd["_surface_mesh_faces"]
    ck = tmp_path / "refined.pt"
    torch.save({"epoch": 15000, "state_dict": {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}}, ck)
    cams = [syn.look_at_camera((6.0, -2.0, 13.0), (6.0, 4.5, 0.0), 64, 48), syn.look_at_camera((1.0, 9.0, 12.0), (6.0, 4.5, 0.0), 64, 48)]
    cj = tmp_path / "cameras.json"
    cj.write_text(json.dumps([_camera_json(i, c) for i, c in enumerate(cams)]))
    for flags, want_faces in (([], faces), (["--postprocess"], faces[kept])):
        out = tmp_path / ("mesh" + "_post" * bool(flags) + ".obj")
        assert main([str(ck), "--cameras", str(cj), "--out", str(out), "--square-size", "4", *flags]) == 0
        line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        T = len(want_faces)
        assert (line["faces_before"], line["faces_after"], line["views_baked"], line["gaussians_per_triangle"]) == (len(faces), T, 2, 1)
        assert line["texture_side"] == texture.texture_size(T, 4) and set(line["seconds"]) >= {"load", "bind", "bake", "save"}
        verts, f, verts_uvs, faces_uvs, tex = load_textured_obj(str(out), DEV)
        assert np.array_equal(f.cpu().numpy(), want_faces)
        assert verts.shape == sd["_points"].shape and np.allclose(verts.cpu().numpy(), sd["_points"], atol=2e-6)   # "%f": 6 decimals, read back as float32
        uv, fuv = texture.uv_layout(T, 4, DEV)
        assert torch.equal(faces_uvs, fuv) and np.allclose(verts_uvs.cpu().numpy(), uv.cpu().numpy(), atol=1e-6)
        S = texture.texture_size(T, 4)
        assert tuple(tex.shape) == (S, S, 3)
        assert bool(torch.isfinite(tex).all()) and float(tex.min()) >= 0.0 and float(tex.max()) <= 1.0
        # a baker that baked no view gives the init image: the written texture differs from it, so the views were baked
        d = {k: _dev(v) for k, v in sd.items()}
        means, scaling, quats, _ = _bound_gaussians(sd, 1)
        sel = np.ones(len(faces), bool) if not flags else kept
        from sugar_amd.field import scaled_rotation
        M = scaled_rotation(_dev(quats[sel]), _dev(scaling[sel]), inverse_scales=True)
        init = texture.TextureBaker(d["_points"], _dev(want_faces), _dev(means[sel]), M, d["_sh_coordinates_dc"][_dev(sel), 0], 1, 4)
        init_img = (init.result().clamp(0, 1) * 255.0).to(torch.uint8).float() / 255.0           # what save_obj would have written
        assert int((tex != init_img).any(-1).sum()) > 50
    with pytest.raises(ValueError, match="one image size"):
        cj.write_text(json.dumps([_camera_json(0, cams[0]), _camera_json(1, syn.look_at_camera((1.0, 9.0, 12.0), (6.0, 4.5, 0.0), 48, 48))]))
        main([str(ck), "--cameras", str(cj), "--out", str(tmp_path / "x.obj"), "--square-size", "4"])
