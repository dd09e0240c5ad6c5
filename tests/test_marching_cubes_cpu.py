"""CPU tests of the marching-cubes path (no GPU): the generated case table, the serial restatement of the kernels' rules on analytic
fields (tests/mc_restatement.py -- the GPU tests then hold the kernels to that restatement bit for bit), the mesh PLY round trip, the
`mcubes` stand-in's surface and the density-grid fixture."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mc_restatement as mcr  # noqa: E402

LEVEL = 0.3


# ------------------------------------------------------------------------------------------------ analytic fields (float64 -> float32)
def _coords(shape, spacing):
    ax = [np.arange(n, dtype=np.float64) * spacing for n in shape]
    return np.meshgrid(*ax, indexing="ij")


# centres and radii at irrational offsets: no grid value equals the level
C0 = np.array([0.5 + (np.sqrt(2.0) - 1.4) / 3, 0.5 + (np.sqrt(3.0) - 1.7) / 3, 0.5 + (np.pi - 3.1) / 3])
R0 = 0.3 + 1.0 / (np.e * 50)


def field(name, shape, spacing=None):
    """value = LEVEL + (signed distance-like function, positive inside), float32"""
    spacing = 1.0 / (max(shape) - 1) if spacing is None else spacing
    x, y, z = _coords(shape, spacing)
    if name == "sphere":
        f = R0 - np.sqrt((x - C0[0]) ** 2 + (y - C0[1]) ** 2 + (z - C0[2]) ** 2)
    elif name == "torus":
        R, r = 0.27 + np.sqrt(5.0) / 100, 0.11 + np.sqrt(7.0) / 300
        q = np.sqrt((x - C0[0]) ** 2 + (y - C0[1]) ** 2) - R
        f = r - np.sqrt(q * q + (z - C0[2]) ** 2)
    elif name == "two_spheres":
        c1, c2 = np.array([0.27 + np.sqrt(2.0) / 90, 0.3, 0.31 + np.pi / 300]), np.array([0.72, 0.69 + np.sqrt(3.0) / 80, 0.7])
        r1, r2 = 0.17 + 1 / (np.e * 40), 0.19 + np.sqrt(2.0) / 150
        f = np.maximum(r1 - np.sqrt((x - c1[0]) ** 2 + (y - c1[1]) ** 2 + (z - c1[2]) ** 2),
                       r2 - np.sqrt((x - c2[0]) ** 2 + (y - c2[1]) ** 2 + (z - c2[2]) ** 2))
    elif name == "cut_sphere":
        c = np.array([0.12 + np.sqrt(2.0) / 100, 0.45 + np.pi / 200, 0.93 + np.sqrt(3.0) / 200])
        f = (0.33 + 1 / (np.e * 30)) - np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2)
    elif name == "empty":
        f = -1.0 - 0.1 * x
    elif name == "full":
        f = 1.0 + 0.1 * x
    else:
        raise KeyError(name)
    return (LEVEL + f).astype(np.float32)


def rect_sphere():
    """a sphere in a 37 x 50 x 64 grid (one spacing for the three axes)"""
    shape, h = (37, 50, 64), 1.0 / 63
    x, y, z = _coords(shape, h)
    c = np.array([18.2 + np.sqrt(2.0) / 10, 24.6 + np.pi / 20, 31.3 + np.sqrt(3.0) / 10]) * h
    r = (14.0 + 1 / np.e) * h
    return (LEVEL + r - np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2)).astype(np.float32)


def smooth_random(n=96, seed=3):
    """a smooth random field: a few low-frequency waves with seeded phases"""
    g = np.random.default_rng(seed)
    x, y, z = _coords((n, n, n), 1.0 / (n - 1))
    f = np.zeros_like(x)
    for _ in range(12):
        k = g.uniform(-9, 9, size=3)
        f += g.uniform(0.3, 1.0) * np.sin(k[0] * x + k[1] * y + k[2] * z + g.uniform(0, 2 * np.pi))
    return (LEVEL + 0.2 * f).astype(np.float32)


def on_volume_face(verts, shape):
    v = np.asarray(verts)
    hi = np.array(shape, dtype=np.float32) - 1
    return ((v == 0) | (v == hi)).any(axis=1)


def check_vertices_on_edges(vol, iso, verts, aux):
    """every vertex lies on the grid edge the restatement names, between its ends, and the linear interpolant there equals iso within
    4 ulp of the largest of |a|, |b|, |iso|: t carries the rounding of two subtractions and a division (<= 1.5 ulp relative), the
    product t (b - a) adds 1, the sum a + . adds 0.5 at the scale of its operands -- under 4 ulp at the largest magnitude involved."""
    nx, ny, nz = vol.shape
    p, a, t = aux["owner"], aux["axis"], aux["t"]
    strides = np.array([ny * nz, nz, 1])
    flat = vol.reshape(-1).astype(np.float64)
    coords = np.stack([p // (ny * nz), (p // nz) % ny, p % nz], axis=1)
    for ax in range(3):
        m = a == ax
        other = [k for k in range(3) if k != ax]
        assert (verts[m][:, other] == coords[m][:, other]).all()
        along = verts[m][:, ax]
        assert ((along >= coords[m][:, ax]) & (along <= coords[m][:, ax] + 1)).all()
    va, vb = flat[p], flat[p + strides[a]]
    lo_in = np.isfinite(va) & (va >= iso)
    out_v, in_v = np.where(lo_in, vb, va), np.where(lo_in, va, vb)
    ok = np.isfinite(out_v)
    assert (out_v[ok] < iso).all() and (in_v >= iso).all()
    interp = out_v[ok] + t[ok].astype(np.float64) * (in_v[ok] - out_v[ok])
    scale = np.maximum(np.maximum(np.abs(out_v[ok]), np.abs(in_v[ok])), abs(iso)).astype(np.float32)
    err = np.abs(interp - np.float64(np.float32(iso)))
    assert (err <= 4 * np.spacing(scale).astype(np.float64)).all(), float((err / np.spacing(scale)).max())
    assert (t[~ok] == 0.5).all()


# ------------------------------------------------------------------------------------------------ 1. the table
def _generator():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        return importlib.import_module("gen_mc_table")
    finally:
        sys.path.pop(0)


def test_committed_table_is_the_generators_output():
    gen = _generator()
    assert open(mcr.TABLE_PATH).read() == gen.generate()


def test_table_consistency():
    gen = _generator()
    max_tris, owner, ntri, tri = mcr.load_table()
    assert max_tris == tri.shape[1] // 3 and list(owner) == [gen.edge_corners(e)[0] for e in range(12)]
    face_sets = {}
    for case in range(256):
        row = tri[case]
        n = int(ntri[case])
        assert (row[:3 * n] >= 0).all() and (row[3 * n:] == -1).all()
        tris = row[:3 * n].reshape(n, 3)
        # every crossed edge is used and no uncrossed edge is
        crossed = {e for e in range(12) if ((case >> gen.edge_corners(e)[0]) & 1) != ((case >> gen.edge_corners(e)[1]) & 1)}
        assert set(tris.reshape(-1).tolist()) == crossed, case
        # consistent winding: no directed edge twice; an edge used twice is used once in each direction
        directed = [(int(t[k]), int(t[(k + 1) % 3])) for t in tris for k in range(3)]
        assert len(set(directed)) == len(directed), case
        boundary = [(a, b) for (a, b) in directed if (b, a) not in directed]
        # the boundary of the case's patches lies on the cell faces: one directed segment per face crossing
        per_face = {k: set() for k in range(6)}
        for a, b in boundary:
            on = [k for k, (_, cyc) in enumerate(gen.FACES) if set(gen.edge_corners(a)) | set(gen.edge_corners(b)) <= set(cyc)]
            assert len(on) == 1, (case, a, b)
            per_face[on[0]].add((a, b))
        for k, (normal, cyc) in enumerate(gen.FACES):
            axis = [i for i in range(3) if normal[i]][0]
            signs = tuple((case >> c) & 1 for c in cyc)
            n_cross = sum(signs[i] != signs[(i + 1) % 4] for i in range(4))
            assert len(per_face[k]) == n_cross // 2, (case, k)
            # in face-local terms (the face's axis dropped) the segments depend on the four signs alone
            local = lambda e: frozenset(tuple(v for i, v in enumerate(gen.corner_offset(c)) if i != axis) for c in gen.edge_corners(e))
            segs = frozenset((local(a), local(b)) for a, b in per_face[k])
            key = (k, signs)
            assert face_sets.setdefault(key, segs) == segs, (case, k)
    # the two cells sharing a face see the same signs: the same segments, traversed in opposite directions
    for axis in range(3):
        lo, hi = 2 * axis, 2 * axis + 1
        for signs in {s for (k, s) in face_sets if k == lo}:
            a, b = face_sets[(lo, signs)], face_sets[(hi, signs)]
            assert a == frozenset((y, x) for (x, y) in b), (axis, signs)
    assert len(face_sets) == 6 * 16


# ------------------------------------------------------------------------------------------------ 2. the restatement on analytic fields
CLOSED = {"sphere": 2, "torus": 0, "two_spheres": 4}


@pytest.mark.parametrize("n", [32, 64])
@pytest.mark.parametrize("name", sorted(CLOSED))
def test_restatement_closed_fields(name, n):
    vol = field(name, (n, n, n))
    assert not (vol == np.float32(LEVEL)).any()
    verts, faces, aux = mcr.marching_cubes(vol, LEVEL)
    assert len(verts) and len(faces) and np.isfinite(verts).all()
    closed, boundary, no_repeat = mcr.edge_report(faces, len(verts))
    assert closed and no_repeat and len(boundary) == 0
    assert mcr.euler_characteristic(faces, len(verts)) == CLOSED[name]
    volume, area = mcr.signed_volume_and_area(verts, faces)
    assert volume > 0 and area > 0
    check_vertices_on_edges(vol, LEVEL, verts, aux)
    assert sorted(np.unique(faces)) == list(range(len(verts)))       # every vertex is used: welded, none orphaned


@pytest.mark.parametrize("n", [32, 64])
def test_restatement_cut_sphere(n):
    vol = field("cut_sphere", (n, n, n))
    verts, faces, aux = mcr.marching_cubes(vol, LEVEL)
    closed, boundary, no_repeat = mcr.edge_report(faces, len(verts))
    assert no_repeat and not closed and len(boundary)
    # boundary edges lie on the volume's faces only
    assert on_volume_face(verts[boundary[:, 0]], vol.shape).all() and on_volume_face(verts[boundary[:, 1]], vol.shape).all()
    check_vertices_on_edges(vol, LEVEL, verts, aux)


@pytest.mark.parametrize("name", ["empty", "full"])
def test_restatement_empty_and_full(name):
    verts, faces, _ = mcr.marching_cubes(field(name, (32, 32, 32)), LEVEL)
    assert verts.shape == (0, 3) and faces.shape == (0, 3)


def test_restatement_rectangular_grid():
    vol = rect_sphere()
    assert vol.shape == (37, 50, 64)
    verts, faces, aux = mcr.marching_cubes(vol, LEVEL)
    closed, boundary, no_repeat = mcr.edge_report(faces, len(verts))
    assert closed and no_repeat
    assert mcr.euler_characteristic(faces, len(verts)) == 2
    assert mcr.signed_volume_and_area(verts, faces)[0] > 0
    check_vertices_on_edges(vol, LEVEL, verts, aux)


def test_restatement_non_finite_values_are_outside():
    vol = field("sphere", (24, 24, 24))
    g = np.random.default_rng(0)
    idx = g.integers(0, 24, size=(60, 3))
    for k, (i, j, l) in enumerate(idx):
        vol[i, j, l] = (np.nan, np.inf, -np.inf)[k % 3]
    verts, faces, aux = mcr.marching_cubes(vol, LEVEL)
    assert np.isfinite(verts).all() and len(faces)
    assert faces.min() >= 0 and faces.max() < len(verts)
    check_vertices_on_edges(vol, LEVEL, verts, aux)
    assert (aux["t"] == 0.5).any()


def test_sphere_volume_and_area_converge_at_second_order():
    """the enclosed volume and the area of the sphere against 4 pi r^3 / 3 and 4 pi r^2: the errors fall by at least 3x from 32^3 to 64^3
    (second order gives 4x)"""
    errs = {}
    for n in (32, 64):
        verts, faces, _ = mcr.marching_cubes(field("sphere", (n, n, n)), LEVEL)
        volume, area = mcr.signed_volume_and_area(verts.astype(np.float64) / (n - 1), faces)
        errs[n] = (abs(volume - 4 * np.pi * R0 ** 3 / 3), abs(area - 4 * np.pi * R0 ** 2))
        print(f"n={n}: volume error {errs[n][0]:.3e}, area error {errs[n][1]:.3e}")
    assert errs[32][0] / errs[64][0] >= 3.0, errs
    assert errs[32][1] / errs[64][1] >= 3.0, errs


# ------------------------------------------------------------------------------------------------ 3. PLY, stand-in surface, CPU refusals
def test_mesh_ply_round_trip(tmp_path):
    from sugar_amd import io
    verts, faces, _ = mcr.marching_cubes(field("torus", (24, 24, 24)), LEVEL)
    g = np.random.default_rng(1)
    normals = g.standard_normal(verts.shape).astype(np.float32)
    colors = g.integers(0, 256, size=verts.shape, dtype=np.uint8)
    path = str(tmp_path / "sub" / "mesh.ply")
    io.save_mesh_ply(path, torch.from_numpy(verts), torch.from_numpy(faces), normals=normals, colors=colors)
    head = open(path, "rb").read(400)
    assert head.startswith(b"ply\nformat binary_little_endian 1.0\n") and b"property list uchar int vertex_indices" in head
    m = io.load_mesh_ply(path)
    assert m["verts"].dtype == torch.float32 and m["faces"].dtype == torch.int64 and m["colors"].dtype == torch.uint8
    assert np.array_equal(m["verts"].numpy().view(np.uint32), verts.view(np.uint32))
    assert np.array_equal(m["faces"].numpy(), faces)
    assert np.array_equal(m["normals"].numpy().view(np.uint32), normals.view(np.uint32))
    assert np.array_equal(m["colors"].numpy(), colors)
    # float colours: clamped RGB in [0, 1] on 255 steps; missing normals / colours: zeros; an empty mesh round-trips
    io.save_mesh_ply(path, verts, faces, colors=np.full(verts.shape, 2.0, np.float32))
    m = io.load_mesh_ply(path)
    assert (m["colors"] == 255).all() and (m["normals"] == 0).all()
    io.save_mesh_ply(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64))
    m = io.load_mesh_ply(path)
    assert m["verts"].shape == (0, 3) and m["faces"].shape == (0, 3)
    with pytest.raises(ValueError, match="outside"):
        io.save_mesh_ply(path, verts, faces + len(verts))


def test_mcubes_stand_in_surface():
    from sugar_amd import shims
    shims.install()
    import mcubes
    assert os.path.abspath(mcubes.__file__).startswith(os.path.join(ROOT, "sugar_amd", "shims")) or hasattr(mcubes, "marching_cubes")
    assert callable(mcubes.marching_cubes)
    if os.path.abspath(mcubes.__file__).startswith(os.path.join(ROOT, "sugar_amd", "shims")):
        assert mcubes.__all__ == ["marching_cubes"]
        with pytest.raises(ValueError, match="3-D"):
            mcubes.marching_cubes(np.zeros((4, 4), np.float32), 0.5)
        with pytest.raises(ValueError, match="finite"):
            mcubes.marching_cubes(np.zeros((4, 4, 4), np.float32), float("nan"))
        with pytest.raises(TypeError):
            mcubes.marching_cubes(np.zeros((4, 4, 4), dtype=object), 0.5)
        if not torch.cuda.is_available():
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                mcubes.marching_cubes(np.zeros((4, 4, 4), np.float32), 0.5)
    # no open3d stand-in is offered
    assert not os.path.exists(os.path.join(ROOT, "sugar_amd", "shims", "open3d"))


def test_cpu_tensors_are_refused():
    from sugar_amd import extract, marching_cubes as mc
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mc.marching_cubes(torch.zeros(4, 4, 4), 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mc.vertex_normals(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        extract.density_grid(torch.zeros(4), torch.zeros(4), torch.zeros(4), torch.zeros(8, 3), torch.zeros(8, 3, 3), torch.zeros(8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        extract.extract_mesh_marching_cubes(torch.zeros(8, 3), torch.ones(8, 3), torch.ones(8, 4), torch.ones(8), torch.zeros(8, 3), 1.0)


def test_abi_refuses_grids_of_2_to_31_points(hip_lib):
    L = hip_lib
    assert L.sgr_marching_cubes_scratch_bytes(2048, 1024, 1024) == 0
    assert L.sgr_marching_cubes_scratch_bytes(0, 4, 4) == 0
    n = L.sgr_marching_cubes_scratch_bytes(512, 512, 512)
    assert 2 * 512 ** 3 < n < 2.5 * 512 ** 3 and n % 256 == 0
    assert L.sgr_marching_cubes_count(2048, 1024, 1024, None, 0.5, None, None, None) == -1     # refused before any pointer is read
    assert L.sgr_marching_cubes_emit(2048, 1024, 1024, None, 0.5, None, 0, 0, None, None, None) == -1
    assert L.sgr_grid_points(2048, 1024, 1024, None, None, None, 0, 0, None, None) == -1
    assert b"2^31" in L.sgr_last_error()


# ------------------------------------------------------------------------------------------------ 4. the density-grid fixture
def test_density_grid_fixture_matches_its_maker():
    """tests/golden/sugar_mcgrid.npz is what tests/golden/make_sugar_mcgrid.py computes with the reference's own SuGaR.compute_density
    (re-run where the reference tree is present)"""
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    try:
        import make_sugar_callsite as mk
        if not os.path.isdir(mk.REF):
            pytest.skip("the reference tree is not present")
        import make_sugar_mcgrid
        out = make_sugar_mcgrid.run()
    finally:
        sys.path.pop(0)
    gold = np.load(os.path.join(ROOT, "tests", "golden", "sugar_mcgrid.npz"))
    assert sorted(gold.files) == sorted(out)
    for k in gold.files:
        a, b = gold[k], np.asarray(out[k])
        assert a.shape == b.shape and a.dtype == b.dtype, k
        if a.dtype.kind == "f":
            np.testing.assert_allclose(b, a, rtol=2e-5, atol=1e-7, err_msg=k)
        else:
            assert np.array_equal(a, b), k
