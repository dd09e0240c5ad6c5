"""CPU tests of the mesh decimation and cleaning (no GPU): the serial restatement tests/decimate_restatement.py on the marching-cubes
meshes of the analytic fields of tests/test_marching_cubes_cpu.py -- the n = 64 mesh of a field decimated to the face count of its
n = 32 mesh -- the cleaning rules on hand-built meshes, the ABI surface and the CPU refusals.  The GPU tests then hold the kernels to
the restatement bit for bit."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decimate_restatement as dr  # noqa: E402
import mc_restatement as mcr  # noqa: E402
import test_marching_cubes_cpu as cpu  # noqa: E402

LEVEL = cpu.LEVEL
FIELDS = ["sphere", "torus", "two_spheres", "cut_sphere"]
FACES = {32: dict(sphere=3408, torus=3708, two_spheres=2608, cut_sphere=1672),
         64: dict(sphere=14120, torus=15784, two_spheres=10800, cut_sphere=6888)}
EULER = dict(sphere=2, torus=0, two_spheres=4, cut_sphere=1)
COMPONENTS = dict(sphere=1, torus=1, two_spheres=2, cut_sphere=1)
# E(decimated) / E(direct n = 32 mesh) measured on the restatement: the bar is max(1.0, 1.25 x measured)
MEASURED_RATIO = dict(sphere=0.643, torus=0.463)


@functools.lru_cache(maxsize=None)
def mc_mesh(name, n):
    """the marching-cubes mesh of a field in the unit cube: (verts float32 [V,3], faces int64 [F,3])"""
    v, f, _ = mcr.marching_cubes(cpu.field(name, (n, n, n)), LEVEL)
    return (v / np.float32(n - 1)).astype(np.float32), f


@functools.lru_cache(maxsize=None)
def decimated(name):
    v, f = mc_mesh(name, 64)
    return dr.decimate(v, f, FACES[32][name])


def signed_distance(name, p):
    """the exact signed distance of the sphere and torus fields (positive inside)"""
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    c = cpu.C0
    if name == "sphere":
        return cpu.R0 - np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2)
    R, r = 0.27 + np.sqrt(5.0) / 100, 0.11 + np.sqrt(7.0) / 300
    q = np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2) - R
    return r - np.sqrt(q * q + (z - c[2]) ** 2)


def surface_error(name, verts, faces):
    """E(mesh): the largest |f| over the vertices and the face centroids"""
    v = np.asarray(verts, dtype=np.float64)
    cen = (v[faces[:, 0]] + v[faces[:, 1]] + v[faces[:, 2]]) / 3.0
    return max(float(np.abs(signed_distance(name, v)).max()), float(np.abs(signed_distance(name, cen)).max()))


def components(faces, n_verts):
    parent = np.arange(n_verts)

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for a, b, c in np.asarray(faces):
        for x, y in ((a, b), (b, c)):
            rx, ry = find(x), find(y)
            if rx != ry:
                parent[rx] = ry
    return len({find(v) for v in np.unique(faces)})


def boundary_loops(boundary):
    """the number of closed loops the directed boundary edges form"""
    nxt = {int(a): int(b) for a, b in boundary}
    assert len(nxt) == len(boundary)
    seen, loops = set(), 0
    for start in nxt:
        if start in seen:
            continue
        loops += 1
        v = start
        while v not in seen:
            seen.add(v)
            v = nxt[v]
    return loops


def outward(name, p):
    """the analytic outward direction (the negated gradient of the field) at the points p"""
    c = cpu.C0
    if name == "sphere":
        return p - c
    if name == "cut_sphere":
        return p - np.array([0.12 + np.sqrt(2.0) / 100, 0.45 + np.pi / 200, 0.93 + np.sqrt(3.0) / 200])
    if name == "torus":
        R = 0.27 + np.sqrt(5.0) / 100
        d = p[:, :2] - c[:2]
        ring = c[:2] + R * d / np.linalg.norm(d, axis=1, keepdims=True)
        return p - np.concatenate([ring, np.full((len(p), 1), c[2])], axis=1)
    c1, c2 = np.array([0.27 + np.sqrt(2.0) / 90, 0.3, 0.31 + np.pi / 300]), np.array([0.72, 0.69 + np.sqrt(3.0) / 80, 0.7])
    near1 = np.linalg.norm(p - c1, axis=1) < np.linalg.norm(p - c2, axis=1)
    return np.where(near1[:, None], p - c1, p - c2)


# ------------------------------------------------------------------------------------------------ the inputs are what the issue counted
@pytest.mark.parametrize("name", FIELDS)
def test_input_meshes(name):
    for n in (32, 64):
        v, f = mc_mesh(name, n)
        assert len(f) == FACES[n][name]
        assert mcr.euler_characteristic(f, len(v)) == EULER[name]
    v, f = mc_mesh(name, 64)
    closed, boundary, no_repeat = mcr.edge_report(f, len(v))
    assert no_repeat and closed == (name != "cut_sphere")
    if name == "cut_sphere":
        assert len(boundary) == 192


# ------------------------------------------------------------------------------------------------ the restatement, 64^3 -> the 32^3 count
@pytest.mark.parametrize("name", FIELDS)
def test_face_count_rounds_and_topology(name):
    v, f, info = decimated(name)
    target = FACES[32][name]
    print(name, info)
    assert target - 2 < len(f) <= target and info["faces"] == len(f) and info["target_met"]
    assert 0 < info["rounds"] <= info["round_limit"] == dr.round_limit(FACES[64][name], target) == 8 * 3 + 32
    assert v.dtype == np.float32 and f.dtype == np.int64 and np.isfinite(v).all()
    assert sorted(np.unique(f)) == list(range(len(v)))
    assert mcr.euler_characteristic(f, len(v)) == EULER[name]
    v_in, f_in = mc_mesh(name, 64)
    assert components(f, len(v)) == COMPONENTS[name] == components(f_in, len(v_in))
    closed, boundary, no_repeat = mcr.edge_report(f, len(v))
    assert no_repeat
    if name == "cut_sphere":
        assert not closed and boundary_loops(boundary) == 1
        # the boundary quadric keeps the rim on the domain's boundary planes (the sphere is cut by x = 0 and by z = 1)
        rim = v[np.unique(boundary)].astype(np.float64)
        assert (np.minimum(np.abs(rim[:, 0]), np.abs(rim[:, 2] - 1.0)) <= 1.5 / 63).all()
    else:
        assert closed and len(boundary) == 0                     # every edge has exactly two faces, once in each direction


@pytest.mark.parametrize("name", FIELDS)
def test_no_face_points_inwards(name):
    v, f, _ = decimated(name)
    p = v.astype(np.float64)
    n = np.cross(p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]])
    cen = (p[f[:, 0]] + p[f[:, 1]] + p[f[:, 2]]) / 3.0
    assert (np.einsum("ij,ij->i", n, outward(name, cen)) > 0).all()


@pytest.mark.parametrize("name", ["sphere", "torus"])
def test_accuracy_against_the_direct_mesh_of_the_same_budget(name):
    """the yardstick is merged code: E of the marching-cubes mesh extracted directly at n = 32, the same face budget placed uniformly"""
    v, f, _ = decimated(name)
    e_dec, e_yard = surface_error(name, v, f), surface_error(name, *mc_mesh(name, 32))
    ratio = e_dec / e_yard
    print(f"{name}: E(decimated) {e_dec:.4e}, E(direct 32^3) {e_yard:.4e}, ratio {ratio:.3f} (measured {MEASURED_RATIO[name]})")
    assert MEASURED_RATIO[name] <= 2.0
    assert ratio <= max(1.0, 1.25 * MEASURED_RATIO[name])


def test_restatement_is_deterministic():
    a, b = dr.decimate(*mc_mesh("cut_sphere", 64), 1672), decimated("cut_sphere")
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1])


def test_a_target_of_at_least_the_face_count_returns_the_input():
    v, f = mc_mesh("sphere", 32)
    for target in (len(f), len(f) + 5):
        v2, f2, info = dr.decimate(v, f, target)
        assert np.array_equal(v2.view(np.uint32), v.view(np.uint32)) and np.array_equal(f2, f)
        assert info["rounds"] == 0 and info["target_met"]


def tetrahedron():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float32)
    f = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], dtype=np.int64)
    return v, f


def test_a_tetrahedron_cannot_be_decimated():
    v, f, info = dr.decimate(*tetrahedron(), 0)
    assert not info["target_met"] and info["faces"] == len(f) == 4 and info["rounds"] == 1


# ------------------------------------------------------------------------------------------------ cleaning
def hand_built_meshes():
    """four meshes of at most 12 faces: one degenerate face; one duplicated face in a rotated vertex order; two bit-equal vertices;
    one edge with three faces"""
    quad = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [2, 0.5, 0]], dtype=np.float32)
    degenerate = (quad, np.array([[0, 1, 2], [0, 2, 3], [1, 4, 4], [1, 4, 2]], dtype=np.int64))
    duplicated = (quad, np.array([[0, 1, 2], [0, 2, 3], [1, 4, 2], [2, 0, 1]], dtype=np.int64))
    twin = np.concatenate([quad, quad[2:3]])                                 # vertex 5 is bit-equal to vertex 2
    twins = (twin, np.array([[0, 1, 2], [0, 2, 3], [1, 4, 5]], dtype=np.int64))
    fin = np.array([[0, 0, 0], [1, 0, 0], [0.5, 1, 0], [0.5, -1, 0], [0.5, 0, 0.25], [3, 3, 3]], dtype=np.float32)
    three = (fin, np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], dtype=np.int64))  # edge (0, 1) has three faces; the fin (0, 1, 4) is smallest
    return dict(degenerate=degenerate, duplicated=duplicated, twins=twins, three=three)


def test_cleaning_rules_on_hand_built_meshes():
    m = hand_built_meshes()
    v, f, vmap = dr.clean(*m["degenerate"])
    assert f.tolist() == [[0, 1, 2], [0, 2, 3], [1, 4, 2]] and len(v) == 5 and vmap.tolist() == [0, 1, 2, 3, 4]
    v, f, vmap = dr.clean(*m["duplicated"])
    assert f.tolist() == [[0, 1, 2], [0, 2, 3], [1, 4, 2]]                    # the lowest face id of the pair survives
    v, f, vmap = dr.clean(*m["twins"])
    assert f.tolist() == [[0, 1, 2], [0, 2, 3], [1, 4, 2]] and len(v) == 5 and vmap.tolist() == [0, 1, 2, 3, 4, 2]
    v, f, vmap = dr.clean(*m["three"])
    assert f.tolist() == [[0, 1, 2], [1, 0, 3]] and len(v) == 4 and vmap.tolist() == [0, 1, 2, 3, -1, -1]
    # each rule can be switched off
    assert len(dr.clean(*m["degenerate"], degenerate=False, non_manifold_edges=False)[1]) == 4
    assert len(dr.clean(*m["duplicated"], duplicated_triangles=False, non_manifold_edges=False)[1]) == 4
    assert len(dr.clean(*m["twins"], duplicated_vertices=False)[0]) == 6
    assert len(dr.clean(*m["three"], non_manifold_edges=False)[1]) == 3
    # ties of the non-manifold rule go to the highest face id
    v3, f3 = m["three"]
    v3 = v3.copy(); v3[4] = [0.5, 0, 1]; v3[2] = [0.5, 1, 0]; v3[3] = [0.5, -1, 0]    # three faces of equal area
    assert dr.clean(v3, f3)[1].tolist() == [[0, 1, 2], [1, 0, 3]]


@pytest.mark.parametrize("name", FIELDS)
def test_clean_is_the_identity_on_marching_cubes_meshes(name):
    v, f = mc_mesh(name, 64)
    v2, f2, vmap = dr.clean(v, f)
    assert np.array_equal(v2.view(np.uint32), v.view(np.uint32)) and np.array_equal(f2, f) and np.array_equal(vmap, np.arange(len(v)))


# ------------------------------------------------------------------------------------------------ ABI and refusals
def test_abi_exports_and_refusals(hip_lib):
    from sugar_amd import _lib
    names = [n for n in _lib.SIGNATURES if n.startswith(("sgr_mesh_decimate_", "sgr_mesh_clean_"))]
    assert len(names) == 11 and all(hasattr(hip_lib, n) for n in names)
    assert hip_lib.sgr_abi_version() == 4
    assert hip_lib.sgr_mesh_decimate_quadrics(0, 4, None, None, None, None, None, 1.0, None, None) == -1
    assert hip_lib.sgr_mesh_decimate_quadrics(4, 2 ** 30, None, None, None, None, None, 1.0, None, None) == -1      # 3 F >= 2^31
    assert b"2^31" in hip_lib.sgr_last_error()
    assert hip_lib.sgr_mesh_decimate_quadrics(4, 4, None, None, None, None, None, 1.0, None, None) == -1          # null pointers
    assert hip_lib.sgr_mesh_clean_degenerate(0, None, None, None) == -1
    text = open(os.path.join(ROOT, "include", "sugar_raster.h")).read()
    assert "#define SGR_MESH_DECIMATE_PASSES 4" in text and dr.PASSES == 4
    assert not os.path.exists(os.path.join(ROOT, "sugar_amd", "shims", "open3d"))


def test_cpu_tensors_are_refused():
    from sugar_amd import decimate as dec, extract
    v, f = (torch.from_numpy(a) for a in tetrahedron())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dec.decimate(v, f, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dec.clean(v, f)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        extract.extract_mesh_marching_cubes(torch.zeros(8, 3), torch.ones(8, 3), torch.ones(8, 4), torch.ones(8), torch.zeros(8, 3), 1.0,
                                            decimation_target=100, clean=True)
    assert dec.round_limit(14120, 3408) == dr.round_limit(14120, 3408) == 56 and dec.round_limit(4, 0) == 48
