"""CPU tests of the refine stage's mesh binding: the topology builder of sugar_amd.mesh_bind against a brute-force enumeration, the
opt-in bindings (`sugar_patch.install_binding`, `shims.install(patch_binding=...)`, `launch --patch-binding`) on a fake SuGaR class, and
-- where the reference tree is present -- the fixture maker against tests/golden/sugar_binding.npz.  The HIP kernels are covered by
tests/test_gpu_mesh_bind.py."""
import itertools
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sugar_binding.npz")

CUBE = [[0, 2, 1], [0, 3, 2], [4, 5, 6], [4, 6, 7], [0, 1, 5], [0, 5, 4], [1, 2, 6], [1, 6, 5], [2, 3, 7], [2, 7, 6], [3, 0, 4], [3, 4, 7]]


def _sheet(nx=4, ny=3):
    faces = []
    for y in range(ny):
        for x in range(nx):
            a = y * (nx + 1) + x
            faces += [[a, a + 1, a + nx + 2], [a, a + nx + 2, a + nx + 1]]
    return faces, (nx + 1) * (ny + 1)


MESHES = {
    "closed": (CUBE, 8),
    "open": _sheet(),
    "non_manifold": ([[0, 1, 2], [1, 0, 3], [0, 1, 4], [2, 1, 5]], 6),          # edge (0, 1) is shared by three faces
    "isolated_vertex": (CUBE[:6] + [[9, 5, 6]], 11),                            # vertices 8 and 10 belong to no face
}


def _brute_force_pairs(faces):
    """{(f, g), f < g} once per edge the two faces share"""
    out = []
    for f, g in itertools.combinations(range(len(faces)), 2):
        ef = {frozenset(e) for e in zip(faces[f], faces[f][1:] + faces[f][:1])}
        eg = {frozenset(e) for e in zip(faces[g], faces[g][1:] + faces[g][:1])}
        out += [(f, g)] * len(ef & eg)
    return sorted(out)


def _standin_pairs(faces, n_verts):
    """the face pairs `shims/pytorch3d/loss` derives, through its own helpers"""
    from sugar_amd import shims
    shims.install()
    import pytorch3d
    if not getattr(pytorch3d, "__version__", "").endswith("sugar_amd.shim"):
        return None
    from pytorch3d.loss import _face_pairs_by_edge
    from pytorch3d.structures import Meshes
    f = torch.tensor(faces)
    m = Meshes(verts=[torch.zeros(n_verts, 3)], faces=[f])
    F_ = f.shape[0]
    edge_idx, order = m.faces_packed_to_edges_packed().reshape(F_ * 3).sort()
    face_of = torch.arange(F_)[:, None].expand(F_, 3).reshape(-1)[order]
    pair = _face_pairs_by_edge(edge_idx)
    return sorted(tuple(sorted((int(face_of[i]), int(face_of[j])))) for i, j in pair.tolist())


@pytest.mark.parametrize("name", list(MESHES))
def test_topology_matches_brute_force(name):
    from sugar_amd.mesh_bind import MeshTopology
    faces, V = MESHES[name]
    MeshTopology.clear()
    t = MeshTopology.get(torch.tensor(faces), V)
    F_ = len(faces)
    assert t.faces.dtype == torch.int32 and t.faces.tolist() == faces and (t.n_faces, t.n_verts) == (F_, V)
    # the pair list: as a multiset of unordered face pairs, the brute-force enumeration and the stand-in's own derivation
    want = _brute_force_pairs(faces)
    got = sorted(tuple(sorted(p)) for p in t.pair_faces.tolist())
    assert got == want and t.n_pairs == len(want) == t.pairs.shape[0]
    standin = _standin_pairs(faces, V)
    if standin is not None:
        assert got == standin
    # every pair row: (v0, v1) is the shared edge with v0 < v1, a / b the remaining vertex of the first / second face
    for (v0, v1, a, b), (f, g) in zip(t.pairs.tolist(), t.pair_faces.tolist()):
        assert v0 < v1 and {v0, v1} <= set(faces[f]) and {v0, v1} <= set(faces[g])
        assert set(faces[f]) == {v0, v1, a} and set(faces[g]) == {v0, v1, b}
    # the two vertex lists: complete, ascending within a vertex, empty for a vertex without faces
    for offsets, items, flat, width in ((t.vert_offsets, t.vert_items, [v for f in faces for v in f], 3),
                                        (t.pair_offsets, t.pair_items, [v for p in t.pairs.tolist() for v in p], 4)):
        offsets, items = offsets.tolist(), items.tolist()
        assert len(offsets) == V + 1 and offsets[0] == 0 and offsets[-1] == len(flat) == len(items)
        assert sorted(items) == list(range(len(flat)))
        for v in range(V):
            mine = items[offsets[v]:offsets[v + 1]]
            assert mine == [i for i, x in enumerate(flat) if x == v]
    if name == "isolated_vertex":
        assert t.vert_offsets[9] == t.vert_offsets[8] and t.vert_offsets[11] == t.vert_offsets[10]
    if name == "non_manifold":
        assert [p for p in got if p in ((0, 1), (0, 2), (1, 2))] == [(0, 1), (0, 2), (1, 2)]
    if name == "open":
        assert t.n_pairs == 3 * 4 * 3 - (4 + 3)          # interior edges of a 4 x 3 sheet: 3 per cell minus the right / top border


def test_topology_cache_and_validation():
    from sugar_amd import mesh_bind
    from sugar_amd.mesh_bind import MeshTopology
    MeshTopology.clear()
    f = torch.tensor(CUBE)
    t = MeshTopology.get(f, 8)
    assert MeshTopology.get(f, 8) is t
    assert MeshTopology.get(f).n_verts == 8                 # the vertex count read from the faces
    f[0, 0] = 0                                             # an in-place write bumps the version counter: a new entry
    assert MeshTopology.get(f, 8) is not t
    for k in range(mesh_bind.CACHE_ENTRIES + 2):
        MeshTopology.get(torch.tensor(CUBE), 8 + k)
    assert len(MeshTopology._cache) == mesh_bind.CACHE_ENTRIES
    with pytest.raises(ValueError):
        MeshTopology.get(torch.tensor([[0, 1, 8]]), 8)
    with pytest.raises(ValueError):
        MeshTopology.get(torch.zeros(4, 3), 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh_bind.bound_points(torch.zeros(8, 3), f, torch.ones(1, 3) / 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh_bind.normal_consistency(torch.zeros(8, 3), f)


def test_a_face_repeating_a_vertex_pairs_with_itself_as_in_the_standin():
    from sugar_amd.mesh_bind import MeshTopology
    faces = CUBE[:4] + [[0, 1, 1]]
    MeshTopology.clear()
    t = MeshTopology.get(torch.tensor(faces), 8)
    got = sorted(tuple(sorted(p)) for p in t.pair_faces.tolist())
    assert (4, 4) in got
    standin = _standin_pairs(faces, 8)
    if standin is not None:
        assert got == standin


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_topology_is_built_once_on_the_route_the_reference_takes(monkeypatch, dtype):
    """refine.py:776-783 calls mesh_normal_consistency(sugar.surface_mesh) every iteration, and `surface_mesh` (sugar_model.py:552-560)
    builds a NEW Meshes from the model's faces Parameter each time.  The stand-in Meshes converts int32 faces (what open3d's triangles
    are) to a fresh int64 tensor per call; the switch must still find the cached topology.  Without a GPU the device test of the switch
    and the kernel call are replaced; the route from Meshes to MeshTopology.get is the real one."""
    from sugar_amd import mesh_bind, shims
    shims.install()
    import pytorch3d
    if not getattr(pytorch3d, "__version__", "").endswith("sugar_amd.shim"):
        pytest.skip("a real pytorch3d is installed: the stand-in loss is not in use")
    import pytorch3d.loss as loss
    from pytorch3d.renderer import TexturesVertex
    from pytorch3d.structures import Meshes
    faces_param = torch.nn.Parameter(torch.tensor(CUBE, dtype=dtype), requires_grad=False)
    points = torch.nn.Parameter(torch.rand(8, 3))
    colors = torch.rand(8, 3)
    surface_mesh = lambda: Meshes(verts=[points.to("cpu")], faces=[faces_param.to("cpu")],
                                  textures=TexturesVertex(verts_features=colors[None].clamp(0, 1)))
    built, served = [], []
    real_init = mesh_bind.MeshTopology.__init__

    def counting_init(self, *a, **k):
        built.append(1)
        real_init(self, *a, **k)
    monkeypatch.setattr(mesh_bind.MeshTopology, "__init__", counting_init)
    monkeypatch.setattr(mesh_bind, "_need_gpu", lambda *a, **k: None)
    monkeypatch.setattr(mesh_bind._NormalConsistency, "apply", staticmethod(lambda verts, topo: served.append(topo) or verts.sum() * 0.0))
    monkeypatch.setattr(loss, "_on_rocm_f32", lambda t: True)
    monkeypatch.setattr(loss, "USE_HIP_NORMAL_CONSISTENCY", True)
    mesh_bind.MeshTopology.clear()
    for _ in range(6):
        loss.mesh_normal_consistency(surface_mesh())
    assert len(served) == 6 and all(t is served[0] for t in served)
    assert len(built) == 1 and len(mesh_bind.MeshTopology._cache) == 1
    assert served[0].n_pairs == 18 and served[0].faces.dtype == torch.int32


# ---------------------------------------------------------------------------------------------------------------- the bindings
def _fake_module():
    class SuGaR:
        binded_to_surface_mesh = True
        editable = False
        scale_activation = torch.exp

        def __init__(self):
            self._points = torch.zeros(8, 3)
            self._scales = torch.zeros(12, 2)
            self._quaternions = torch.zeros(12, 2)
            self._surface_mesh_faces = torch.tensor(CUBE)
            self.surface_mesh_thickness = torch.tensor(1e-6)

        points = property(lambda self: "points of the reference")
        scaling = property(lambda self: "scaling of the reference")
        quaternions = property(lambda self: "quaternions of the reference")

        def get_normals(self):
            return "normals of the reference"
    SuGaR.scale_activation = torch.exp
    return types.SimpleNamespace(SuGaR=SuGaR, use_old_method=False)


class _OnDevice:
    """makes `_binding_applies` see ROCm tensors without a GPU: the three checks it makes are `torch.is_tensor` and `.is_cuda`"""
    def __enter__(self):
        from sugar_amd import sugar_patch
        self.sp, self.real = sugar_patch, sugar_patch.torch
        fake = types.SimpleNamespace(is_tensor=lambda t: True, exp=torch.exp, float32=torch.float32)
        sugar_patch.torch = fake
        return self

    def __exit__(self, *a):
        self.sp.torch = self.real


class _Cuda:
    is_cuda = True
    dtype = torch.float32


class _CudaDouble(_Cuda):
    dtype = torch.float64


def _put_on_device(model):
    for k in ("_points", "_scales", "_quaternions", "_surface_mesh_faces", "surface_mesh_thickness"):
        setattr(model, k, _Cuda())


def test_install_binding_takes_over_only_what_it_implements(monkeypatch):
    from sugar_amd import sugar_patch
    sm = _fake_module()
    originals = {k: sm.SuGaR.__dict__[k] for k in sugar_patch.BINDING_PROPERTIES}
    assert sugar_patch.install_binding(sm) == list(sugar_patch.BINDING_PROPERTIES)
    assert sugar_patch.install_binding(sm) == list(sugar_patch.BINDING_PROPERTIES)          # idempotent
    assert all(sm.SuGaR.__dict__[k].original is originals[k] for k in originals)
    m = sm.SuGaR()
    # CPU tensors: the reference's getters
    assert (m.points, m.scaling, m.quaternions) == ("points of the reference", "scaling of the reference", "quaternions of the reference")
    served = []
    monkeypatch.setattr(sugar_patch, "_binding_value", lambda self, name: served.append(name) or f"{name} of the kernels")
    with _OnDevice():
        _put_on_device(m)
        assert (m.points, m.scaling, m.quaternions) == ("points of the kernels", "scaling of the kernels", "quaternions of the kernels")
        m.editable = True
        assert (m.points, m.scaling, m.quaternions) == ("points of the reference", "scaling of the reference", "quaternions of the reference")
        m.editable = False
        sm.use_old_method = True
        assert m.quaternions == "quaternions of the reference"
        sm.use_old_method = False
        m.scale_activation = torch.nn.functional.softplus          # not exp: scaling alone falls back
        assert (m.points, m.scaling, m.quaternions) == ("points of the kernels", "scaling of the reference", "quaternions of the kernels")
        m.scale_activation = torch.exp
        # parameters that are not float32 keep the reference's getter (and with it their dtype)
        m._points = _CudaDouble()
        assert (m.points, m.scaling, m.quaternions) == ("points of the reference", "scaling of the kernels", "quaternions of the reference")
        m._points, m._scales = _Cuda(), _CudaDouble()
        assert (m.points, m.scaling, m.quaternions) == ("points of the kernels", "scaling of the reference", "quaternions of the kernels")
        m._scales, m._quaternions = _Cuda(), _CudaDouble()
        assert (m.points, m.scaling, m.quaternions) == ("points of the kernels", "scaling of the kernels", "quaternions of the reference")
        m._quaternions = _Cuda()
        m.binded_to_surface_mesh = False
        assert m.points == "points of the reference"
    sugar_patch.uninstall_binding(sm)
    assert all(sm.SuGaR.__dict__[k] is originals[k] for k in originals)
    sugar_patch.uninstall_binding(sm)                                                       # harmless when nothing is installed


@pytest.mark.parametrize("order", ["binding_first", "gathers_first"])
@pytest.mark.parametrize("undo", ["binding_first", "gathers_first", "uninstall"])
def test_binding_composes_with_row_gathers(monkeypatch, order, undo):
    from sugar_amd import row_gather, sugar_patch
    sm = _fake_module()
    originals = {k: sm.SuGaR.__dict__[k] for k in sugar_patch.BINDING_PROPERTIES}
    monkeypatch.setattr(row_gather, "as_row_gather", lambda t: ("row gather", t))     # (the installers bind it when they run)
    steps = [sugar_patch.install_binding, sugar_patch.install_row_gathers]
    for step in (steps if order == "binding_first" else steps[::-1]):
        step(sm)
    sugar_patch.install_binding(sm)                      # idempotent in both orders
    monkeypatch.setattr(sugar_patch, "_binding_value", lambda self, name: f"{name} of the kernels")
    m = sm.SuGaR()
    assert m.points == ("row gather", "points of the reference")
    with _OnDevice():
        _put_on_device(m)
        assert m.quaternions == ("row gather", "quaternions of the kernels") and m.scaling == ("row gather", "scaling of the kernels")
    assert m.get_normals() == ("row gather", "normals of the reference")
    if undo == "uninstall":
        sugar_patch.uninstall(sm)
    else:
        undos = [sugar_patch.uninstall_binding, sugar_patch.uninstall_row_gathers]
        first, second = undos if undo == "binding_first" else undos[::-1]
        first(sm)
        with _OnDevice():                                # the other binding is still in place, alone
            if first is sugar_patch.uninstall_binding:
                assert m.quaternions == ("row gather", "quaternions of the reference")
            else:
                assert m.quaternions == "quaternions of the kernels"
        second(sm)
    assert all(sm.SuGaR.__dict__[k] is originals[k] for k in originals)
    assert m.points == "points of the reference" and m.get_normals() == "normals of the reference"


def test_shims_install_patch_binding_sets_the_loss_switch():
    from sugar_amd import shims, sugar_patch
    sm = _fake_module()
    shims.install()
    import pytorch3d
    standin = getattr(pytorch3d, "__version__", "").endswith("sugar_amd.shim")
    import pytorch3d.loss as loss
    if standin:
        assert loss.USE_HIP_NORMAL_CONSISTENCY is False                     # off unless asked for
    try:
        shims.install(patch_binding=sm)
        assert isinstance(sm.SuGaR.__dict__["points"], sugar_patch._BindingProperty)
        if standin:
            assert loss.USE_HIP_NORMAL_CONSISTENCY is True
            # a CPU mesh still takes the stand-in's own torch path
            from pytorch3d.structures import Meshes
            v = torch.tensor([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]], dtype=torch.float32)
            assert abs(float(loss.mesh_normal_consistency(Meshes([v], [torch.tensor(CUBE)]))) - 12 / 18) < 1e-6
    finally:
        shims.uninstall_binding(sm)
    assert not isinstance(sm.SuGaR.__dict__["points"], sugar_patch._BindingProperty)
    if standin:
        assert loss.USE_HIP_NORMAL_CONSISTENCY is False


def test_launch_patch_binding_is_opt_in(monkeypatch, tmp_path):
    from sugar_amd import launch, shims, sugar_patch
    sm = _fake_module()
    sm.__name__ = "sugar_scene.sugar_model"
    monkeypatch.setitem(sys.modules, "sugar_scene.sugar_model", sm)
    script = tmp_path / "train.py"
    script.write_text("")
    syspath = list(sys.path)
    off = dict(patch_sugar=False, patch_gathers=False, patch_losses=False, patch_optimizer=False, patch_densifier=False,
               patch_texture=False)
    try:
        done = launch.prepare(str(script), **off)
        assert done["patch_binding"] == 0 and not isinstance(sm.SuGaR.__dict__["points"], sugar_patch._BindingProperty)
        done = launch.prepare(str(script), **off, patch_binding=True)
        assert done["patch_binding"] >= 3 and isinstance(sm.SuGaR.__dict__["points"], sugar_patch._BindingProperty)
        with pytest.raises(TypeError):
            launch.prepare(str(script), False, False, False, False, False, False, True)          # keyword-only
    finally:
        shims.uninstall_binding(sm)
        sys.path[:] = syspath
    with pytest.raises(SystemExit):
        launch.main(["--patch-binding", "--help"])


# ---------------------------------------------------------------------------------------------------------------- the fixture
def test_fixture_meets_its_conditions():
    """what the GPU test relies on: shapes, and -- recomputed from the recorded float64 quaternions -- the arg-max margin"""
    d = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) < 1 << 20
    for n in (1, 3, 4, 6):
        F_ = d[f"n{n}_faces"].shape[0]
        assert d[f"n{n}_bary"].shape == (n, 3) and d[f"n{n}__scales"].shape == (F_ * n, 2)
        assert d[f"n{n}_out_quaternions"].shape == (F_ * n, 4) and d[f"n{n}_out_quaternions_f64"].dtype == np.float64
        q = d[f"n{n}_out_quaternions_f64"]
        q_abs = np.sort(2.0 * np.abs(q), axis=1)        # q_abs of a rotation matrix = 2 |q| component-wise
        assert float((q_abs[:, 3] - q_abs[:, 2]).min()) > 1e-3


def test_maker_reproduces_the_fixture():
    """the unmodified reference class on the CPU writes tests/golden/sugar_binding.npz"""
    from tests import ref_env
    if ref_env.reference_root() is None:
        pytest.skip("no reference tree")
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    try:
        import make_sugar_binding as mk
        out = mk.run()
    finally:
        sys.path.remove(os.path.join(ROOT, "tests", "golden"))
    d = np.load(GOLDEN)
    assert sorted(out) == sorted(d.files)
    for k in d.files:
        a, b = np.asarray(out[k]), d[k]
        assert a.shape == b.shape and a.dtype == b.dtype, k
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)) if a.dtype.kind == "f" else np.array_equal(a, b), k
