"""CPU tests of the refined-mesh texture path: the stand-in shading classes the reference's
`extract_texture_image_and_uv_from_gaussians` imports (SoftPhongShader over TexturesUV with nearest sampling, softmax_rgb_blend,
AmbientLights, MeshRenderer), `pytorch3d.io.save_obj`, the UV layout of sugar_amd.texture against the fixture, the bindings of
`shims.install(patch_texture=...)` / `launch --no-patch-texture`, and -- where the reference tree is present -- the reference's own
function on the CPU against tests/golden/sugar_texture.npz.  The HIP kernels are covered by tests/test_gpu_texture.py."""
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sugar_texture.npz")


@pytest.fixture(scope="module")
def p3d():
    from sugar_amd import shims
    shims.install()
    import pytorch3d
    if not getattr(pytorch3d, "__version__", "").endswith("sugar_amd.shim"):
        pytest.skip("a real pytorch3d is installed: the stand-in classes are not in use")
    return pytorch3d


def _fragments(p2f, bary, zbuf, dists):
    from pytorch3d.renderer import Fragments
    t = lambda a, dt=torch.float32: torch.as_tensor(a, dtype=dt)
    return Fragments(pix_to_face=t(p2f, torch.int64)[None, :, :, None], zbuf=t(zbuf)[None, :, :, None],
                     bary_coords=t(bary)[None, :, :, None, :], dists=t(dists)[None, :, :, None])


def _index_mesh(S, verts_uv):
    """one triangle carrying the reference's index texture (texture_idx[a, b] = (a, b, 0), sugar_model.py:2628-2646)"""
    from pytorch3d.renderer import TexturesUV
    from pytorch3d.structures import Meshes
    a = torch.arange(S)
    idx = torch.cartesian_prod(a, a).reshape(S, S, 2)
    idx = torch.cat([idx, torch.zeros_like(idx[..., :1])], dim=-1)
    tex = TexturesUV(maps=idx[None].float(), verts_uvs=torch.as_tensor(verts_uv, dtype=torch.float32)[None],
                     faces_uvs=torch.tensor([[0, 1, 2]])[None], sampling_mode="nearest")
    return Meshes(verts=[torch.zeros(3, 3)], faces=[torch.tensor([[0, 1, 2]])], textures=tex)


def _shade(S, verts_uv, bary, zbuf=1.0, dists=-1.0, znear=1e-4, zfar=100.0):
    from pytorch3d.renderer import AmbientLights, FoVPerspectiveCameras, SoftPhongShader
    from pytorch3d.renderer.blending import BlendParams
    bary = torch.as_tensor(bary, dtype=torch.float32).reshape(1, -1, 3)
    n = bary.shape[1]
    fr = _fragments(torch.zeros(1, n), bary, torch.full((1, n), zbuf), torch.full((1, n), dists))
    cams = FoVPerspectiveCameras(znear=znear, zfar=zfar)
    shader = SoftPhongShader(cameras=cams, lights=AmbientLights(), blend_params=BlendParams(background_color=(0.0, 0.0, 0.0)))
    return shader(fr, _index_mesh(S, verts_uv), cameras=cams)[0, 0, :, :2]


def test_shader_nearest_texel_indices(p3d):
    """the texel a UV lands on: column = round(u (S-1)), row of the y-flipped map = S-1-round(v (S-1)) -> (S-1-row, col)"""
    S = 11
    # vertex k of the triangle sits exactly at UV k, so bary = e_k reads the texel under that corner
    uv = [[0.0, 0.0], [1.0, 0.0], [0.3, 0.7]]
    got = _shade(S, uv, [[1, 0, 0], [0, 1, 0], [0, 0, 1]])
    assert got.tolist() == [[10.0, 0.0], [10.0, 10.0], [3.0, 3.0]]


def test_shader_border_clamp_and_round_half_even(p3d):
    S = 11
    uv = [[-0.5, 1.7], [0.25, 0.25], [0.75, 0.75]]    # corner 0 outside the map: clamped to the border
    got = _shade(S, uv, [[1, 0, 0], [0, 1, 0], [0, 0, 1]])
    # 0.25 -> 2.5 -> 2 and 0.75 -> 7.5 -> 8 (exact halves, rounded to even); the row is flipped: 10 - 2 = 8, 10 - 8 = 2
    assert got.tolist() == [[0.0, 0.0], [8.0, 2.0], [2.0, 8.0]]


def test_shader_beyond_zfar_lands_on_texel_zero(p3d):
    """a covered pixel beyond zfar blends to the background 0 -> texel (0, 0); just beyond, the blend is partial"""
    S = 101
    uv = [[0.8, 0.2], [0.8, 0.2], [0.8, 0.2]]
    inside = _shade(S, uv, [[1, 0, 0]], zbuf=50.0)
    assert inside.tolist() == [[80.0, 80.0]]
    assert _shade(S, uv, [[1, 0, 0]], zbuf=101.0).round().tolist() == [[0.0, 0.0]]
    partial = _shade(S, uv, [[1, 0, 0]], zbuf=100.0 + 5e-4)
    assert 0.0 < float(partial[0, 0]) < 80.0


def test_shader_rejects_what_it_does_not_implement(p3d):
    from pytorch3d.renderer import FoVPerspectiveCameras, SoftPhongShader
    fr = _fragments(torch.zeros(1, 1), torch.ones(1, 1, 3) / 3, torch.ones(1, 1), -torch.ones(1, 1))
    with pytest.raises(NotImplementedError):
        SoftPhongShader(cameras=FoVPerspectiveCameras(), lights=object())(fr, _index_mesh(4, [[0, 0], [1, 0], [0, 1]]))
    mesh = _index_mesh(4, [[0, 0], [1, 0], [0, 1]])
    mesh.textures.sampling_mode = "bilinear"
    with pytest.raises(NotImplementedError):
        SoftPhongShader(cameras=FoVPerspectiveCameras())(fr, mesh)


def test_save_obj_round_trip(p3d, tmp_path):
    from PIL import Image
    from pytorch3d.io import save_obj
    g = torch.Generator().manual_seed(3)
    verts = torch.randn(7, 3, generator=g)
    faces = torch.tensor([[0, 1, 2], [2, 3, 4], [4, 5, 6]])
    verts_uv = torch.rand(9, 2, generator=g)
    faces_uv = torch.arange(9).view(3, 3)
    tmap = torch.rand(6, 5, 3, generator=g)
    path = tmp_path / "mesh.obj"
    save_obj(str(path), verts=verts, faces=faces, verts_uvs=verts_uv, faces_uvs=faces_uv, texture_map=tmap)
    text = path.read_text()
    assert text.startswith("mtllib mesh.mtl\nusemtl mesh\n") and not text.endswith("\n")
    v, vt, f = [], [], []
    for line in text.splitlines():
        parts = line.split()
        if not parts:
            continue
        if parts[0] == "v":
            v.append([float(x) for x in parts[1:]])
        elif parts[0] == "vt":
            vt.append([float(x) for x in parts[1:]])
        elif parts[0] == "f":
            f.append([[int(i) - 1 for i in p.split("/")] for p in parts[1:]])
    assert np.abs(np.array(v) - verts.numpy()).max() <= 5e-7
    assert np.abs(np.array(vt) - verts_uv.numpy()).max() <= 5e-7
    f = np.array(f)
    assert np.array_equal(f[..., 0], faces.numpy()) and np.array_equal(f[..., 1], faces_uv.numpy())
    assert "map_Kd mesh.png" in (tmp_path / "mesh.mtl").read_text()
    img = np.asarray(Image.open(tmp_path / "mesh.png"))
    assert np.array_equal(img, (tmap * 255.0).numpy().astype(np.uint8))


def test_uv_layout_matches_the_fixture():
    from sugar_amd.texture import texture_size, uv_layout
    d = np.load(GOLDEN)
    T = d["faces"].shape[0]
    verts_uv, faces_uv = uv_layout(T, int(d["square_size"]), "cpu")
    assert verts_uv.dtype == torch.float32 and faces_uv.dtype == torch.int64
    assert np.array_equal(verts_uv.numpy().view(np.uint32), d["verts_uv"].view(np.uint32))
    assert np.array_equal(faces_uv.numpy(), d["faces_uv"])
    assert texture_size(T, int(d["square_size"])) == d["counter"].shape[0]
    # other sizes: P = int(sqrt(T // 2 + 1) + 1), verts_uv has 6 P^2 rows, every UV inside [-3/S, 1 + 3/S]
    for T, s in ((1, 3), (2, 10), (7, 4), (1000, 10), (12345, 6)):
        S = texture_size(T, s)
        vu, fu = uv_layout(T, s, "cpu")
        assert vu.shape == (6 * (S // s) ** 2, 2) and fu.shape == (T, 3) and int(fu.max()) < vu.shape[0]
        assert float(vu.min()) >= -3.0 / S and float(vu.max()) <= 1.0 + 3.0 / S


def test_cpu_tensors_raise():
    from sugar_amd.texture import TextureBaker, extract_texture_image_and_uv_from_gaussians
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        TextureBaker(torch.zeros(3, 3), torch.tensor([[0, 1, 2]]), torch.zeros(1, 3), torch.zeros(1, 3, 3), torch.zeros(1, 3), 1, 10)
    rc = types.SimpleNamespace(surface_mesh=types.SimpleNamespace(verts_list=lambda: [torch.zeros(3, 3)],
                                                                  faces_list=lambda: [torch.tensor([[0, 1, 2]])]),
                               n_gaussians_per_surface_triangle=1, sh_coordinates=torch.zeros(1, 1, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        extract_texture_image_and_uv_from_gaussians(rc)
    with pytest.raises(ValueError):
        extract_texture_image_and_uv_from_gaussians(rc, square_size=2)
    rc.sh_coordinates = torch.zeros(1, 4, 3)
    with pytest.raises(ValueError):
        extract_texture_image_and_uv_from_gaussians(rc)          # n_sh = -1 on a degree-1 model: 4 features
    with pytest.raises(ValueError):
        extract_texture_image_and_uv_from_gaussians(rc, n_sh=4)


def _fake_reference_modules():
    def original(rc, square_size=10, n_sh=-1, texture_with_gaussian_renders=True):
        return "reference"
    sm = types.ModuleType("sugar_scene.sugar_model")
    sm.extract_texture_image_and_uv_from_gaussians = original
    rm = types.ModuleType("sugar_extractors.refined_mesh")
    rm.extract_texture_image_and_uv_from_gaussians = original
    return sm, rm, original


def test_install_patch_texture_rebinds_both_names(monkeypatch):
    from sugar_amd import shims, texture
    sm, rm, original = _fake_reference_modules()
    monkeypatch.setitem(sys.modules, "sugar_scene.sugar_model", sm)
    monkeypatch.setitem(sys.modules, "sugar_extractors.refined_mesh", rm)
    shims.install(patch_texture=sm)
    for mod in (sm, rm):
        f = mod.extract_texture_image_and_uv_from_gaussians
        assert f is not original and f._sugar_amd_original is original
    calls = []
    monkeypatch.setattr(texture, "extract_texture_image_and_uv_from_gaussians", lambda *a: calls.append(a) or "hip")
    assert rm.extract_texture_image_and_uv_from_gaussians("rc", square_size=8, n_sh=1) == "hip"
    assert calls == [("rc", 8, 1, True)]
    assert shims.install_texture(sm) == 2          # idempotent
    assert sm.extract_texture_image_and_uv_from_gaussians._sugar_amd_original is original
    assert shims.uninstall_texture() == 2
    assert sm.extract_texture_image_and_uv_from_gaussians is original and rm.extract_texture_image_and_uv_from_gaussians is original


def test_launch_no_patch_texture_leaves_the_names_alone(monkeypatch, tmp_path):
    from sugar_amd import launch, shims
    sm, rm, original = _fake_reference_modules()
    monkeypatch.setitem(sys.modules, "sugar_scene.sugar_model", sm)
    monkeypatch.setitem(sys.modules, "sugar_extractors.refined_mesh", rm)
    monkeypatch.setattr(shims, "install", lambda *a, **k: "shim")     # (the fake module has no SuGaR class to patch)
    script = tmp_path / "train.py"
    script.write_text("")
    syspath = list(sys.path)
    try:
        done = launch.prepare(str(script), patch_sugar=False, patch_gathers=False, patch_losses=False, patch_optimizer=False,
                              patch_densifier=False, patch_texture=False)
        assert done["patch_texture"] == 0
        assert sm.extract_texture_image_and_uv_from_gaussians is original and rm.extract_texture_image_and_uv_from_gaussians is original
        done = launch.prepare(str(script), patch_sugar=False, patch_gathers=False, patch_losses=False, patch_optimizer=False,
                              patch_densifier=False)
        assert done["patch_texture"] == 2
        assert rm.extract_texture_image_and_uv_from_gaussians._sugar_amd_original is original
    finally:
        shims.uninstall_texture()
        sys.path[:] = syspath
    with pytest.raises(SystemExit):
        launch.main(["--no-patch-texture", "--help"])


def test_reference_function_reproduces_the_fixture():
    """the unmodified reference function on the CPU (stand-in shader, oracle rasterizers) writes tests/golden/sugar_texture.npz"""
    from tests import ref_env
    if ref_env.reference_root() is None:
        pytest.skip("no reference tree")
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    try:
        import make_sugar_texture as mk
        out = mk.run()
    finally:
        sys.path.remove(os.path.join(ROOT, "tests", "golden"))
    d = np.load(GOLDEN)
    assert sorted(out) == sorted(d.files)
    for k in d.files:
        a, b = np.asarray(out[k]), d[k]
        assert a.shape == b.shape and a.dtype == b.dtype, k
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)) if a.dtype.kind == "f" else np.array_equal(a, b), k
