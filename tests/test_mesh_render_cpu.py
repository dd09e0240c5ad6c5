"""CPU tests of the textured-mesh render path: the stand-in `pytorch3d.io.load_obj` / `load_objs_as_meshes` against what `save_obj`
writes and against hand-written files, the argument checks of `sugar_amd.mesh_render`, and the float32-against-float64 run of the
reference formulation (tests/mesh_render_scenes.py) that the GPU tolerances come from.  The HIP kernel is covered by
tests/test_gpu_mesh_render.py."""
import ast
import os

import numpy as np
import pytest
import torch

from tests import mesh_render_scenes as ms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def p3d():
    from sugar_amd import shims
    shims.install()
    import pytorch3d
    if not getattr(pytorch3d, "__version__", "").endswith("sugar_amd.shim"):
        pytest.skip("a real pytorch3d is installed: the stand-in classes are not in use")
    return pytorch3d


def _small_mesh():
    g = torch.Generator().manual_seed(5)
    verts = torch.randn(7, 3, generator=g)
    faces = torch.tensor([[0, 1, 2], [2, 3, 4], [4, 5, 6], [6, 0, 3]])
    verts_uv = torch.rand(12, 2, generator=g)
    faces_uv = torch.arange(12).view(4, 3)
    tmap = torch.rand(6, 5, 3, generator=g)
    return verts, faces, verts_uv, faces_uv, tmap


def test_obj_round_trip(p3d, tmp_path):
    """save_obj -> load_obj / load_objs_as_meshes: vertices and UVs to the six decimals save_obj writes, indices equal, the texture
    exactly the uint8 image / 255, the TexturesUV at the container's defaults"""
    from pytorch3d.io import load_obj, load_objs_as_meshes, save_obj
    verts, faces, verts_uv, faces_uv, tmap = _small_mesh()
    path = tmp_path / "mesh.obj"
    save_obj(str(path), verts=verts, faces=faces, verts_uvs=verts_uv, faces_uvs=faces_uv, texture_map=tmap)
    v, f, aux = load_obj(str(path))
    assert v.dtype == torch.float32 and f.verts_idx.dtype == torch.int64 and f.textures_idx.dtype == torch.int64
    assert float((v - verts).abs().max()) <= 5e-7 and float((aux.verts_uvs - verts_uv).abs().max()) <= 5e-7
    assert torch.equal(f.verts_idx, faces) and torch.equal(f.textures_idx, faces_uv)
    assert torch.equal(f.materials_idx, torch.zeros(4, dtype=torch.int64)) and bool((f.normals_idx == -1).all()) and aux.normals is None
    expect = torch.from_numpy((tmap * 255.0).numpy().astype(np.uint8).astype(np.float32) / np.float32(255.0))
    assert list(aux.texture_images) == ["mesh"]
    img = aux.texture_images["mesh"]
    assert img.dtype == torch.float32 and img.shape == (6, 5, 3) and torch.equal(img, expect)
    mesh = load_objs_as_meshes([str(path)])
    assert len(mesh) == 1 and torch.equal(mesh.verts_list()[0], v) and torch.equal(mesh.faces_list()[0], faces)
    t = mesh.textures
    assert (t.sampling_mode, t.align_corners, t.padding_mode) == ("bilinear", True, "border")
    assert t.maps_padded().shape == (1, 6, 5, 3) and torch.equal(t.maps_padded()[0], expect)
    assert torch.equal(t.verts_uvs_list()[0], aux.verts_uvs) and torch.equal(t.faces_uvs_list()[0], faces_uv)
    two = load_objs_as_meshes([str(path), str(path)], device="cpu")
    assert len(two) == 2 and two.textures.maps_padded().shape == (2, 6, 5, 3)


_VARIANTS = """# a comment
o thing
v 0 0 0
v 1 0 0   # trailing comment tokens are ignored past the third value
v 1 1 0
v 0 1 0
v 0.5 0.5 1
vt 0 0
vt 1 0
vt 1 1
vt 0 1
vn 0 0 1
vn 0 1 0
s off
g group
f 1/1/1 2/2/1 3/3/2
f 1//2 3//2 4//1
f -5 -4 -1
f 1/1 2/2 3/3 4/4

f 5 1 2
"""


def test_loader_variants(p3d, tmp_path):
    """a/b/c, a//c, negative indices (counted from the end of the list, pytorch3d's rule), a quad fanned into two triangles, comments
    and unknown statements skipped, no mtllib -> no textures"""
    from pytorch3d.io import load_obj, load_objs_as_meshes
    path = tmp_path / "v.obj"
    path.write_text(_VARIANTS)
    v, f, aux = load_obj(str(path))
    assert v.shape == (5, 3) and aux.verts_uvs.shape == (4, 2) and aux.normals.shape == (2, 3) and aux.texture_images is None
    assert f.verts_idx.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 4], [0, 1, 2], [0, 2, 3], [4, 0, 1]]
    assert f.textures_idx.tolist() == [[0, 1, 2], [-1] * 3, [-1] * 3, [0, 1, 2], [0, 2, 3], [-1] * 3]
    assert f.normals_idx.tolist() == [[0, 0, 1], [1, 1, 0], [-1] * 3, [-1] * 3, [-1] * 3, [-1] * 3]
    assert f.materials_idx.tolist() == [-1] * 6
    mesh = load_objs_as_meshes([str(path)])
    assert mesh.textures is None and mesh.faces_list()[0].shape == (6, 3)


@pytest.mark.parametrize("line", ["f 1 2 6", "f 1/5 2/1 3/1", "f 1 2 -6", "f 1//3 2//1 3//1"])
def test_loader_rejects_an_index_past_the_end(p3d, tmp_path, line):
    from pytorch3d.io import load_obj
    path = tmp_path / "bad.obj"
    path.write_text(_VARIANTS + line + "\n")
    with pytest.raises(ValueError, match="invalid indices"):
        load_obj(str(path))


def test_loader_materials(p3d, tmp_path):
    from pytorch3d.io import load_obj, load_objs_as_meshes, save_obj
    verts, faces, verts_uv, faces_uv, tmap = _small_mesh()
    path = tmp_path / "m.obj"
    save_obj(str(path), verts=verts, faces=faces, verts_uvs=verts_uv, faces_uvs=faces_uv, texture_map=tmap)
    text = path.read_text()
    (tmp_path / "two.obj").write_text(text + "\nusemtl other\nf 1/1 2/2 3/3\n")
    with pytest.raises(NotImplementedError):
        load_obj(str(tmp_path / "two.obj"))
    (tmp_path / "partial.obj").write_text(text + "\nf 1 2 3\n")          # a textured file with a face that has no vt index
    assert load_obj(str(tmp_path / "partial.obj"))[1].textures_idx[-1].tolist() == [-1, -1, -1]
    with pytest.raises(ValueError):
        load_objs_as_meshes([str(tmp_path / "partial.obj")])
    (tmp_path / "lost.obj").write_text(text.replace("mtllib m.mtl", "mtllib gone.mtl"))
    with pytest.warns(UserWarning, match="does not exist"):
        assert load_obj(str(tmp_path / "lost.obj"))[2].texture_images is None
    assert load_obj(str(path), load_textures=False)[2].texture_images is None


def _cpu_fragments(K=1, H=4, W=5):
    return (torch.zeros(H, W, K, dtype=torch.int64), torch.ones(H, W, K), torch.full((H, W, K, 3), 1 / 3), -torch.ones(H, W, K))


def test_shade_textured_argument_checks():
    from sugar_amd.mesh_render import TexturedMeshRenderer, image_metrics, shade_textured
    uv, fuv, tex = torch.rand(3, 2), torch.tensor([[0, 1, 2]]), torch.rand(4, 4, 3)
    kw = dict(znear=1e-4, zfar=100.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        shade_textured(_cpu_fragments(), uv, fuv, tex, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        shade_textured(_cpu_fragments(3), uv, fuv, tex, sampling_mode="nearest", align_corners=False, **kw)
    with pytest.raises(NotImplementedError):
        shade_textured(_cpu_fragments(), uv, fuv, tex, padding_mode="zeros", **kw)
    p2f, z, b, d = _cpu_fragments()
    for bad in ((p2f, z[:, :-1], b, d), (p2f, z, b[..., :2], d), (p2f.int(), z, b, d), (p2f, z.double(), b, d),
                _cpu_fragments(17), (p2f[None].expand(2, -1, -1, -1), z, b, d), (p2f, z, b)):
        with pytest.raises(ValueError):
            shade_textured(bad, uv, fuv, tex, **kw)
    for args in ((uv[:, :1], fuv, tex), (uv, fuv.int(), tex), (uv, fuv, tex[..., :2]), (uv.double(), fuv, tex)):
        with pytest.raises(ValueError):
            shade_textured(_cpu_fragments(), *args, **kw)
    with pytest.raises(ValueError):
        shade_textured(_cpu_fragments(), uv, fuv, tex, sampling_mode="bicubic", **kw)
    with pytest.raises(TypeError):
        shade_textured(_cpu_fragments(), uv, fuv, tex)                      # znear / zfar are required
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        TexturedMeshRenderer(torch.zeros(3, 3), fuv, uv, fuv, tex, (4, 5))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        image_metrics(torch.zeros(8, 8, 3), torch.zeros(8, 8, 3))


def test_mesh_render_never_imports_the_oracle():
    for name in ("mesh_render.py", "render_mesh.py", os.path.join("shims", "pytorch3d", "io", "__init__.py")):
        tree = ast.parse(open(os.path.join(ROOT, "sugar_amd", name)).read())
        mods = [a.name for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names]
        mods += [n.module or "" for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)]
        assert not [m for m in mods if m.split(".")[0] in ("oracle", "tests")], name


def test_gs_camera_conversion_projects_to_the_same_pixels():
    """p3d_camera_from_gs: a world point lands on the pixel the Gaussian rasterizer's full projection puts it on"""
    from sugar_amd import synthetic as syn
    from sugar_amd.mesh_render import p3d_camera_from_gs
    Wd, Hd = 128, 96
    cam = syn.orbit_cameras(Wd, Hd, n=3, radius=2.5)[1]
    p3 = p3d_camera_from_gs(cam, "cpu")
    pts = torch.tensor([[0.1, -0.2, 0.3], [-0.4, 0.25, -0.1], [0.0, 0.0, 0.0]])
    ndc = p3.transform_points(pts)
    s = min(Wd, Hd) / 2.0
    px = torch.stack([Wd / 2.0 - ndc[:, 0] * s, Hd / 2.0 - ndc[:, 1] * s], dim=-1)       # pytorch3d NDC: +x left, +y up
    h = torch.cat([pts, torch.ones(3, 1)], dim=1) @ cam.projmatrix
    gs = h[:, :2] / h[:, 3:4]
    expect = torch.stack([(gs[:, 0] + 1) * Wd / 2.0, (gs[:, 1] + 1) * Hd / 2.0], dim=-1)
    assert float((px - expect).abs().max()) < 1e-3
    assert float(p3.znear[0]) == pytest.approx(1e-4) and float(p3.zfar[0]) == 100.0


@pytest.mark.parametrize("K", ms.KS)
def test_reference_float32_against_float64(K):
    """where the GPU tolerances come from: the float32 run of the reference formulation stays within the recorded maxima (MEASURED,
    per (K, gamma), with a factor 2 for another host's libm; the GPU tests allow 4x); in nearest mode the share of pixels left out
    for a texel coordinate near a half-integer is below 2 %, and on every kept pixel float32 picks the float64 texel"""
    s = ms.scene(K)
    covered = (s.pix_to_face >= 0).any(-1)
    assert not covered[list(ms.EMPTY_ROWS)].any() and 0.7 < float(covered.float().mean()) < 1.0
    for Kk, mode, ac, (sigma, gamma) in ms.GRID:
        if Kk != K:
            continue
        r64, uv = ms.reference_scene(K, mode, ac, sigma, gamma)
        r32, _ = ms.reference_scene(K, mode, ac, sigma, gamma, dtype=torch.float32)
        assert r64.dtype == torch.float64 and r32.dtype == torch.float32 and r64.shape == (ms.H, ms.W, 4)
        assert not torch.isnan(r64).any() and not torch.isnan(r32).any()
        keep = torch.ones(ms.H, ms.W, dtype=torch.bool)
        if mode == "nearest":
            keep = ms.kept_pixels(s.pix_to_face, uv, ms.TEX_H, ms.TEX_W, ac)
            left_out = float((~keep & covered).sum()) / float(covered.sum())
            assert left_out <= ms.MAX_LEFT_OUT, left_out
        d = float((r32.double() - r64).abs().amax(-1)[keep].max())
        assert d <= 2 * ms.MEASURED[(K, gamma)], (mode, ac, gamma, d)
        bg = torch.tensor(ms.BACKGROUND, dtype=torch.float64)
        assert float((r64[~covered][:, :3] - bg.float().double()).abs().max()) == 0 and float(r64[~covered][:, 3].abs().max()) == 0
    assert ms.TOL == {k: 4 * v for k, v in ms.MEASURED.items()}
