"""GPU tests of the textured-mesh shading kernel (csrc/mesh_shade.hip via sugar_amd.mesh_render) against the float64 reference of
tests/mesh_render_scenes.py, end to end through the stand-in pytorch3d classes the way the reference's metrics.py renders the refined
mesh's .obj, and of `image_metrics`.  The tolerances are 4x the float32-against-float64 error of the reference formulation itself
(mesh_render_scenes.MEASURED; tests/test_mesh_render_cpu.py re-measures it).  No test feeds the kernel an index out of range."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import mesh_render_scenes as ms

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def p3d(hip_lib):
    from sugar_amd import shims
    shims.install()
    import pytorch3d
    if not getattr(pytorch3d, "__version__", "").endswith("sugar_amd.shim"):
        pytest.skip("a real pytorch3d is installed: the stand-in classes are not in use")
    return pytorch3d


_dev_scenes = {}


def _dev_scene(K):
    if K not in _dev_scenes:
        _dev_scenes[K] = ms.Scene(*(t.to(DEV) for t in ms.scene(K)))
    return _dev_scenes[K]


def _shade(K, mode, ac, sigma, gamma, s=None, **kw):
    from sugar_amd.mesh_render import shade_textured
    from sugar_amd.shims.pytorch3d.renderer.blending import BlendParams
    s = _dev_scene(K) if s is None else s
    return shade_textured((s.pix_to_face, s.zbuf, s.bary_coords, s.dists), s.verts_uvs, s.faces_uvs, s.texture, sampling_mode=mode,
                          align_corners=ac, blend_params=BlendParams(sigma, gamma, ms.BACKGROUND), znear=ms.ZNEAR, zfar=ms.ZFAR, **kw)


@pytest.mark.parametrize("K,mode,ac,sg", ms.GRID, ids=lambda v: str(v).replace(" ", ""))
def test_shade_textured_against_the_float64_reference(hip_lib, K, mode, ac, sg):
    sigma, gamma = sg
    out = _shade(K, mode, ac, sigma, gamma)
    assert out.shape == (ms.H, ms.W, 4) and out.dtype == torch.float32
    out = out.cpu()
    assert not torch.isnan(out).any()
    ref, uv = ms.reference_scene(K, mode, ac, sigma, gamma)
    s = ms.scene(K)
    covered = (s.pix_to_face >= 0).any(-1)
    keep = torch.ones(ms.H, ms.W, dtype=torch.bool)
    if mode == "nearest":
        keep = ms.kept_pixels(s.pix_to_face, uv, ms.TEX_H, ms.TEX_W, ac)
        left_out = float((~keep & covered).sum()) / float(covered.sum())
        assert left_out <= ms.MAX_LEFT_OUT, left_out
    d = (out.double() - ref).abs().amax(-1)
    worst = float(d[keep].max())
    print(f"K={K} {mode} align_corners={ac} gamma={gamma}: max |hip - float64| = {worst:.3g} (tolerance {ms.TOL[(K, gamma)]:.3g})")
    assert worst <= ms.TOL[(K, gamma)], worst
    bg = torch.tensor(ms.BACKGROUND)
    assert torch.equal(out[~covered][:, :3], bg.expand(int((~covered).sum()), 3)) and float(out[~covered][:, 3].abs().max()) == 0


def _icosphere(levels=2, radius=0.8):
    t = (1 + 5 ** 0.5) / 2
    v = [[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t], [t, 0, -1], [t, 0, 1],
         [-t, 0, -1], [-t, 0, 1]]
    f = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
         [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]]
    v = [torch.tensor(x, dtype=torch.float64) / torch.tensor(x, dtype=torch.float64).norm() for x in v]
    for _ in range(levels):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / p.norm())
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        f = nf
    return (torch.stack(v) * radius).float(), torch.tensor(f, dtype=torch.int64)


def _sphere_obj(tmp_path):
    """an icosphere of 320 faces with a UV triangle of its own per face (an 18 x 18 grid of cells) and a smooth 64 x 64 texture,
    written by save_obj"""
    from pytorch3d.io import save_obj
    verts, faces = _icosphere()
    nF = faces.shape[0]
    assert nF == 320
    cell = torch.arange(nF)
    cx, cy = (cell % 18).double(), (cell // 18).double()
    corners = torch.tensor([[0.1, 0.1], [0.9, 0.15], [0.3, 0.9]], dtype=torch.float64)
    verts_uv = ((torch.stack([cx, cy], dim=-1)[:, None, :] + corners[None]) / 18.0).reshape(-1, 2).float()
    faces_uv = torch.arange(3 * nF).view(nF, 3)
    y, x = torch.meshgrid(torch.linspace(0, 1, 64), torch.linspace(0, 1, 64), indexing="ij")
    tmap = torch.stack([0.5 + 0.45 * torch.sin(9 * x + 2 * y), 0.5 + 0.45 * torch.cos(7 * y - 3 * x), 0.25 + 0.5 * x * y + 0.2 * y], dim=-1)
    path = tmp_path / "sphere.obj"
    save_obj(str(path), verts=verts, faces=faces, verts_uvs=verts_uv, faces_uvs=faces_uv, texture_map=tmap)
    return str(path)


def _orbit(n=3):
    from sugar_amd import synthetic as syn
    from sugar_amd.mesh_render import p3d_camera_from_gs
    return [p3d_camera_from_gs(c, DEV) for c in syn.orbit_cameras(128, 96, n=n, radius=2.5)]


def test_end_to_end_through_the_stand_in(p3d, tmp_path):
    """save_obj -> load_objs_as_meshes -> MeshRenderer(MeshRasterizer(K = 1), SoftPhongShader(AmbientLights, background 0)) under
    no_grad, as metrics.py:268-300, 372: bit-identical to TexturedMeshRenderer.render, and within the K = 1 tolerance of the float64
    reference applied to the same fragments"""
    from pytorch3d.io import load_objs_as_meshes
    from pytorch3d.renderer import AmbientLights, MeshRasterizer, MeshRenderer, RasterizationSettings, SoftPhongShader
    from pytorch3d.renderer.blending import BlendParams
    from sugar_amd.mesh_render import TexturedMeshRenderer
    mesh = load_objs_as_meshes([_sphere_obj(tmp_path)]).to(DEV)
    tex = mesh.textures
    assert tex.sampling_mode == "bilinear" and tex.maps_padded().is_cuda
    cams = _orbit()
    settings = RasterizationSettings(image_size=(96, 128), blur_radius=0.0, faces_per_pixel=1)
    blend = BlendParams(background_color=(0.0, 0.0, 0.0))
    renderer = MeshRenderer(rasterizer=MeshRasterizer(cameras=cams[0], raster_settings=settings),
                            shader=SoftPhongShader(device=DEV, cameras=cams[0], lights=AmbientLights(device=DEV), blend_params=blend))
    own = TexturedMeshRenderer(mesh.verts_list()[0], mesh.faces_list()[0], tex.verts_uvs_list()[0], tex.faces_uvs_list()[0],
                               tex.maps_padded()[0], (96, 128), blend_params=blend)
    for cam in cams:
        with torch.no_grad():
            img = renderer(mesh, cameras=cam)
            frags = renderer.rasterizer(mesh, cameras=cam)
        assert img.shape == (1, 96, 128, 4) and not torch.isnan(img).any()
        mine = own.render(cam)
        assert torch.equal(img[0].view(torch.int32), mine.view(torch.int32))
        covered = frags.pix_to_face[0, ..., 0] >= 0
        assert float(covered.float().mean()) > 0.2
        ref, _ = ms.reference_shade(frags.pix_to_face[0], frags.zbuf[0], frags.bary_coords[0], frags.dists[0], tex.verts_uvs_list()[0],
                                    tex.faces_uvs_list()[0], tex.maps_padded()[0], "bilinear", True, blend.sigma, blend.gamma,
                                    background=(0.0, 0.0, 0.0), znear=float(cam.znear[0]), zfar=float(cam.zfar[0]))
        worst = float((img[0].cpu().double() - ref).abs().max())
        print(f"end to end: max |hip - float64| = {worst:.3g} (tolerance {ms.TOL[(1, 1e-4)]:.3g})")
        assert worst <= ms.TOL[(1, 1e-4)], worst
        # (a pixel centre inside a face has dists <= 0: its coverage probability is at least sigmoid(0))
        assert float(img[0][covered][:, 3].min()) >= 0.5 - 1e-6 and float(img[0][~covered].abs().max()) == 0


def test_repeatable_sync_free_and_stream_ordered(hip_lib):
    for K, mode in ((1, "bilinear"), (3, "nearest"), (3, "bilinear")):
        _dev_scene(K)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            a = _shade(K, mode, True, 1e-4, 1e-4)
            b = _shade(K, mode, True, 1e-4, 1e-4)
        finally:
            torch.cuda.set_sync_debug_mode(0)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            c = _shade(K, mode, True, 1e-4, 1e-4)
        st.synchronize()
        assert torch.equal(a.view(torch.int32), c.view(torch.int32))


def test_face_index_base(hip_lib):
    s = _dev_scene(3)
    shifted = s._replace(pix_to_face=torch.where(s.pix_to_face >= 0, s.pix_to_face + 1000, s.pix_to_face))
    for mode in ms.MODES:
        a = _shade(3, mode, True, 1e-2, 1e-2)
        b = _shade(3, mode, True, 1e-2, 1e-2, s=shifted, face_index_base=1000)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def _ssim64(a, b):
    """mean SSIM of two [3,H,W] images in float64: sugar_utils/loss_utils.py:39-63 (11-tap Gaussian window, sigma 1.5, zero padding)"""
    g = torch.tensor([math.exp(-(x - 5) ** 2 / (2 * 1.5 ** 2)) for x in range(11)], dtype=torch.float64)
    g = g / g.sum()
    w = (g[:, None] @ g[None, :]).expand(3, 1, 11, 11).contiguous()
    conv = lambda t: F.conv2d(t[None], w, padding=5, groups=3)
    mu1, mu2 = conv(a), conv(b)
    s1, s2, s12 = conv(a * a) - mu1 * mu1, conv(b * b) - mu2 * mu2, conv(a * b) - mu1 * mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    return float((((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))).mean())


def test_image_metrics(hip_lib):
    """against itself: PSNR inf, SSIM 1; against a noised copy: SSIM within 5e-6 of the float64 formula (the bar of
    tests/test_gpu_loss.py), PSNR within 1e-4 dB (a float32 mean of 6 k squares is good to a relative 1e-5 at worst, and
    d PSNR = 10 / ln 10 x the relative error of the MSE = 4.3e-5 dB)"""
    from sugar_amd.mesh_render import image_metrics
    img = _shade(1, "bilinear", True, 1e-4, 1e-4)[..., :3].clamp(0, 1).contiguous()
    m = image_metrics(img, img)
    assert m["psnr"] == math.inf and abs(m["ssim"] - 1.0) < 5e-6
    g = torch.Generator().manual_seed(4)
    noisy = (img.cpu() + 0.1 * torch.randn(img.shape, generator=g)).clamp(0, 1)
    m = image_metrics(img, noisy.to(DEV))
    a, b = img.cpu().double().permute(2, 0, 1), noisy.double().permute(2, 0, 1)
    psnr = 20 * math.log10(1.0 / math.sqrt(float(((a - b) ** 2).mean())))
    ssim = _ssim64(a, b)
    print(f"psnr {m['psnr']:.6f} vs {psnr:.6f}; ssim {m['ssim']:.7f} vs {ssim:.7f}")
    assert 10 < psnr < 40 and 0.05 < ssim < 0.99
    assert abs(m["psnr"] - psnr) < 1e-4 and abs(m["ssim"] - ssim) < 5e-6
    chw = image_metrics(img.permute(2, 0, 1).contiguous(), noisy.to(DEV).permute(2, 0, 1).contiguous())
    assert chw == m


def test_a_graph_that_needs_gradients_keeps_the_torch_path(p3d):
    """requires_grad on the texture map: nearest sampling still runs in torch and yields a gradient; bilinear still raises, as before"""
    from pytorch3d.renderer import AmbientLights, FoVPerspectiveCameras, Fragments, SoftPhongShader, TexturesUV
    from pytorch3d.renderer.blending import BlendParams
    from pytorch3d.structures import Meshes
    s = _dev_scene(1)
    fr = Fragments(s.pix_to_face[None], s.zbuf[None], s.bary_coords[None], s.dists[None])
    cams = FoVPerspectiveCameras(znear=ms.ZNEAR, zfar=ms.ZFAR, device=DEV)
    shader = SoftPhongShader(device=DEV, cameras=cams, lights=AmbientLights(device=DEV), blend_params=BlendParams(background_color=ms.BACKGROUND))
    verts = torch.zeros(3, 3, device=DEV)
    tmap = s.texture.clone().requires_grad_(True)
    tex = TexturesUV(maps=tmap[None], faces_uvs=[s.faces_uvs], verts_uvs=[s.verts_uvs], sampling_mode="nearest")
    out = shader(fr, Meshes(verts=[verts], faces=[torch.tensor([[0, 1, 2]], device=DEV)], textures=tex))
    assert out.requires_grad
    out[..., :3].sum().backward()
    assert tmap.grad is not None and float(tmap.grad.abs().sum()) > 0
    with torch.no_grad():                                                 # the same call without a graph: nearest keeps the torch path too
        plain = shader(fr, Meshes(verts=[verts], faces=[torch.tensor([[0, 1, 2]], device=DEV)], textures=tex))
    assert torch.equal(plain, out.detach())
    tex.sampling_mode = "bilinear"
    with pytest.raises(NotImplementedError):
        shader(fr, Meshes(verts=[verts], faces=[torch.tensor([[0, 1, 2]], device=DEV)], textures=tex))
    with torch.no_grad():                                                 # ... and without a graph the same call is served by the kernel
        hip = shader(fr, Meshes(verts=[verts], faces=[torch.tensor([[0, 1, 2]], device=DEV)], textures=tex))
    assert torch.equal(hip[0].view(torch.int32), _shade(1, "bilinear", True, 1e-4, 1e-4).view(torch.int32))
