"""GPU tests of the refined mesh's UV texture on the HIP kernels (csrc/texture.hip via sugar_amd.texture) against the fixture the
reference's own `extract_texture_image_and_uv_from_gaussians` wrote on the CPU (tests/golden/make_sugar_texture.py), and at
BASELINE config 4 size against an independent torch formulation of the baking loop.  The reference is never imported here."""
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sugar_texture.npz")
C0 = np.float32(0.28209479177387814)


class _Golden:
    """tests/golden/sugar_texture.npz by the names the tests use: "n1_" / "n6_" + key, where the mesh, the cameras, the UV layout and
    the counters are stored once for both models, and "<model>texture" is the reference's final texture (the visited texels
    recorded, the init value everywhere else)"""
    def __init__(self, path):
        self.d = np.load(path)

    def __getitem__(self, key):
        if key in self.d.files:
            return self.d[key]
        pre, base = key[:3], key[3:]
        if base == "texture":
            return np.where(self.d["counter"][..., None] > 0, self.d[pre + "texture_visited"], self.d[pre + "texture_init"])
        return self.d[base]


@pytest.fixture(scope="module")
def gold():
    return _Golden(GOLDEN)


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _baker(gold, pre):
    from sugar_amd.texture import TextureBaker
    T = gold[pre + "faces"].shape[0]
    n = gold[pre + "points"].shape[0] // T
    return TextureBaker(_dev(gold[pre + "verts"]), _dev(gold[pre + "faces"]), _dev(gold[pre + "points"]), _dev(gold[pre + "M"]),
                        _dev(gold[pre + "features_dc"]), n, int(gold["square_size"]))


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("pre", ["n1_", "n6_"])
def test_baking_is_bit_identical_to_the_reference(hip_lib, gold, pre):
    """the fixture's NDC face verts through the HIP z-buffer (bit-exact to the oracle), the fixture's renders baked: the counters and
    every visited texel equal the reference's bit for bit"""
    from sugar_amd.texture import rasterize_mesh
    H, W = int(gold["H"]), int(gold["W"])
    b = _baker(gold, pre)
    for c in range(gold[pre + "rgb"].shape[0]):
        fr = rasterize_mesh(_dev(gold[pre + "face_verts_ndc"][c]), (H, W), float(gold[pre + "znear"][c]))
        b.bake_view(fr, _dev(gold[pre + "rgb"][c]), float(gold[pre + "znear"][c]), float(gold[pre + "zfar"][c]))
    tex = b.result().cpu().numpy()
    cnt = b.counter.cpu().numpy()
    assert _bits_equal(cnt, gold[pre + "counter"])
    seen = gold[pre + "counter"] > 0
    assert seen.sum() > 1000
    assert _bits_equal(tex[seen], gold[pre + "texture"][seen])


def test_atlas_n1_is_bit_identical(hip_lib, gold):
    tex = _baker(gold, "n1_").result().cpu().numpy()
    assert _bits_equal(tex, gold["n1_texture_init"])


def _owner(T, s, S):
    """triangle owning every texel of the final [S,S] image (-1: nobody) and its barycentrics, in float64"""
    r, c = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    i, j = c, S - 1 - r
    P = S // s
    di, dj = i % s, j % s
    sq = (i // s) * P + (j // s)
    half = np.where((di <= s - 2) & (dj <= di), 0, np.where(dj >= di + 1, 1, -1))
    t = np.where(half >= 0, 2 * sq + half, -1)
    t = np.where(t < T, t, -1)
    b1 = np.where(half == 0, s - 2 - di, di - 1) / (s - 3)
    b2 = np.where(half == 0, dj - 1, s - 1 - dj) / (s - 3)
    return t, np.stack([1 - (b1 + b2), b1, b2], axis=-1)


def test_atlas_n6_chooses_the_densest_gaussian(hip_lib, gold):
    """n = 6: the chosen Gaussian is the fixture's on >= 99.9 % of owned texels, anywhere else both choices are within
    1e-3 (1 + q_min) of the smallest float64 q; every texel is SH2RGB of one of its triangle's features, bit for bit"""
    pre = "n6_"
    s = int(gold["square_size"])
    tex = _baker(gold, pre).result().cpu().numpy()
    ref = gold[pre + "texture_init"]
    S = tex.shape[0]
    faces, verts = gold[pre + "faces"], gold[pre + "verts"].astype(np.float64)
    T = faces.shape[0]
    n = gold[pre + "points"].shape[0] // T
    t, bary = _owner(T, s, S)
    assert _bits_equal(tex[t < 0], ref[t < 0]) and np.all(tex[t < 0] == 0.5)
    feats = gold[pre + "features_dc"].reshape(T, n, 3)
    cand = feats * C0 + np.float32(0.5)                                       # (T, n, 3) float32, SH2RGB of every candidate
    own = np.nonzero(t >= 0)
    tt = t[own]

    def choice(img):
        v = img[own]
        hit = np.all(cand[tt] == v[:, None, :], axis=-1)                     # (N, n)
        assert hit.any(axis=-1).all(), "a texel is not SH2RGB of one of its triangle's features"
        return hit.argmax(axis=-1)
    g_hip, g_ref = choice(tex), choice(ref)
    same = g_hip == g_ref
    assert same.mean() >= 0.999, same.mean()
    x = np.einsum("nk,nkc->nc", bary[own], verts[faces[tt]])
    pts = gold[pre + "points"].astype(np.float64).reshape(T, n, 3)[tt]
    M = gold[pre + "M"].astype(np.float64).reshape(T, n, 3, 3)[tt]
    w = np.einsum("ngki,ngk->ngi", M, x[:, None, :] - pts)
    q = np.clip((w * w).sum(-1), 0, 1e8)
    qmin = q.min(-1)
    for k in np.nonzero(~same)[0]:
        for g in (g_hip[k], g_ref[k]):
            assert q[k, g] - qmin[k] <= 1e-3 * (1 + qmin[k]), (k, g, q[k], qmin[k])


class _Mesh:
    def __init__(self, v, f):
        self.v, self.f = v, f

    def verts_list(self):
        return [self.v]

    def faces_list(self):
        return [self.f]


def _duck_rc(gold, pre, sh_rows=1):
    from sugar_amd import shims
    shims.install()
    from pytorch3d.renderer import FoVPerspectiveCameras
    T = gold[pre + "faces"].shape[0]
    rgb = _dev(gold[pre + "rgb"])
    cams = FoVPerspectiveCameras(R=_dev(gold[pre + "R"]), T=_dev(gold[pre + "T"]), K=_dev(gold[pre + "K"]), znear=_dev(gold[pre + "znear"]),
                                 zfar=_dev(gold[pre + "zfar"]), device=DEV)
    training = type("TrainingCameras", (), {"__len__": lambda self: rgb.shape[0], "p3d_cameras": cams})()
    feats = _dev(gold[pre + "features_dc"])
    sh = torch.cat([feats[:, None], torch.zeros(feats.shape[0], sh_rows - 1, 3, device=DEV)], dim=1)
    M = _dev(gold[pre + "M"])
    calls = []

    def render(camera_indices, sh_deg, compute_color_in_rasterizer):
        assert sh_deg == 0 and compute_color_in_rasterizer
        calls.append(camera_indices)
        return rgb[camera_indices].transpose(0, 1).contiguous().transpose(0, 1)   # a strided [H,W,3] view, as the reference returns
    rc = types.SimpleNamespace(surface_mesh=_Mesh(_dev(gold[pre + "verts"]), _dev(gold[pre + "faces"])),
                               n_gaussians_per_surface_triangle=gold[pre + "points"].shape[0] // T, sh_coordinates=sh,
                               points=_dev(gold[pre + "points"]), get_covariance=lambda **k: M, nerfmodel=types.SimpleNamespace(
                                   training_cameras=training), image_height=int(gold["H"]), image_width=int(gold["W"]),
                               render_image_gaussian_rasterizer=render, device=torch.device(DEV))
    return rc, calls


@pytest.mark.parametrize("pre", ["n1_", "n6_"])
def test_drop_in_function_end_to_end(hip_lib, gold, pre):
    from sugar_amd.texture import extract_texture_image_and_uv_from_gaussians
    rc, calls = _duck_rc(gold, pre)
    verts_uv, faces_uv, tex = extract_texture_image_and_uv_from_gaussians(rc, square_size=int(gold["square_size"]), n_sh=1)
    assert calls == list(range(gold[pre + "rgb"].shape[0]))
    assert _bits_equal(verts_uv.cpu().numpy(), gold[pre + "verts_uv"]) and np.array_equal(faces_uv.cpu().numpy(), gold[pre + "faces_uv"])
    tex = tex.cpu().numpy()
    same = np.all(tex.view(np.uint32) == gold[pre + "texture"].view(np.uint32), axis=-1)
    assert same.mean() >= 0.999, same.mean()


def _texel_torch(fr, verts_uv, S, znear, zfar):
    """contract item 4 as torch operations on the device: the texel of every covered pixel ([H*W], -1 = none).  Divisors are device
    tensors: torch turns a division by a Python scalar on the GPU into a multiplication by its rounded reciprocal."""
    p2f = fr.pix_to_face.reshape(-1)
    zb = fr.zbuf.reshape(-1)
    bary = fr.bary_coords.reshape(-1, 3)
    d = fr.dists.reshape(-1)
    f = p2f.clamp(min=0)
    uv = verts_uv[(3 * f)[:, None] + torch.arange(3, device=DEV)]          # [N,3,2]
    u = bary[:, 0] * uv[:, 0, 0]
    u = u + bary[:, 1] * uv[:, 1, 0]
    u = u + bary[:, 2] * uv[:, 2, 0]
    v = bary[:, 0] * uv[:, 0, 1]
    v = v + bary[:, 1] * uv[:, 1, 1]
    v = v + bary[:, 2] * uv[:, 2, 1]
    mx = torch.tensor(float(S - 1), device=DEV)
    hs = mx / 2
    col = torch.round(torch.minimum(mx, torch.clamp((u * 2 - 1 + 1) * hs, min=0)))
    row = torch.round(torch.minimum(mx, torch.clamp((v * 2 - 1 + 1) * hs, min=0)))
    sig = torch.tensor(1e-4, device=DEV)
    one = torch.ones_like(d)
    prob = one / (1 + torch.exp(-((-d) / sig)))
    zi = (zfar - zb) / (torch.tensor(zfar, device=DEV) - torch.tensor(znear, device=DEV))
    zmax = zi.clamp(min=1e-10)
    w = prob * torch.exp((zi - zmax) / sig)
    den = w + torch.exp((1e-10 - zmax) / sig).clamp(min=1e-10)
    a = torch.round((w * (mx - row)) / den)
    b = torch.round((w * col) / den)
    ok = (zb > 0) & (p2f >= 0)
    return torch.where(ok, a.long() * S + b.long(), torch.full_like(p2f, -1))


def test_config4_size_matches_an_independent_torch_formulation(hip_lib):
    """make_bound_scene(1M, n = 1), s = 10 (S = 7 080), 8 views at 1080p: bit-identical to a torch restatement whose duplicate rule
    is scatter_reduce('amax') of the pixel index per texel; two runs identical; bake_view never synchronises"""
    import sys
    from sugar_amd import synthetic as syn
    from sugar_amd.field import scaled_rotation
    from sugar_amd.texture import TextureBaker, project_verts, rasterize_mesh
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_sugar_field as mf
    bs = syn.make_bound_scene(1_000_000, 5, n_per_triangle=1)
    verts, faces = bs.verts.to(DEV), bs.faces.to(DEV)
    sc = bs.scene
    M = scaled_rotation(sc.rotations.to(DEV), sc.scales.to(DEV), inverse_scales=True)
    feats = sc.shs[:, 0].to(DEV)
    W, H = 1920, 1080
    cams = mf.p3d_cameras_like_the_reference(syn.orbit_cameras(W, H, n=8, radius=2.6)).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(3)
    frags, rgbs = [], []
    for c in range(8):
        fv = project_verts(cams[c], verts)[faces]
        frags.append(rasterize_mesh(fv, (H, W), 1e-4))
        rgbs.append(torch.rand(H, W, 3, device=DEV, generator=g))
    zn, zf = float(cams.znear[0]), float(cams.zfar[0])

    def bake():
        b = TextureBaker(verts, faces, sc.means3D.to(DEV), M, feats, 1, 10)
        init = b.texture.clone()
        torch.cuda.set_sync_debug_mode("error")
        try:
            for c in range(8):
                b.bake_view(frags[c], rgbs[c], zn, zf)
        finally:
            torch.cuda.set_sync_debug_mode(0)
        return b, init, b.result()
    b, init, out1 = bake()
    assert b.S == 7080
    _, _, out2 = bake()
    assert torch.equal(out1.view(torch.int32), out2.view(torch.int32))
    S = b.S
    tex = init.reshape(-1, 3).clone()
    cnt = torch.zeros(S * S, device=DEV)
    visited = 0
    for c in range(8):
        t = _texel_torch(frags[c], b.verts_uv, S, zn, zf)
        pix = torch.arange(t.numel(), device=DEV)
        ok = t >= 0
        tv, pv = t[ok], pix[ok]
        win = torch.full((S * S,), -1, dtype=torch.int64, device=DEV).scatter_reduce(0, tv, pv, "amax")
        keep = win[tv] == pv
        tt, pp = tv[keep], pv[keep]
        old = tex[tt]
        tex[tt] = torch.where((cnt[tt] != 0)[:, None], old, torch.zeros_like(old)) + rgbs[c].reshape(-1, 3)[pp]
        cnt[tt] += 1
        visited += int(tt.numel())
    assert visited > 1_000_000
    ref = tex / cnt.clamp(min=1)[:, None]
    n_cnt = int((b.counter.reshape(-1) != cnt).sum())
    assert n_cnt == 0, f"{n_cnt} counters differ"
    n_tex = int((out1.reshape(-1, 3).view(torch.int32) != ref.view(torch.int32)).any(-1).sum())
    assert n_tex == 0, f"{n_tex} texels differ"


def test_bad_inputs_raise(hip_lib, gold):
    from sugar_amd.texture import TextureBaker, extract_texture_image_and_uv_from_gaussians
    rc, _ = _duck_rc(gold, "n1_", sh_rows=4)
    with pytest.raises(ValueError):
        extract_texture_image_and_uv_from_gaussians(rc, square_size=10, n_sh=4)
    with pytest.raises(ValueError):
        extract_texture_image_and_uv_from_gaussians(rc, square_size=10)      # n_sh = -1 on a degree-1 model
    with pytest.raises(ValueError):
        extract_texture_image_and_uv_from_gaussians(rc, square_size=2, n_sh=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        TextureBaker(torch.zeros(3, 3), torch.tensor([[0, 1, 2]]), torch.zeros(1, 3), torch.zeros(1, 3, 3), torch.zeros(1, 3), 1, 10)
    b = _baker(gold, "n1_")
    H, W = int(gold["H"]), int(gold["W"])
    with pytest.raises(ValueError):          # fragments of another image size
        b.bake_view((torch.zeros(1, H, W - 1, 1, dtype=torch.int64, device=DEV), torch.zeros(1, H, W - 1, 1, device=DEV),
                     torch.zeros(1, H, W - 1, 1, 3, device=DEV), torch.zeros(1, H, W - 1, 1, device=DEV)),
                    torch.zeros(H, W, 3, device=DEV), 1e-4, 100.0)
