"""Shared by tests/test_mesh_render_cpu.py and tests/test_gpu_mesh_render.py: a seeded generator of synthetic hard fragments over a small
UV-textured mesh, the float64 reference of the shading, and the tolerances measured with both.

The reference is the stand-in's own `interpolate_face_attributes` and `softmax_rgb_blend` on CPU tensors, with
`F.grid_sample(torch.flip(map, [2]), uv * 2 - 1, mode, align_corners, padding_mode="border")` between them -- the formulation of
shims/pytorch3d/renderer/mesh/shader.py with the sampling mode as a parameter.  It is not code under test.

Scene (the smallest shapes at which the kernel can still go wrong): a 37 x 53 image (no multiple of a block or a wave), K in {1, 3}, 40
faces over 61 shared UV vertices in [-0.15, 1.15]^2 (the border is exercised), a 19 x 23 x 3 texture (non-square: a swapped axis or a
missing flip shows), ~20 % empty slots and three fully empty rows, |dists| log-uniform in [1e-6, 1e-1] (negative), depths sorted in
[0.5, 6]; at K = 3 the second face of 30 % of the pixels lies within 0.02 of the first, so the softmax mixes; four pixels sit at
zfar + 4e-4 (a partial blend into the background) and four at zfar + 1 (background).  Background (0.1, 0.2, 0.3), znear 1e-4, zfar 100."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch
import torch.nn.functional as F

H, W = 37, 53
N_FACES, N_UV = 40, 61
TEX_H, TEX_W = 19, 23
ZNEAR, ZFAR = 1e-4, 100.0
BACKGROUND = (0.1, 0.2, 0.3)
EMPTY_ROWS = (0, 17, 36)
KS = (1, 3)
MODES = ("nearest", "bilinear")
ALIGNS = (True, False)
SIGMA_GAMMA = ((1e-4, 1e-4), (1e-2, 1e-2))
GRID = [(K, mode, ac, sg) for K in KS for mode in MODES for ac in ALIGNS for sg in SIGMA_GAMMA]

# max |float32 CPU reference - float64 CPU reference| over all pixels and channels of `scene(K)`, both sampling modes and both
# align_corners settings, per (K, gamma): measured with `measure_float32_error()` below and rounded up to two digits (DESIGN.md section
# 15).  The K = 3, gamma = 1e-4 figure is a 6e-8 rounding of z_inv divided by gamma.  The GPU tests allow 4x: the device's expf, division
# and sigmoid each differ from the host's by a few ulp.
MEASURED = {(1, 1e-4): 1.8e-6, (1, 1e-2): 1.8e-6, (3, 1e-4): 1.9e-4, (3, 1e-2): 2.2e-6}   # raw: 1.71e-6, 1.71e-6, 1.88e-4, 2.16e-6
TOL = {k: 4 * v for k, v in MEASURED.items()}
HALF_GUARD = 1e-3          # nearest: a pixel with a float64 texel coordinate this close to a half-integer is left out
MAX_LEFT_OUT = 0.02        # ... and at most this share of the covered pixels may be


class Scene(NamedTuple):
    pix_to_face: torch.Tensor   # [H,W,K] int64, -1 = empty
    zbuf: torch.Tensor          # [H,W,K] float32
    bary_coords: torch.Tensor   # [H,W,K,3] float32
    dists: torch.Tensor         # [H,W,K] float32
    verts_uvs: torch.Tensor     # [N_UV,2] float32
    faces_uvs: torch.Tensor     # [N_FACES,3] int64
    texture: torch.Tensor       # [TEX_H,TEX_W,3] float32


_scenes = {}


def scene(K: int) -> Scene:
    """the scene for K faces per pixel (CPU tensors; built once per K and shared: do not write into it)"""
    if K in _scenes:
        return _scenes[K]
    rng = np.random.default_rng(20 + K)
    covered = rng.random((H, W, K)) >= 0.2
    covered = -np.sort(-covered.astype(np.int8), axis=-1) > 0          # covered slots first, as a z-buffer leaves them
    covered[list(EMPTY_ROWS)] = False
    z = np.sort(rng.uniform(0.5, 6.0, (H, W, K)), axis=-1)
    if K > 1:
        close = rng.random((H, W)) < 0.3
        z[..., 1] = np.where(close, z[..., 0] + rng.uniform(0.0, 0.02, (H, W)), z[..., 1])
        z = np.sort(z, axis=-1)
    far = [(3, 5), (9, 50), (20, 20), (30, 1), (5, 40), (12, 12), (25, 33), (35, 52)]
    for i, (y, x) in enumerate(far):
        z[y, x] = (ZFAR + 4e-4 if i < 4 else ZFAR + 1.0) + 1e-4 * np.arange(K)
        covered[y, x, 0] = True
    p2f = np.where(covered, rng.integers(0, N_FACES, (H, W, K)), -1)
    bary = rng.random((H, W, K, 3)) + 0.02
    bary = bary / bary.sum(-1, keepdims=True)
    dists = -np.exp(rng.uniform(np.log(1e-6), np.log(1e-1), (H, W, K)))
    z = np.where(covered, z, -1.0)
    bary = np.where(covered[..., None], bary, -1.0)
    dists = np.where(covered, dists, -1.0)
    verts_uvs = rng.uniform(-0.15, 1.15, (N_UV, 2))
    faces_uvs = rng.integers(0, N_UV, (N_FACES, 3))
    tex = rng.random((TEX_H, TEX_W, 3))
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    s = Scene(torch.from_numpy(p2f.astype(np.int64)), f32(z), f32(bary), f32(dists), f32(verts_uvs),
              torch.from_numpy(faces_uvs.astype(np.int64)), f32(tex))
    _scenes[K] = s
    return s


def _standin():
    from sugar_amd.shims.pytorch3d.renderer.blending import BlendParams, softmax_rgb_blend
    from sugar_amd.shims.pytorch3d.renderer.mesh.rasterizer import Fragments
    from sugar_amd.shims.pytorch3d.renderer.mesh.shader import interpolate_face_attributes
    return BlendParams, softmax_rgb_blend, Fragments, interpolate_face_attributes


def reference_shade(p2f, zbuf, bary, dists, verts_uvs, faces_uvs, texture, mode, align_corners, sigma, gamma, background=BACKGROUND,
                    znear=ZNEAR, zfar=ZFAR, ambient=(1.0, 1.0, 1.0), dtype=torch.float64, face_index_base=0):
    """(rgba[H,W,4], pixel_uvs[H,W,K,2]) in `dtype` on the CPU from fragments [H,W,K](,3) of any device and float dtype"""
    BlendParams, softmax_rgb_blend, Fragments, interpolate_face_attributes = _standin()
    cpu = lambda t: t.detach().cpu()
    p2f = cpu(p2f)
    p2f = torch.where(p2f >= 0, p2f - face_index_base, p2f)
    fr = Fragments(p2f[None], cpu(zbuf)[None].to(dtype), cpu(bary)[None].to(dtype), cpu(dists)[None].to(dtype))
    Hh, Ww, K = p2f.shape
    face_uvs = cpu(verts_uvs).to(dtype)[cpu(faces_uvs)]                                  # [F,3,2]
    uv = interpolate_face_attributes(fr.pix_to_face, fr.bary_coords, face_uvs)          # [1,H,W,K,2]
    grid = uv.permute(0, 3, 1, 2, 4).reshape(K, Hh, Ww, 2) * 2.0 - 1.0
    maps = cpu(texture).to(dtype).permute(2, 0, 1)[None].expand(K, -1, -1, -1)
    texels = F.grid_sample(torch.flip(maps, [2]), grid, mode=mode, align_corners=align_corners, padding_mode="border")
    texels = texels.reshape(1, K, 3, Hh, Ww).permute(0, 3, 4, 1, 2)                      # [1,H,W,K,3]
    colors = torch.tensor(ambient, dtype=dtype) * texels
    out = softmax_rgb_blend(colors, fr, BlendParams(sigma, gamma, background), znear=znear, zfar=zfar)
    return out[0], uv[0]


def reference_scene(K, mode, align_corners, sigma, gamma, dtype=torch.float64):
    s = scene(K)
    return reference_shade(s.pix_to_face, s.zbuf, s.bary_coords, s.dists, s.verts_uvs, s.faces_uvs, s.texture, mode, align_corners,
                           sigma, gamma, dtype=dtype)


def kept_pixels(p2f, pixel_uvs64, tex_h, tex_w, align_corners):
    """nearest sampling: [H,W] bool, False where the float64 unnormalised texel coordinate of a covered face lies within HALF_GUARD of a
    half-integer (float32 may round it to the other texel)"""
    g = pixel_uvs64.double() * 2.0 - 1.0
    near = torch.zeros(p2f.shape, dtype=torch.bool)
    for axis, size in ((0, tex_w), (1, tex_h)):
        c = g[..., axis]
        x = ((c + 1) / 2) * (size - 1) if align_corners else ((c + 1) * size - 1) / 2
        x = x.clamp(0, size - 1)
        near |= ((x - torch.floor(x)) - 0.5).abs() < HALF_GUARD
    return ~(near & (p2f.cpu() >= 0)).any(-1)


def measure_float32_error():
    """{(K, gamma): max |float32 - float64|} over the grid (nearest: over the kept pixels), the figures MEASURED rounds up"""
    worst = {}
    for K, mode, ac, (sigma, gamma) in GRID:
        r64, uv = reference_scene(K, mode, ac, sigma, gamma)
        r32, _ = reference_scene(K, mode, ac, sigma, gamma, dtype=torch.float32)
        d = (r32.double() - r64).abs().amax(-1)
        if mode == "nearest":
            d = d[kept_pixels(scene(K).pix_to_face, uv, TEX_H, TEX_W, ac)]
        worst[(K, gamma)] = max(worst.get((K, gamma), 0.0), float(d.max()))
    return worst


if __name__ == "__main__":
    for K, mode, ac, (sigma, gamma) in GRID:
        r64, uv = reference_scene(K, mode, ac, sigma, gamma)
        r32, _ = reference_scene(K, mode, ac, sigma, gamma, dtype=torch.float32)
        keep = kept_pixels(scene(K).pix_to_face, uv, TEX_H, TEX_W, ac) if mode == "nearest" else torch.ones(H, W, dtype=torch.bool)
        cov = (scene(K).pix_to_face >= 0).any(-1)
        d = (r32.double() - r64).abs().amax(-1)
        print(K, mode, ac, gamma, "max diff %.3g" % float(d[keep].max()), "left out %.2f %%" % (100 * float((~keep & cov).sum()) / float(cov.sum())))
    print(measure_float32_error())
