"""The UV texture of SuGaR's refined mesh on the HIP kernels of csrc/texture.hip (C ABI: sgr_texture_* in include/sugar_raster.h).

`extract_texture_image_and_uv_from_gaussians(rc, square_size, n_sh, texture_with_gaussian_renders)` is a drop-in for the function of
the same name in sugar_scene/sugar_model.py:2464-2677 (called by sugar_extractors/refined_mesh.py:191-219): same signature, checks
and return value `(verts_uv, faces_uv, texture_img)`.  It needs none of pytorch3d's shading classes:
  * the UV layout (`uv_layout`) is integer arithmetic and one division in torch on the host, bit for bit the reference's;
  * the atlas initialisation (the first Gaussian of maximal density per texel -> SH2RGB of its DC feature) is one kernel that never
    materialises the reference's T x s(s-1)/2 x n x 3 intermediates;
  * per training camera: the reference's own Gaussian render (`rc.render_image_gaussian_rasterizer`), the hard mesh z-buffer of
    `sugar_amd.mesh_raster` (K = 1, the stand-in MeshRasterizer's world -> NDC transform and near-plane clip), then claim + apply:
    the nearest-texel lookup of pytorch3d's SoftPhongShader over the index texture, and the reference's averaging update in its
    order.  A texel several pixels of one view map to takes the pixel with the largest row-major index (what the reference's
    index_put_ keeps on the CPU; on a GPU the reference's winner is unspecified).

`TextureBaker` is the layer underneath, for callers that have fragments and renders already.  There is no CPU path: CPU tensors raise.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from . import _lib
from ._call import call, ptr

SH_C0 = 0.28209479177387814

# per-vertex pixel offsets of the six UV corners of a square (bottom triangle: corners 0-2, top triangle: corners 3-5), and the
# corners themselves in units of the square side (sugar_model.py:2500-2535)
_CORNER = ((1, 0), (0, 0), (1, 1), (0, 1), (0, 0), (1, 1))
_OFFSET = ((-2, 1), (2, 1), (-2, -3), (1, -1), (1, 3), (-3, -1))


def squares_per_axis(T: int) -> int:
    """P = int(sqrt(T // 2 + 1) + 1): squares per side of the atlas, two triangles per square"""
    import numpy as np
    return int(np.sqrt(T // 2 + 1) + 1)


def texture_size(T: int, square_size: int) -> int:
    return int(square_size) * squares_per_axis(int(T))


def uv_layout(T: int, s: int, device):
    """(verts_uv[6 P^2, 2] float32, faces_uv[T, 3] int64): triangle t uses UV rows 3t..3t+2 -- corners of half t % 2 of square t // 2
    (row-major over the P x P squares), in texel units, divided by the texture side S = s P."""
    T, s = int(T), int(s)
    P = squares_per_axis(T)
    S = s * P
    # (built on the host and copied: the reference's division is the CPU's correctly rounded one; torch's GPU integer true
    # division rounds differently in the last place)
    sq = torch.arange(P * P)
    base = torch.stack([sq // P, sq % P], dim=-1)                                   # (P^2, 2) int64
    corner = torch.tensor(_CORNER, dtype=torch.int64)
    offset = torch.tensor(_OFFSET, dtype=torch.int64)
    uv = (base[:, None, :] + corner[None]) * s + offset[None]                       # (P^2, 6, 2) int64
    verts_uv = (uv.reshape(-1, 2) / S).to(device)                                   # true division -> float32
    faces_uv = torch.arange(3 * T, device=device).view(T, 3)
    return verts_uv, faces_uv


def _check(cond, msg):
    if not cond:
        raise ValueError(msg)


class TextureBaker:
    """The texture of one surface mesh: construction runs the atlas kernel (the init image), every `bake_view` adds one camera
    (claim + apply; views must be baked in the reference's camera order), `result()` divides by the visit counts.

      verts[V,3], faces[T,3], points[T*n,3] (Gaussian centres, triangle-major), M[T*n,3,3] (`get_covariance(return_full_matrix=True,
      return_sqrt=True, inverse_scales=True)`), features_dc[T*n,3] (rows may be strided, e.g. `sh_coordinates[:, 0]`), n Gaussians
      per triangle, s = square_size."""

    def __init__(self, verts, faces, points, M, features_dc, n: int, s: int):
        for name, t in (("verts", verts), ("faces", faces), ("points", points), ("M", M), ("features_dc", features_dc)):
            if not torch.is_tensor(t) or not t.is_cuda:
                raise RuntimeError(f"TextureBaker: {name} must be a tensor on a ROCm device; there is no CPU fallback")
        n, s = int(n), int(s)
        if s < 3:
            raise ValueError("square_size must be >= 3")
        T = int(faces.shape[0])
        _check(T > 0 and n > 0, "TextureBaker: need at least one face and one Gaussian per face")
        _check(verts.dim() == 2 and verts.shape[1] == 3, "TextureBaker: verts must be [V,3]")
        _check(faces.dim() == 2 and faces.shape[1] == 3, "TextureBaker: faces must be [T,3]")
        _check(points.shape == (T * n, 3), f"TextureBaker: points must be [T*n,3] = [{T * n},3]")
        _check(M.shape == (T * n, 3, 3), f"TextureBaker: M must be [T*n,3,3] = [{T * n},3,3]")
        _check(features_dc.dim() == 2 and features_dc.shape[0] == T * n and features_dc.shape[1] == 3,
               "TextureBaker: features_dc must be [T*n,3]")
        self.device = verts.device
        self.T, self.n, self.s = T, n, s
        lib = _lib.load()
        S = lib.sgr_texture_size(T, s)
        if S < 0:
            raise ValueError(f"TextureBaker: a texture for {T} triangles at square_size {s} exceeds 2^31 texels")
        self.S = S
        f32 = lambda t: t.detach().to(device=self.device, dtype=torch.float32).contiguous()
        self._verts, self._points, self._M = f32(verts), f32(points), f32(M)
        self._faces = faces.detach().to(device=self.device, dtype=torch.int64).contiguous()
        feat = features_dc.detach().to(device=self.device, dtype=torch.float32)
        if feat.stride(1) != 1 or feat.stride(0) < 3:
            feat = feat.contiguous()
        self.verts_uv, self.faces_uv = uv_layout(T, s, self.device)
        self._verts_uv = self.verts_uv.contiguous()
        self.texture = torch.empty(S, S, 3, dtype=torch.float32, device=self.device)
        self.counter = torch.empty(S, S, dtype=torch.float32, device=self.device)
        self._winner = torch.empty(S, S, dtype=torch.int64, device=self.device)   # uint64 tags, stored as int64 bits
        self._feat = feat
        self.reset()

    def reset(self) -> None:
        """(re)start baking: the atlas kernel writes the init image and clears the counters and the winner tags"""
        self.view = 0
        call("sgr_texture_atlas", self.device, self.T, self.n, self.s, int(self._verts.shape[0]), ptr(self._verts), ptr(self._faces),
             ptr(self._points), ptr(self._M), ptr(self._feat), int(self._feat.stride(0)), self.S, ptr(self.texture), ptr(self.counter),
             ptr(self._winner))

    def bake_view(self, fragments, rgb: torch.Tensor, znear: float, zfar: float) -> None:
        """fragments: a pytorch3d-style `Fragments` (or the tuple pix_to_face, zbuf, bary_coords, dists) of ONE image at K = 1,
        shapes [1,H,W,1](,3) or [H,W](,3); rgb[H,W,3] float32 on the device (any strides; the reference clamps it to [0,1] first);
        znear / zfar: the camera's, as Python floats.  Enqueues two kernels; no host synchronisation."""
        p2f, zbuf, bary, dists = (fragments.pix_to_face, fragments.zbuf, fragments.bary_coords, fragments.dists) \
            if hasattr(fragments, "pix_to_face") else tuple(fragments)
        if bary is None or dists is None:
            raise ValueError("bake_view needs the fragments' bary_coords and dists")
        H, W = int(rgb.shape[0]), int(rgb.shape[1])
        n_pix = H * W
        for name, t, per in (("pix_to_face", p2f, 1), ("zbuf", zbuf, 1), ("bary_coords", bary, 3), ("dists", dists, 1)):
            if not torch.is_tensor(t) or not t.is_cuda:
                raise RuntimeError(f"bake_view: {name} must be a tensor on a ROCm device; there is no CPU fallback")
            _check(t.numel() == n_pix * per, f"bake_view: {name} must hold one entry per pixel of a {H}x{W} image at K = 1")
        if not torch.is_tensor(rgb) or not rgb.is_cuda:
            raise RuntimeError("bake_view: rgb must be a tensor on a ROCm device; there is no CPU fallback")
        _check(rgb.dim() == 3 and rgb.shape[2] == 3 and rgb.dtype == torch.float32, "bake_view: rgb must be float32 [H,W,3]")
        _check(p2f.dtype == torch.int64, "bake_view: pix_to_face must be int64")
        if torch.is_tensor(znear) or torch.is_tensor(zfar):
            if (torch.is_tensor(znear) and znear.is_cuda) or (torch.is_tensor(zfar) and zfar.is_cuda):
                raise TypeError("bake_view: pass znear / zfar as Python floats (reading a device tensor would synchronise)")
        p2f, zbuf, bary, dists = (t.contiguous() for t in (p2f, zbuf, bary, dists))
        _check(zbuf.dtype == torch.float32 and bary.dtype == torch.float32 and dists.dtype == torch.float32,
               "bake_view: zbuf, bary_coords and dists must be float32")
        sh, sw, sc = (int(x) for x in rgb.stride())
        call("sgr_texture_bake_view", self.device, W, H, self.view, ptr(p2f), ptr(bary), ptr(zbuf), ptr(dists), float(znear), float(zfar),
             self.T, ptr(self._verts_uv), ptr(rgb), sh, sw, sc, self.S, ptr(self._winner), ptr(self.texture), ptr(self.counter))
        self.view += 1

    def result(self) -> torch.Tensor:
        """texture / counter.clamp(min=1): [S,S,3] float32 (the init image where no view reached a texel)"""
        out = torch.empty_like(self.texture)
        call("sgr_texture_finalize", self.device, self.S, ptr(self.texture), ptr(self.counter), ptr(out))
        return out


class MeshFragments(NamedTuple):
    pix_to_face: torch.Tensor
    zbuf: torch.Tensor
    bary_coords: torch.Tensor
    dists: torch.Tensor


def project_verts(camera, verts: torch.Tensor) -> torch.Tensor:
    """world -> NDC x, y with view-space z: the vertex transform of pytorch3d's MeshRasterizer for a single camera"""
    view = camera.get_world_to_view_transform().transform_points(verts)
    ndc = camera.get_projection_transform().transform_points(view)
    return torch.cat([ndc[..., :2], view[..., 2:3]], dim=-1)


def rasterize_mesh(face_verts: torch.Tensor, image_size, znear: float, perspective_correct: bool = True,
                   faces_per_pixel: int = 1) -> MeshFragments:
    """hard z-buffer (K = faces_per_pixel; the baking uses 1) of one mesh's NDC face verts with the near-plane clip of a perspective
    camera (z = znear / 2), as the stand-in MeshRasterizer runs it; the common case (nothing to clip) passes plain lists to the rasterizer"""
    from .mesh_raster import rasterize_face_verts
    from .shims.pytorch3d.renderer.mesh.clip import ClipFrustum, clip_faces, convert_clipped_rasterization_to_original_faces
    F_ = int(face_verts.shape[0])
    dev = face_verts.device
    z_clip = None if znear is None else float(znear) / 2
    clipped = None
    if z_clip is not None:
        frustum = ClipFrustum(left=-1, right=1, top=-1, bottom=1, perspective_correct=perspective_correct, cull=False,
                              z_clip_value=z_clip)
        clipped = clip_faces(face_verts, torch.zeros(1, dtype=torch.int64, device=dev), torch.full((1,), F_, dtype=torch.int64, device=dev),
                             frustum)
        if clipped.faces_clipped_to_unclipped_idx is None:
            clipped = None
    if clipped is None:
        p2f, zbuf, bary, dists = rasterize_face_verts(face_verts, [0], [F_], image_size, 0.0, faces_per_pixel, perspective_correct, False,
                                                      False)
    else:
        p2f, zbuf, bary, dists = rasterize_face_verts(clipped.face_verts, [0], [int(clipped.face_verts.shape[0])], image_size, 0.0,
                                                      faces_per_pixel, perspective_correct, False, False)
        p2f, bary = convert_clipped_rasterization_to_original_faces(p2f, bary, clipped)
    return MeshFragments(p2f, zbuf, bary, dists)


def _camera_planes(p3d_cameras, n_views):
    """(znear, zfar) of every training camera as Python floats, read once"""
    zn, zf = getattr(p3d_cameras, "znear", None), getattr(p3d_cameras, "zfar", None)
    conv = lambda z, d: ([float(x) for x in z.reshape(-1).tolist()] if torch.is_tensor(z) else [float(z)]) if z is not None else [d]
    zn, zf = conv(zn, 1.0), conv(zf, 100.0)
    zn = zn * n_views if len(zn) == 1 else zn
    zf = zf * n_views if len(zf) == 1 else zf
    return zn, zf


def extract_texture_image_and_uv_from_gaussians(rc, square_size: int = 10, n_sh=-1, texture_with_gaussian_renders=True):
    """Drop-in for sugar_scene/sugar_model.py:2464-2677 on the HIP kernels.  Returns (verts_uv[6P^2,2], faces_uv[T,3],
    texture_img[S,S,3]).  Only n_sh = 1 (or -1 on a degree-0 model) is supported -- the only case the reference itself completes."""
    if square_size < 3:
        raise ValueError("square_size must be >= 3")
    mesh = rc.surface_mesh
    verts = mesh.verts_list()[0]
    faces = mesh.faces_list()[0]
    n = int(rc.n_gaussians_per_surface_triangle)
    sh = rc.sh_coordinates
    if n_sh == -1:
        n_sh = int(sh.shape[1])
    if n_sh != 1:
        raise ValueError(f"n_sh = {n_sh}: the texture holds the DC colour only (n_sh must be 1, or -1 on a degree-0 model)")
    if not verts.is_cuda:
        raise RuntimeError("extract_texture_image_and_uv_from_gaussians needs the model on a ROCm device; there is no CPU fallback")
    T = int(faces.shape[0])
    with torch.no_grad():
        M = rc.get_covariance(return_full_matrix=True, return_sqrt=True, inverse_scales=True)
        baker = TextureBaker(verts, faces, rc.points.reshape(-1, 3), M.reshape(-1, 3, 3), sh[:, 0], n, square_size)
        cams = rc.nerfmodel.training_cameras
        n_views = len(cams)
        p3d = cams.p3d_cameras
        znear, zfar = _camera_planes(p3d, n_views)
        H, W = int(rc.image_height), int(rc.image_width)
        faces_l = faces.to(device=verts.device, dtype=torch.int64)
        for c in range(n_views):
            rgb = rc.render_image_gaussian_rasterizer(camera_indices=c, sh_deg=0, compute_color_in_rasterizer=True).clamp(min=0, max=1)
            cam = p3d[c]
            fv = project_verts(cam, verts)[faces_l]
            persp = bool(cam.is_perspective()) if hasattr(cam, "is_perspective") else True
            frags = rasterize_mesh(fv.float(), (H, W), znear[c] if persp else None, persp)
            baker.bake_view(frags, rgb.float(), znear[c], zfar[c])
        return baker.verts_uv, baker.faces_uv, baker.result()
