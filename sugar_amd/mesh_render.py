"""Rendering and scoring of the UV-textured refined mesh on the HIP kernel of csrc/mesh_shade.hip (C ABI: sgr_shade_texture_uv in
include/sugar_raster.h): what the reference's `metrics.py --use_uv_texture` leg does through pytorch3d's
`MeshRenderer(MeshRasterizer(K = 1), SoftPhongShader(AmbientLights, background 0))` (metrics.py:260-300, 370-372).

  * `shade_textured` shades the hard fragments of one view of one mesh: UV interpolation, `grid_sample` of the y-flipped map ('nearest'
    or 'bilinear', padding_mode 'border') read in place, colour = ambient x texel, `softmax_rgb_blend` -- one launch, no host
    synchronisation.  It restates the stand-in `SoftPhongShader` (shims/pytorch3d/renderer/mesh/shader.py) operation by operation.
  * `TexturedMeshRenderer` chains the vertex transform, the HIP z-buffer (`sugar_amd.texture.rasterize_mesh`) and `shade_textured`.
  * `image_metrics` gives PSNR (gaussian_splatting/utils/image_utils.py:17-19, in torch) and SSIM (the fused kernels of
    `sugar_amd.fused_loss`).  There is no LPIPS: it needs VGG weights that are not shipped with this package.

There is no CPU path: CPU tensors raise.  Gradients do not flow through the shader."""
from __future__ import annotations

import torch

from . import _lib
from ._call import call, need_gpu, ptr
from .mesh_raster import MAX_FACES_PER_PIXEL


def _check(cond, msg):
    if not cond:
        raise ValueError(msg)


def _host_floats(x, n, name):
    """n Python floats of a sequence, a scalar or a host tensor; a device tensor raises (reading it would synchronise)"""
    if torch.is_tensor(x):
        if x.is_cuda:
            raise TypeError(f"shade_textured: pass {name} as Python floats or a CPU tensor (reading a device tensor would synchronise)")
        x = x.reshape(-1).tolist()
    elif not isinstance(x, (list, tuple)):
        x = [x]
    x = [float(v) for v in x]
    _check(len(x) == n, f"shade_textured: {name} must hold {n} value{'s' if n > 1 else ''}")
    return x


def _fragment_tensors(fragments):
    if hasattr(fragments, "pix_to_face"):
        return fragments.pix_to_face, fragments.zbuf, fragments.bary_coords, fragments.dists
    fragments = tuple(fragments)
    _check(len(fragments) == 4, "shade_textured: fragments must be (pix_to_face, zbuf, bary_coords, dists)")
    return fragments


def shade_textured(fragments, verts_uvs, faces_uvs, texture_map, *, sampling_mode="bilinear", align_corners=True, padding_mode="border",
                   blend_params=None, znear, zfar, ambient=(1.0, 1.0, 1.0), face_index_base=0) -> torch.Tensor:
    """RGBA [H,W,4] float32 of one view of one mesh.

    fragments: `sugar_amd.texture.MeshFragments`, the stand-in pytorch3d `Fragments`, or the tuple (pix_to_face, zbuf, bary_coords,
      dists), of shapes [1,H,W,K](,3) or [H,W,K](,3) with 1 <= K <= 16; pix_to_face int64, the rest float32; a covered slot names face
      `pix_to_face - face_index_base` of `faces_uvs` (a packed batch of meshes numbers its faces through).
    verts_uvs[n_uv,2] float32, faces_uvs[F,3] int64, texture_map[TH,TW,3] float32 as stored (row 0 is v = 1).  An index outside its
      array gives NaN at that pixel; indices that come from `pytorch3d.io.load_obj` are validated there.
    blend_params: a `BlendParams` (sigma, gamma, background_color; default `BlendParams()`); znear / zfar / ambient / the background:
      Python floats or CPU tensors."""
    if sampling_mode not in ("nearest", "bilinear"):
        raise ValueError(f"shade_textured: sampling_mode must be 'nearest' or 'bilinear', got {sampling_mode!r}")
    if padding_mode != "border":
        raise NotImplementedError(f"shade_textured: padding_mode {padding_mode!r} is not implemented (TexturesUV's default 'border' is)")
    if blend_params is None:
        from .shims.pytorch3d.renderer.blending import BlendParams
        blend_params = BlendParams()
    p2f, zbuf, bary, dists = _fragment_tensors(fragments)
    if bary is None or dists is None:
        raise ValueError("shade_textured needs the fragments' bary_coords and dists")
    tensors = dict(pix_to_face=p2f, zbuf=zbuf, bary_coords=bary, dists=dists, verts_uvs=verts_uvs, faces_uvs=faces_uvs,
                   texture_map=texture_map)
    for name, t in tensors.items():
        if not torch.is_tensor(t):
            raise TypeError(f"shade_textured: {name} must be a tensor")
    if p2f.dim() == 4:
        _check(p2f.shape[0] == 1, "shade_textured: fragments of one view ([1,H,W,K]); loop over a batch")
        p2f, zbuf, bary, dists = p2f[0], zbuf[0] if zbuf.dim() == 4 else zbuf, bary[0] if bary.dim() == 5 else bary, \
            dists[0] if dists.dim() == 4 else dists
    _check(p2f.dim() == 3, "shade_textured: pix_to_face must be [1,H,W,K] or [H,W,K]")
    H, W, K = (int(x) for x in p2f.shape)
    _check(H > 0 and W > 0, "shade_textured: empty image")
    _check(1 <= K <= MAX_FACES_PER_PIXEL, f"shade_textured: faces per pixel must be in 1..{MAX_FACES_PER_PIXEL}, got {K}")
    _check(tuple(zbuf.shape) == (H, W, K) and tuple(dists.shape) == (H, W, K) and tuple(bary.shape) == (H, W, K, 3),
           f"shade_textured: zbuf, dists must be [{H},{W},{K}] and bary_coords [{H},{W},{K},3]")
    _check(p2f.dtype == torch.int64, "shade_textured: pix_to_face must be int64")
    _check(zbuf.dtype == torch.float32 and bary.dtype == torch.float32 and dists.dtype == torch.float32,
           "shade_textured: zbuf, bary_coords and dists must be float32")
    _check(verts_uvs.dim() == 2 and verts_uvs.shape[1] == 2 and verts_uvs.shape[0] > 0 and verts_uvs.dtype == torch.float32,
           "shade_textured: verts_uvs must be float32 [n_uv,2]")
    _check(faces_uvs.dim() == 2 and faces_uvs.shape[1] == 3 and faces_uvs.shape[0] > 0 and faces_uvs.dtype == torch.int64,
           "shade_textured: faces_uvs must be int64 [F,3]")
    _check(texture_map.dim() == 3 and texture_map.shape[2] == 3 and texture_map.shape[0] > 0 and texture_map.shape[1] > 0
           and texture_map.dtype == torch.float32, "shade_textured: texture_map must be float32 [TH,TW,3]")
    need_gpu("shade_textured", **tensors)
    dev = p2f.device
    for name, t in (("verts_uvs", verts_uvs), ("faces_uvs", faces_uvs), ("texture_map", texture_map)):
        _check(t.device == dev, f"shade_textured: {name} is on {t.device}, the fragments on {dev}")
    amb = _host_floats(ambient, 3, "ambient")
    bg = _host_floats(blend_params.background_color, 3, "blend_params.background_color")
    zn, zf = _host_floats(znear, 1, "znear")[0], _host_floats(zfar, 1, "zfar")[0]
    c3 = _lib.C.c_float * 3
    p2f, zbuf, bary, dists = (t.detach().contiguous() for t in (p2f, zbuf, bary, dists))
    verts_uvs, faces_uvs, texture_map = (t.detach().contiguous() for t in (verts_uvs, faces_uvs, texture_map))
    out = torch.empty(H, W, 4, dtype=torch.float32, device=dev)
    call("sgr_shade_texture_uv", dev, W, H, K, int(face_index_base), ptr(p2f), ptr(bary), ptr(zbuf), ptr(dists), int(faces_uvs.shape[0]),
         ptr(faces_uvs), int(verts_uvs.shape[0]), ptr(verts_uvs), ptr(texture_map), int(texture_map.shape[0]), int(texture_map.shape[1]),
         int(sampling_mode == "bilinear"), int(bool(align_corners)), c3(*amb), c3(*bg), float(blend_params.sigma),
         float(blend_params.gamma), zn, zf, ptr(out))
    return out


class TexturedMeshRenderer:
    """One textured mesh, drawn at one camera per `render` call: the vertex transform of pytorch3d's MeshRasterizer, the hard HIP z-buffer
    with the near-plane clip of a perspective camera, `shade_textured`.

      verts[V,3] float32, faces[F,3], verts_uvs[n_uv,2], faces_uvs[F,3], texture_map[TH,TW,3] on a ROCm device; image_size (H, W);
      shade_kwargs: `shade_textured`'s keywords (sampling_mode, align_corners, blend_params, ambient, and znear / zfar to override
      the camera's).
    `render(camera)` takes a single pytorch3d-style camera (the stand-in `FoVPerspectiveCameras` of length 1) and returns [H,W,4]."""

    def __init__(self, verts, faces, verts_uvs, faces_uvs, texture_map, image_size, faces_per_pixel: int = 1, **shade_kwargs):
        need_gpu("TexturedMeshRenderer", verts=verts, faces=faces, verts_uvs=verts_uvs, faces_uvs=faces_uvs, texture_map=texture_map)
        _check(verts.dim() == 2 and verts.shape[1] == 3, "TexturedMeshRenderer: verts must be [V,3]")
        _check(faces.dim() == 2 and faces.shape[1] == 3, "TexturedMeshRenderer: faces must be [F,3]")
        _check(faces_uvs.shape == faces.shape, "TexturedMeshRenderer: faces_uvs must have one row per face")
        _check(1 <= int(faces_per_pixel) <= MAX_FACES_PER_PIXEL, f"TexturedMeshRenderer: faces_per_pixel must be in 1..{MAX_FACES_PER_PIXEL}")
        self.image_size = (int(image_size), int(image_size)) if isinstance(image_size, int) else (int(image_size[0]), int(image_size[1]))
        self.faces_per_pixel = int(faces_per_pixel)
        self.verts = verts.detach().float()
        self.faces = faces.detach().to(torch.int64)
        self.verts_uvs = verts_uvs.detach().float().contiguous()
        self.faces_uvs = faces_uvs.detach().to(torch.int64).contiguous()
        self.texture_map = texture_map.detach().float().contiguous()
        self.shade_kwargs = shade_kwargs

    def fragments(self, camera):
        from .texture import project_verts, rasterize_mesh
        persp = bool(camera.is_perspective()) if hasattr(camera, "is_perspective") else True
        znear = _camera_plane(camera, "znear", 1.0)
        face_verts = project_verts(camera, self.verts)[self.faces]
        return rasterize_mesh(face_verts, self.image_size, znear if persp else None, persp, faces_per_pixel=self.faces_per_pixel)

    def render(self, camera) -> torch.Tensor:
        kw = dict(self.shade_kwargs)
        kw.setdefault("znear", _camera_plane(camera, "znear", 1.0))
        kw.setdefault("zfar", _camera_plane(camera, "zfar", 100.0))
        return shade_textured(self.fragments(camera), self.verts_uvs, self.faces_uvs, self.texture_map, **kw)


def _camera_plane(camera, name, default) -> float:
    """znear / zfar of a single camera as a Python float (a device tensor is read once: a camera is set up outside the hot path)"""
    z = getattr(camera, name, None)
    if z is None:
        return float(default)
    if torch.is_tensor(z):
        z = z.reshape(-1)
        _check(z.numel() == 1, "TexturedMeshRenderer.render takes a single camera")
        return float(z[0])
    return float(z)


def p3d_camera_from_gs(cam, device, znear: float = 1e-4, zfar: float = 100.0):
    """the pytorch3d-style camera of one Gaussian-splatting camera (`sugar_amd.synthetic.Camera`, what `io.cameras_from_json` returns),
    as sugar_scene/cameras.py:252-326 (convert_camera_from_gs_to_pytorch3d) builds it: the COLMAP frame turned to pytorch3d's (x left,
    y up), the focal lengths in NDC units of half the shorter image side, the principal point in the centre"""
    from .shims.pytorch3d.renderer.cameras import FoVPerspectiveCameras, _get_sfm_calibration_matrix
    w2c = cam.viewmatrix.detach().cpu().t().double()
    flip = torch.tensor([-1.0, -1.0, 1.0], dtype=torch.float64)
    R = (w2c[:3, :3].t() * flip).float()
    T = (w2c[:3, 3] * flip).float()
    Wd, Hd = int(cam.image_width), int(cam.image_height)
    scale = min(Wd, Hd) / 2.0
    fx, fy = Wd / (2 * cam.tanfovx), Hd / (2 * cam.tanfovy)
    K = _get_sfm_calibration_matrix(1, "cpu", torch.tensor([[fx / scale, fy / scale]]), torch.zeros(1, 2))
    return FoVPerspectiveCameras(R=R[None], T=T[None], K=K, znear=znear, zfar=zfar, device=device)


def image_metrics(image: torch.Tensor, gt: torch.Tensor) -> dict:
    """{"psnr", "ssim"} of two images [H,W,3] or [3,H,W] (float32 in [0,1], on a ROCm device) as Python floats.  PSNR is
    20 log10(1 / sqrt(mean((a - b)^2))) (inf for equal images); SSIM is the reference's 11-tap Gaussian-window mean SSIM
    (sugar_utils/loss_utils.py:39-63) from the fused HIP kernels of `sugar_amd.fused_loss`.  LPIPS is not computed: its VGG weights are
    not part of this package."""
    need_gpu("image_metrics", image=image, gt=gt)
    _check(image.shape == gt.shape and image.dim() == 3 and 3 in (image.shape[0], image.shape[2]),
           "image_metrics: two images of one shape, [H,W,3] or [3,H,W]")
    _check(image.dtype == torch.float32 and gt.dtype == torch.float32, "image_metrics: float32 images")
    if image.shape[0] != 3:   # [H,W,3]
        image, gt = image.permute(2, 0, 1), gt.permute(2, 0, 1)
    a, b = image.detach().contiguous(), gt.detach().contiguous()
    from .fused_loss import _SSIM
    with torch.no_grad():
        ssim = _SSIM.apply(a, b)
        mse = ((a - b) ** 2).mean()
        psnr = 20 * torch.log10(1.0 / torch.sqrt(mse))
    return {"psnr": float(psnr), "ssim": float(ssim)}


def load_textured_obj(path, device):
    """(verts, faces, verts_uvs, faces_uvs, texture_map) of a one-material .obj (what `save_obj` writes) on `device`, through the stand-in
    `pytorch3d.io.load_obj` (a host parser that validates every index)"""
    from .shims.pytorch3d.io import load_obj
    verts, faces, aux = load_obj(path)
    if aux.verts_uvs is None or not aux.texture_images:
        raise ValueError(f"{path}: no UV texture (the file needs vt rows, v/vt faces and a material with map_Kd)")
    tex = next(iter(aux.texture_images.values()))
    return tuple(t.to(device) for t in (verts, faces.verts_idx, aux.verts_uvs, faces.textures_idx, tex))

