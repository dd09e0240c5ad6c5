"""`pytorch3d.renderer.MeshRenderer` / `SoftPhongShader` for what the texture baking of the refined mesh uses
(sugar_scene/sugar_model.py:2607-2661): ambient-only lights (`AmbientLights`, default materials: colour = 1 x texel + 0) over a
`TexturesUV` sampled with `sampling_mode='nearest'`, blended by `softmax_rgb_blend`.  Restated from pytorch3d 0.7.4's published
`shader.py`, `shading.py`, `textures.py` (TexturesUV.sample_textures) and `ops/interp_face_attrs.py` (the CPU path,
interpolate_face_attributes_python); PARITY-UNPINNED against pytorch3d itself.  Other lights or sampling modes raise
NotImplementedError.  Plain torch: this is the CPU path the fixtures are written with; the product bakes textures with the HIP
kernels of sugar_amd.texture instead.  The one call the torch path does not serve -- `sampling_mode='bilinear'` (the default of the
`TexturesUV` that `load_objs_as_meshes` builds) on a ROCm device with no gradient wanted, what metrics.py:289-300, 372 runs -- goes to
the HIP shading kernel of sugar_amd.mesh_render, view by view.  Everything the torch path served before keeps it."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from ..blending import BlendParams, softmax_rgb_blend
from ..lighting import AmbientLights


def interpolate_face_attributes(pix_to_face, barycentric_coords, face_attributes):
    """pix_to_face (N,H,W,K), bary (N,H,W,K,3), face_attributes (F,3,D) -> (N,H,W,K,D); 0 where no face"""
    F_, FV, D = face_attributes.shape
    N, H, W, K, _ = barycentric_coords.shape
    mask = pix_to_face < 0
    pix_to_face = pix_to_face.clone()
    pix_to_face[mask] = 0
    idx = pix_to_face.view(N * H * W * K, 1, 1).expand(N * H * W * K, 3, D)
    pixel_face_vals = face_attributes.gather(0, idx).view(N, H, W, K, 3, D)
    pixel_vals = (barycentric_coords[..., None] * pixel_face_vals).sum(dim=-2)
    pixel_vals[mask] = 0
    return pixel_vals


def sample_textures_uv(textures, fragments) -> torch.Tensor:
    """TexturesUV.sample_textures (N,H,W,K,C) for one map per mesh: UV interpolation, then grid_sample of the y-flipped map"""
    if textures.sampling_mode != "nearest":
        raise NotImplementedError("the stand-in shader samples TexturesUV with sampling_mode='nearest' only")
    texture_maps = textures.maps_padded()
    faces_verts_uvs = torch.cat([v[f] for v, f in zip(textures.verts_uvs_list(), textures.faces_uvs_list())])
    pixel_uvs = interpolate_face_attributes(fragments.pix_to_face, fragments.bary_coords, faces_verts_uvs)
    N, H_out, W_out, K = fragments.pix_to_face.shape
    N, H_in, W_in, C = texture_maps.shape
    pixel_uvs = pixel_uvs.permute(0, 3, 1, 2, 4).reshape(N * K, H_out, W_out, 2)
    texture_maps = texture_maps.permute(0, 3, 1, 2)[None, ...].expand(K, -1, -1, -1, -1).transpose(0, 1).reshape(N * K, C, H_in, W_in)
    pixel_uvs = pixel_uvs * 2.0 - 1.0
    texture_maps = torch.flip(texture_maps, [2])
    if texture_maps.device != pixel_uvs.device:
        texture_maps = texture_maps.to(pixel_uvs.device)
    texels = F.grid_sample(texture_maps, pixel_uvs, mode=textures.sampling_mode, align_corners=textures.align_corners,
                           padding_mode=textures.padding_mode)
    return texels.reshape(N, K, C, H_out, W_out).permute(0, 3, 4, 1, 2)


def _takes_hip_path(fragments, textures, lights) -> bool:
    """bilinear sampling on a ROCm device with nothing to differentiate: exactly the call `sample_textures_uv` raises for"""
    if getattr(textures, "sampling_mode", None) != "bilinear" or not fragments.pix_to_face.is_cuda:
        return False
    if not torch.is_grad_enabled():
        return True
    tensors = [fragments.zbuf, fragments.bary_coords, fragments.dists, textures.maps_padded(), lights.ambient_color]
    tensors += list(textures.verts_uvs_list())
    return not any(torch.is_tensor(t) and t.requires_grad for t in tensors)


def _per_view(z, N):
    """znear / zfar as N Python floats (a camera's device tensor is read here, once per call)"""
    if torch.is_tensor(z):
        z = z.detach().reshape(-1).tolist()
    else:
        z = [float(z)]
    if len(z) not in (1, N):
        raise ValueError(f"expected 1 or {N} znear / zfar values, got {len(z)}")
    return z * N if len(z) == 1 else z


def _shade_hip(fragments, meshes, lights, blend_params, znear, zfar) -> torch.Tensor:
    """(N,H,W,4): view n shades mesh n (or the only mesh) with sugar_amd.mesh_render.shade_textured"""
    from sugar_amd.mesh_render import shade_textured
    textures = meshes.textures
    N = int(fragments.pix_to_face.shape[0])
    maps, uvs, fuvs = textures.maps_padded(), textures.verts_uvs_list(), textures.faces_uvs_list()
    if len(uvs) != N or maps.shape[0] != N:
        raise ValueError(f"{N} views of fragments, but textures for {len(uvs)} meshes")
    ambient = lights.ambient_color.detach().cpu().reshape(-1, 3)
    bg = blend_params.background_color
    bg = bg.detach().cpu() if torch.is_tensor(bg) else bg
    bp = BlendParams(blend_params.sigma, blend_params.gamma, bg)
    zn, zf = _per_view(znear, N), _per_view(zfar, N)
    out, base = [], 0
    for n in range(N):
        frag = (fragments.pix_to_face[n], fragments.zbuf[n], fragments.bary_coords[n], fragments.dists[n])
        out.append(shade_textured(frag, uvs[n].float(), fuvs[n].long(), maps[n].float(), sampling_mode="bilinear",
                                  align_corners=textures.align_corners, padding_mode=textures.padding_mode, blend_params=bp,
                                  znear=zn[n], zfar=zf[n], ambient=ambient[n if ambient.shape[0] > 1 else 0], face_index_base=base))
        base += int(fuvs[n].shape[0])
    return torch.stack(out)


class SoftPhongShader(torch.nn.Module):
    def __init__(self, device="cpu", cameras=None, lights=None, materials=None, blend_params=None):
        super().__init__()
        self.lights = lights if lights is not None else AmbientLights(device=device)
        self.materials = materials
        self.cameras = cameras
        self.blend_params = blend_params if blend_params is not None else BlendParams()

    def to(self, device):
        if self.cameras is not None:
            self.cameras = self.cameras.to(device)
        self.lights = self.lights.to(device)
        return self

    def forward(self, fragments, meshes, **kwargs) -> torch.Tensor:
        cameras = kwargs.get("cameras", self.cameras)
        if cameras is None:
            raise ValueError("Cameras must be specified either at initialization or in the forward pass of SoftPhongShader")
        lights = kwargs.get("lights", self.lights)
        if not isinstance(lights, AmbientLights):
            raise NotImplementedError("the stand-in SoftPhongShader supports AmbientLights only")
        if kwargs.get("materials", self.materials) is not None:
            raise NotImplementedError("the stand-in SoftPhongShader uses pytorch3d's default Materials only")
        blend_params = kwargs.get("blend_params", self.blend_params)
        if _takes_hip_path(fragments, meshes.textures, lights):
            return _shade_hip(fragments, meshes, lights, blend_params, kwargs.get("znear", getattr(cameras, "znear", 1.0)),
                              kwargs.get("zfar", getattr(cameras, "zfar", 100.0)))
        texels = sample_textures_uv(meshes.textures, fragments)
        # phong_shading with AmbientLights and the default Materials (all colours 1): ambient = 1 * ambient_color, diffuse = specular = 0
        ambient = lights.ambient_color.to(texels.device)[:, None, None, None, :]
        zero = torch.zeros((), dtype=texels.dtype, device=texels.device)
        colors = (ambient + zero) * texels + zero
        znear = kwargs.get("znear", getattr(cameras, "znear", 1.0))
        zfar = kwargs.get("zfar", getattr(cameras, "zfar", 100.0))
        return softmax_rgb_blend(colors, fragments, blend_params, znear=znear, zfar=zfar)


class MeshRenderer(torch.nn.Module):
    def __init__(self, rasterizer, shader):
        super().__init__()
        self.rasterizer = rasterizer
        self.shader = shader

    def to(self, device):
        self.rasterizer.to(device)
        self.shader.to(device)
        return self

    def forward(self, meshes_world, **kwargs) -> torch.Tensor:
        fragments = self.rasterizer(meshes_world, **kwargs)
        return self.shader(fragments, meshes_world, **kwargs)
