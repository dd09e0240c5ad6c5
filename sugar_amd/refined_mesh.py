"""From a refine-stage checkpoint to the textured .obj -- SuGaR's last stage (sugar_extractors/refined_mesh.py) as a command:

    python -m sugar_amd.refined_mesh CHECKPOINT.pt --cameras cameras.json --out mesh.obj
           [--square-size 10] [--postprocess] [--postprocess-iterations 5] [--postprocess-density-threshold 0.1] [--device cuda:0]

CHECKPOINT.pt is what sugar_trainers/refine.py saves: a dict whose `state_dict` holds `_points` (the mesh vertices),
`_surface_mesh_faces`, `surface_mesh_thickness`, `_scales` [F*n,2], `_quaternions` [F*n,2] (complex numbers), `all_densities` [F*n,1],
`_sh_coordinates_dc` and `_sh_coordinates_rest`; n = rows // F must be 1, 3, 4 or 6.  The command derives the bound Gaussians
(`sugar_amd.mesh_bind`), with --postprocess removes the border faces and revives the dense ones (`sugar_amd.mesh_postprocess`, the
reference's defaults) and rebinds to the kept faces, then for every camera of cameras.json, in file order as `io.cameras_from_json`
returns them, renders the Gaussians with their DC colour on black, z-buffers the mesh and bakes the view into the UV texture
(`sugar_amd.texture.TextureBaker`); it writes verts, faces, UVs and the texture clamped to [0, 1] with the stand-in
`pytorch3d.io.save_obj` (mesh.obj, mesh.mtl, mesh.png) and prints one JSON line.  Vertices are kept as they are.  Every camera must
have the same image size.  No reference file and no open3d are needed; there is no CPU fallback."""
from __future__ import annotations

import argparse
import json
import sys
import time

import torch

CHECKPOINT_KEYS = ("_points", "_surface_mesh_faces", "surface_mesh_thickness", "_scales", "_quaternions", "all_densities",
                   "_sh_coordinates_dc", "_sh_coordinates_rest")
GAUSSIANS_PER_TRIANGLE = (1, 3, 4, 6)


def parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m sugar_amd.refined_mesh", description=__doc__.split("\n\n")[0])
    ap.add_argument("checkpoint", help="a refine-stage checkpoint (.pt) with a state_dict")
    ap.add_argument("--cameras", required=True, help="cameras.json (the 3DGS format)")
    ap.add_argument("--out", required=True, help="the .obj to write (its .mtl and .png go next to it)")
    ap.add_argument("--square-size", type=int, default=10, help="texels per side of a square of two triangles (>= 3)")
    ap.add_argument("--postprocess", action="store_true", help="remove border faces whose Gaussians have a low density")
    ap.add_argument("--postprocess-iterations", type=int, default=5)
    ap.add_argument("--postprocess-density-threshold", type=float, default=0.1)
    ap.add_argument("--device", default="cuda:0")
    return ap


def model_from_state_dict(sd, device="cpu") -> dict:
    """dict(verts[V,3], faces[F,3] int64, n, thickness[1], scales[F*n,2], complex_numbers[F*n,2], all_densities[F*n,1],
    sh_dc[F*n,1,3], sh_rest[F*n,R,3]) of a refine checkpoint's state_dict, on `device`.  A missing key, or a row count that is not F*n
    with n in {1, 3, 4, 6}, is a ValueError."""
    for k in CHECKPOINT_KEYS:
        if k not in sd:
            raise ValueError(f"the checkpoint's state_dict has no `{k}` (a refine-stage checkpoint holds {', '.join(CHECKPOINT_KEYS)})")
    t = lambda k, dtype: torch.as_tensor(sd[k]).detach().to(device=device, dtype=dtype).contiguous()
    verts, faces = t("_points", torch.float32), t("_surface_mesh_faces", torch.int64)
    if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3 or faces.shape[0] == 0:
        raise ValueError("the checkpoint's `_points` must be [V,3] and `_surface_mesh_faces` [F,3] with F > 0")
    F_ = int(faces.shape[0])
    m = dict(verts=verts, faces=faces, thickness=t("surface_mesh_thickness", torch.float32).reshape(-1),
             scales=t("_scales", torch.float32), complex_numbers=t("_quaternions", torch.float32),
             all_densities=t("all_densities", torch.float32), sh_dc=t("_sh_coordinates_dc", torch.float32),
             sh_rest=t("_sh_coordinates_rest", torch.float32))
    rows = int(m["scales"].shape[0])
    n = rows // F_
    if n * F_ != rows or n not in GAUSSIANS_PER_TRIANGLE:
        raise ValueError(f"`_scales` has {rows} rows for {F_} faces: not F*n with n in {GAUSSIANS_PER_TRIANGLE}")
    for k in ("complex_numbers", "all_densities", "sh_dc", "sh_rest"):
        if int(m[k].shape[0]) != rows:
            raise ValueError(f"the checkpoint's per-Gaussian tensors disagree: `_scales` has {rows} rows, {k} has {int(m[k].shape[0])}")
    if tuple(m["scales"].shape) != (rows, 2) or tuple(m["complex_numbers"].shape) != (rows, 2) or m["thickness"].numel() != 1:
        raise ValueError("`_scales` and `_quaternions` must be [F*n,2] and `surface_mesh_thickness` one element")
    if tuple(m["sh_dc"].shape) != (rows, 1, 3) or m["sh_rest"].dim() != 3 or m["sh_rest"].shape[2] != 3:
        raise ValueError("`_sh_coordinates_dc` must be [F*n,1,3] and `_sh_coordinates_rest` [F*n,R,3]")
    m["all_densities"] = m["all_densities"].reshape(rows, 1)
    m["n"] = n
    return m


def load_checkpoint(path, device="cpu") -> dict:
    ck = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(ck, dict) or "state_dict" not in ck:
        raise ValueError(f"{path}: not a refine-stage checkpoint (a dict with a `state_dict`)")
    return model_from_state_dict(ck["state_dict"], device)


def _render_dc(cam, points, shs, opacities, scaling, quaternions, dev):
    """the Gaussians at one camera with their DC colour on black (`render_image_gaussian_rasterizer(sh_deg=0,
    compute_color_in_rasterizer=True)`, sugar_model.py:2085-2281): [H,W,3], clamped to [0, 1]"""
    from .diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    settings = GaussianRasterizationSettings(
        image_height=int(cam.image_height), image_width=int(cam.image_width), tanfovx=cam.tanfovx, tanfovy=cam.tanfovy,
        bg=torch.zeros(3, device=dev), scale_modifier=1.0, viewmatrix=cam.viewmatrix.to(dev), projmatrix=cam.projmatrix.to(dev),
        sh_degree=0, campos=cam.campos.to(dev), prefiltered=False, debug=False)
    image, _ = GaussianRasterizer(settings)(means3D=points, means2D=torch.zeros_like(points), shs=shs, opacities=opacities,
                                           scales=scaling, rotations=quaternions)
    return image.permute(1, 2, 0).clamp(min=0, max=1)


def main(argv=None) -> int:
    a = parser().parse_args(argv)
    if a.square_size < 3:
        raise ValueError("--square-size must be >= 3")
    if a.postprocess_iterations < 0:
        raise ValueError("--postprocess-iterations must not be negative")
    from . import io as sio
    from . import mesh_bind
    from .field import scaled_rotation
    from .mesh_postprocess import bary_coords, postprocess_bound_mesh
    from .mesh_render import _camera_plane, p3d_camera_from_gs
    from .shims.pytorch3d.io import save_obj
    from .texture import TextureBaker, project_verts, rasterize_mesh
    if not torch.cuda.is_available():
        raise RuntimeError("refined_mesh needs a ROCm device; there is no CPU fallback")
    dev = torch.device(a.device)
    seconds = {}
    t0 = time.perf_counter()

    def phase(name):
        nonlocal t0
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        seconds[name] = round(t1 - t0, 4)
        t0 = t1

    m = load_checkpoint(a.checkpoint, dev)
    cams, _ = sio.cameras_from_json(a.cameras, device=dev)
    if not cams:
        raise ValueError(f"{a.cameras}: no camera")
    H, W = int(cams[0].image_height), int(cams[0].image_width)
    if any((int(c.image_height), int(c.image_width)) != (H, W) for c in cams):
        raise ValueError(f"{a.cameras}: the cameras must share one image size")
    verts, faces, n = m["verts"], m["faces"], m["n"]
    scales, cplx, dens, sh_dc, sh_rest = m["scales"], m["complex_numbers"], m["all_densities"], m["sh_dc"], m["sh_rest"]
    faces_before = int(faces.shape[0])
    phase("load")
    with torch.no_grad():
        if a.postprocess:
            post = postprocess_bound_mesh(verts, faces, n, scales, cplx, dens, m["thickness"], sh_dc, sh_rest,
                                          iterations=a.postprocess_iterations, density_threshold=a.postprocess_density_threshold)
            faces = post.faces.contiguous()
            scales, cplx, dens, sh_dc, sh_rest = (t.contiguous() for t in post.per_gaussian)
            if faces.shape[0] == 0:
                raise ValueError("the postprocess removed every face: nothing to texture")
            phase("postprocess")
        points = mesh_bind.bound_points(verts, faces, bary_coords(n).to(dev))
        scaling = mesh_bind.bound_scaling(scales, m["thickness"])
        quats = mesh_bind.bound_quaternions(verts, faces, cplx, n)
        opacities = torch.sigmoid(dens)
        shs = torch.cat([sh_dc, sh_rest], dim=1).contiguous()
        baker = TextureBaker(verts, faces, points, scaled_rotation(quats, scaling, inverse_scales=True), sh_dc[:, 0], n, a.square_size)
        phase("bind")
        for cam in cams:
            rgb = _render_dc(cam, points, shs, opacities, scaling, quats, dev)
            p3d = p3d_camera_from_gs(cam, dev)
            znear, zfar = _camera_plane(p3d, "znear", 1.0), _camera_plane(p3d, "zfar", 100.0)
            frags = rasterize_mesh(project_verts(p3d, verts)[faces].float(), (H, W), znear, True)
            baker.bake_view(frags, rgb.float(), znear, zfar)
        texture = baker.result().clamp(0.0, 1.0)
        phase("bake")
        save_obj(a.out, verts=verts, faces=faces, verts_uvs=baker.verts_uv, faces_uvs=baker.faces_uv, texture_map=texture)
        phase("save")
    print(json.dumps({"faces_before": faces_before, "faces_after": int(faces.shape[0]), "gaussians_per_triangle": n,
                      "views_baked": len(cams), "texture_side": int(baker.S), "seconds": seconds}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
