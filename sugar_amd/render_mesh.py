"""Draw a UV-textured .obj (what the refined-mesh extractor's `save_obj` writes) at the cameras of a `cameras.json`, and score the
renders against ground-truth images -- the textured leg of the reference's metrics.py (:260-300, 370-372) as a command:

    python -m sugar_amd.render_mesh mesh.obj --cameras cameras.json --out DIR [--gt DIR] [--sampling nearest|bilinear]

One PNG per camera (named after the camera's image) goes to --out.  With --gt, every camera whose image is found there (same name, any
of .png / .jpg / .jpeg / .JPG, same size as the render) is scored: `metrics.json` holds PSNR and SSIM per view and their means.  The
render is clamped to [0, 1] first, as metrics.py does; the background is black.  There is no LPIPS (see `mesh_render.image_metrics`)."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

_GT_SUFFIXES = ("", ".png", ".jpg", ".jpeg", ".JPG", ".PNG")


def _find_gt(gt_dir, name):
    for suffix in _GT_SUFFIXES:
        p = os.path.join(gt_dir, name + suffix)
        if os.path.isfile(p):
            return p
    return None


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m sugar_amd.render_mesh", description=__doc__.split("\n\n")[0])
    ap.add_argument("mesh", help="a .obj with vt rows, v/vt faces and one material whose map_Kd names the texture image")
    ap.add_argument("--cameras", required=True, help="cameras.json (the 3DGS format)")
    ap.add_argument("--out", required=True, help="directory for the renders (and metrics.json)")
    ap.add_argument("--gt", default=None, help="directory of ground-truth images named like the cameras")
    ap.add_argument("--sampling", choices=("nearest", "bilinear"), default="bilinear")
    ap.add_argument("--faces-per-pixel", type=int, default=1)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    from PIL import Image
    from . import io as sio
    from .mesh_render import TexturedMeshRenderer, image_metrics, load_textured_obj, p3d_camera_from_gs
    from .shims.pytorch3d.renderer.blending import BlendParams
    if not torch.cuda.is_available():
        raise RuntimeError("render_mesh needs a ROCm device; there is no CPU fallback")
    dev = torch.device(a.device)
    verts, faces, verts_uvs, faces_uvs, tex = load_textured_obj(a.mesh, dev)
    cams, names = sio.cameras_from_json(a.cameras)
    os.makedirs(a.out, exist_ok=True)
    blend = BlendParams(background_color=(0.0, 0.0, 0.0))
    renderers = {}
    views = {}
    for cam, name in zip(cams, names):
        size = (int(cam.image_height), int(cam.image_width))
        if size not in renderers:
            renderers[size] = TexturedMeshRenderer(verts, faces, verts_uvs, faces_uvs, tex, size, faces_per_pixel=a.faces_per_pixel,
                                                   sampling_mode=a.sampling, blend_params=blend)
        with torch.no_grad():
            rgb = renderers[size].render(p3d_camera_from_gs(cam, dev))[..., :3].clamp(min=0, max=1)
        Image.fromarray((rgb * 255.0).round().to(torch.uint8).cpu().numpy()).save(os.path.join(a.out, name + ".png"))
        if a.gt is not None:
            p = _find_gt(a.gt, name)
            if p is None:
                continue
            with Image.open(p) as im:
                gt = torch.from_numpy(np.asarray(im.convert("RGB"), dtype=np.uint8).astype(np.float32) / np.float32(255.0)).to(dev)
            if tuple(gt.shape[:2]) != size:
                raise ValueError(f"{p}: {gt.shape[1]}x{gt.shape[0]}, the camera renders {size[1]}x{size[0]}")
            views[name] = image_metrics(rgb, gt)
    if a.gt is not None:
        mean = {k: (sum(v[k] for v in views.values()) / len(views) if views else None) for k in ("psnr", "ssim")}
        with open(os.path.join(a.out, "metrics.json"), "w") as f:
            json.dump({"mesh": os.path.basename(a.mesh), "sampling": a.sampling, "views": views, "mean": mean}, f, indent=1)
        print(json.dumps({"views_scored": len(views), **mean}))
    print(f"{len(names)} view{'s' if len(names) != 1 else ''} written to {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
