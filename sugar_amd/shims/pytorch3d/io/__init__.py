"""`pytorch3d.io` as far as SuGaR's refined-mesh extractor needs it (sugar_extractors/refined_mesh.py:207-216): `save_obj` with a
UV texture, restated from pytorch3d 0.7.4's published `pytorch3d/io/obj_io.py` (`save_obj` / `_save`): the .obj (vertices,
`vt` UVs, `f v/vt` faces, no newline after the last face), a .mtl naming the texture and a .png of texture_map * 255 cast to
uint8, written through PIL.  PARITY-UNPINNED against pytorch3d itself.  `load_objs_as_meshes` stays a placeholder."""
from __future__ import annotations

import os
from pathlib import Path

import numpy as np
import torch

from .._placeholder import out_of_scope_fn

load_objs_as_meshes = out_of_scope_fn("io.load_objs_as_meshes")
load_obj = out_of_scope_fn("io.load_obj")


def save_obj(f, verts, faces, decimal_places=None, path_manager=None, *, normals=None, faces_normals=None, verts_uvs=None,
             faces_uvs=None, texture_map=None) -> None:
    if path_manager is not None:
        raise NotImplementedError("the stand-in save_obj writes to local paths only")
    if len(verts) and (verts.dim() != 2 or verts.size(1) != 3):
        raise ValueError("Argument 'verts' should either be empty or of shape (num_verts, 3).")
    if len(faces) and (faces.dim() != 2 or faces.size(1) != 3):
        raise ValueError("Argument 'faces' should either be empty or of shape (num_faces, 3).")
    if normals is not None or faces_normals is not None:
        raise NotImplementedError("the stand-in save_obj does not write normals")
    if texture_map is not None and (texture_map.dim() != 3 or texture_map.size(2) != 3):
        raise ValueError("Argument 'texture_map' should be of shape (H, W, 3).")
    if faces_uvs is not None and (faces_uvs.dim() != 2 or faces_uvs.size(1) != 3):
        raise ValueError("Argument 'faces_uvs' should be of shape (num_faces, 3).")
    if verts_uvs is not None and (verts_uvs.dim() != 2 or verts_uvs.size(1) != 2):
        raise ValueError("Argument 'verts_uvs' should be of shape (num_verts, 2).")
    save_texture = all(t is not None for t in (faces_uvs, verts_uvs, texture_map))
    output_path = Path(f)
    float_str = "%f" if decimal_places is None else "%" + ".%df" % decimal_places
    with open(output_path, "w") as fh:
        if save_texture:
            fh.write(f"mtllib {output_path.stem}.mtl\n")
            fh.write("usemtl mesh\n\n")
        fh.write(_obj_lines(verts, faces, float_str, verts_uvs if save_texture else None, faces_uvs if save_texture else None))
    if save_texture:
        image_path = output_path.with_suffix(".png")
        mtl_path = output_path.with_suffix(".mtl")
        from PIL import Image
        tm = texture_map.detach().cpu() * 255.0
        Image.fromarray(tm.numpy().astype(np.uint8)).save(os.fspath(image_path))
        with open(mtl_path, "w") as f_mtl:
            f_mtl.write(f"newmtl mesh\nmap_Kd {output_path.stem}.png\n"
                        "Ka 1.000 1.000 1.000\nKd 1.000 1.000 1.000\nKs 0.000 0.000 0.000\nNs 0.0\nillum 0\n")


def _obj_lines(verts, faces, float_str, verts_uvs, faces_uvs) -> str:
    parts = []
    v = verts.detach().cpu().double().tolist()
    parts += ["v %s\n" % " ".join(float_str % x for x in row) for row in v]
    if verts_uvs is not None:
        parts += ["vt %s\n" % " ".join(float_str % x for x in row) for row in verts_uvs.detach().cpu().double().tolist()]
    fc = faces.detach().cpu().long().tolist()
    if verts_uvs is not None:
        fu = faces_uvs.detach().cpu().long().tolist()
        rows = ["f %s" % " ".join("%d/%d" % (a + 1, b + 1) for a, b in zip(fr, ur)) for fr, ur in zip(fc, fu)]
    else:
        rows = ["f %s" % " ".join("%d" % (a + 1) for a in fr) for fr in fc]
    return "".join(parts) + "\n".join(rows)   # no newline after the last face
