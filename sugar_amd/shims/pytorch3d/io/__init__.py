"""`pytorch3d.io` as far as SuGaR's refined-mesh extractor needs it (sugar_extractors/refined_mesh.py:207-216): `save_obj` with a
UV texture, restated from pytorch3d 0.7.4's published `pytorch3d/io/obj_io.py` (`save_obj` / `_save`): the .obj (vertices,
`vt` UVs, `f v/vt` faces, no newline after the last face), a .mtl naming the texture and a .png of texture_map * 255 cast to
uint8, written through PIL; and, for reading that artefact back (metrics.py:268), `load_obj` / `load_objs_as_meshes`, a host parser
restated from the same file's `load_obj` / `_load_obj` / `load_objs_as_meshes` and `mtl_io.py` for files with at most one material.
PARITY-UNPINNED against pytorch3d itself."""
from __future__ import annotations

import os
from pathlib import Path

import numpy as np
import torch

import warnings
from collections import namedtuple

_Faces = namedtuple("Faces", "verts_idx normals_idx textures_idx materials_idx")
_Aux = namedtuple("Properties", "normals verts_uvs material_colors texture_images texture_atlas")


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



def _floats(rows, cols, what):
    """[n, cols] float32 from the token lists of `v` / `vt` / `vn` statements (parsed as doubles, then rounded, like a Python float)"""
    if not rows:
        return torch.zeros(0, cols, dtype=torch.float32)
    if any(len(r) < cols for r in rows):
        raise ValueError(f"{what} does not have {cols} values.")
    return torch.from_numpy(np.array([r[:cols] for r in rows], dtype=np.float64).astype(np.float32))


def _format_faces_indices(idx, max_index, what, pad_value=None):
    """pytorch3d's rule: 1-based -> 0-based, a negative index counts back from the END of the file's list; every index is checked
    here, on the host, so the renderer needs no device check"""
    t = torch.tensor(idx, dtype=torch.int64).reshape(-1, 3)
    pad = t.eq(pad_value).all(dim=-1) if pad_value is not None else None
    t[t > 0] -= 1
    t[t < 0] += max_index
    if pad is not None:
        t[pad] = pad_value
    ok = t if pad is None else t[~pad]
    if ok.numel() and (int(ok.max()) >= max_index or int(ok.min()) < 0):
        raise ValueError(f"{what} have invalid indices")
    return t


def _parse_mtl(path):
    """{material name: map_Kd file name or None} of a .mtl, in file order"""
    maps, name = {}, None
    with open(path) as fh:
        for line in fh:
            tok = line.split()
            if not tok:
                continue
            if tok[0] == "newmtl":
                name = line.strip()[len("newmtl"):].strip()
                maps[name] = None
            elif tok[0] == "map_Kd" and name is not None:
                maps[name] = line.strip()[len("map_Kd"):].strip()
    return maps


def load_obj(f, load_textures: bool = True, create_texture_atlas: bool = False, texture_atlas_size: int = 4, texture_wrap="repeat",
             device="cpu", path_manager=None):
    """(verts[V,3], Faces(verts_idx[F,3], normals_idx, textures_idx, materials_idx), Properties(normals, verts_uvs, material_colors,
    texture_images, texture_atlas)) of a Wavefront .obj on the local disk.  Reads `v`, `vt`, `vn`, `f` (as `a`, `a/b`, `a/b/c`, `a//c`;
    polygons are fan-triangulated), `mtllib` / `usemtl` and the material's `map_Kd` image (through PIL, float32 / 255); comments and every
    other statement are skipped.  An index absent from a face is -1; a file without `vt` has verts_uvs None, one without a material
    texture_images None.  A file that uses more than one material raises NotImplementedError (material_colors and texture_atlas stay
    None: nothing here reads them)."""
    if path_manager is not None:
        raise NotImplementedError("the stand-in load_obj reads local paths only")
    if create_texture_atlas:
        raise NotImplementedError("the stand-in load_obj does not build per-face texture atlases")
    path = Path(f)
    v, vt, vn = [], [], []
    fv, ft, fn = [], [], []
    mtllibs, used = [], []
    with open(path) as fh:
        for line in fh:
            tok = line.split()
            if not tok:
                continue
            key = tok[0]
            if key == "v":
                v.append(tok[1:])
            elif key == "vt":
                vt.append(tok[1:])
            elif key == "vn":
                vn.append(tok[1:])
            elif key == "f":
                corners = []
                for c in tok[1:]:
                    parts = c.split("/")
                    if len(parts) > 3:
                        raise ValueError(f"Face vertices can only have 3 properties. Face vert {c}, Line: {line.strip()}")
                    a = int(parts[0])
                    b = int(parts[1]) if len(parts) > 1 and parts[1] != "" else -1
                    n = int(parts[2]) if len(parts) > 2 and parts[2] != "" else -1
                    corners.append((a, b, n))
                if len(corners) < 3:
                    raise ValueError(f"Face has fewer than 3 vertices. Line: {line.strip()}")
                if len({(b == -1, n == -1) for _, b, n in corners}) != 1:
                    raise ValueError(f"Face is inconsistent: {line.strip()}")
                for i in range(len(corners) - 2):                     # fan triangulation
                    tri = (corners[0], corners[i + 1], corners[i + 2])
                    fv.append([c[0] for c in tri])
                    ft.append([c[1] for c in tri])
                    fn.append([c[2] for c in tri])
            elif key == "mtllib":
                mtllibs.append(line.strip()[len("mtllib"):].strip())
            elif key == "usemtl":
                name = line.strip()[len("usemtl"):].strip()
                if name not in used:
                    used.append(name)
    if len(used) > 1:
        raise NotImplementedError(f"{path}: {len(used)} materials; the stand-in load_obj reads files with one material (what save_obj writes)")
    verts = _floats(v, 3, "Vertex")
    verts_uvs = _floats(vt, 2, "Texture") if vt else None
    normals = _floats(vn, 3, "Normal") if vn else None
    n_faces = len(fv)
    verts_idx = _format_faces_indices(fv, len(v), "Faces") if n_faces else torch.zeros(0, 3, dtype=torch.int64)
    textures_idx = _format_faces_indices(ft, len(vt), "Faces textures", pad_value=-1) if n_faces \
        else torch.zeros(0, 3, dtype=torch.int64)
    normals_idx = _format_faces_indices(fn, len(vn), "Faces normals", pad_value=-1) if n_faces else torch.zeros(0, 3, dtype=torch.int64)
    materials_idx = torch.full((n_faces,), 0 if used else -1, dtype=torch.int64)
    texture_images = None
    if load_textures and mtllibs and used:
        mtl_path = path.parent / mtllibs[0]
        if not mtl_path.is_file():
            warnings.warn(f"Mtl file does not exist: {mtl_path}")
        else:
            maps = _parse_mtl(mtl_path)
            if used[0] not in maps:
                raise ValueError(f"{path}: material {used[0]!r} is not defined in {mtl_path.name}")
            texture_images = {}
            if maps[used[0]] is not None:
                from PIL import Image
                with Image.open(os.fspath(mtl_path.parent / maps[used[0]])) as im:
                    arr = np.asarray(im.convert("RGB"), dtype=np.uint8)
                texture_images[used[0]] = torch.from_numpy(arr.astype(np.float32) / np.float32(255.0))
    to = lambda t: None if t is None else t.to(device)
    faces = _Faces(to(verts_idx), to(normals_idx), to(textures_idx), to(materials_idx))
    aux = _Aux(to(normals), to(verts_uvs), None, None if texture_images is None else {k: to(t) for k, t in texture_images.items()}, None)
    return to(verts), faces, aux


def load_objs_as_meshes(files, device=None, load_textures: bool = True, create_texture_atlas: bool = False,
                        texture_atlas_size: int = 4, texture_wrap="repeat", path_manager=None):
    """a `Meshes` of the .obj files, each with its `TexturesUV` at the container's defaults (bilinear, align_corners=True, border) where
    the file has a textured material, `textures=None` where none has.  Every face of a textured file must carry a `vt` index."""
    from ..renderer import TexturesUV
    from ..structures import Meshes
    device = "cpu" if device is None else device
    verts_l, faces_l, uvs_l, fuv_l, maps_l = [], [], [], [], []
    for f in files:
        verts, faces, aux = load_obj(f, load_textures=load_textures, create_texture_atlas=create_texture_atlas,
                                     texture_atlas_size=texture_atlas_size, texture_wrap=texture_wrap, path_manager=path_manager)
        verts_l.append(verts.to(device))
        faces_l.append(faces.verts_idx.to(device))
        if aux.texture_images:
            if aux.verts_uvs is None or bool((faces.textures_idx < 0).any()):
                raise ValueError(f"{f}: a textured material, but not every face has a vt index")
            uvs_l.append(aux.verts_uvs.to(device))
            fuv_l.append(faces.textures_idx.to(device))
            maps_l.append(next(iter(aux.texture_images.values())).to(device))
    tex = None
    if maps_l:
        if len(maps_l) != len(verts_l):
            raise NotImplementedError("load_objs_as_meshes: textured and untextured files in one batch")
        if len({tuple(m.shape) for m in maps_l}) != 1:
            raise NotImplementedError("load_objs_as_meshes: texture maps of different sizes in one batch")
        tex = TexturesUV(maps=maps_l, faces_uvs=fuv_l, verts_uvs=uvs_l)
    return Meshes(verts=verts_l, faces=faces_l, textures=tex)
