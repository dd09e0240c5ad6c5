#!/usr/bin/env python
"""Timing of the textured-mesh shading kernel (sugar_amd.mesh_render.shade_textured) at BASELINE config 4 size: the mesh of
make_bound_scene(1M, n = 1) with the UV layout of square_size 10 (S = 7 080), 1920 x 1080, K = 1, 8 orbit views.  Prints one JSON line:
  shade_bilinear_us / shade_nearest_us   sgr_shade_texture_uv on one view's fragments (device events, mean over the 8 views)
  torch_shader_nearest_ms                the torch stand-in SoftPhongShader on the same fragments, same GPU, same process (nearest is the
                                         one mode it has)
  mesh_zbuffer_ms                        projection + clip test + sgr_rasterize_meshes of one view, timed separately
  render_ms                              TexturedMeshRenderer.render: all of the above per view
Each kernel figure also comes as time / (algorithmic bytes / 8 TB/s), the MI355X's HBM peak: 44 B per pixel (8 pix_to_face, 12 bary, 4
zbuf, 4 dists, 16 rgba) plus, per covered pixel, 24 B of faces_uvs, 24 B of UV rows and 12 B (nearest) or 48 B (bilinear) of texels.

    python scripts/mesh_render_bench.py [--out file.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
HBM = 8e12


def _events(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    a = ap.parse_args()
    from sugar_amd import shims
    shims.install()
    from pytorch3d.renderer import AmbientLights, Fragments, SoftPhongShader, TexturesUV
    from pytorch3d.renderer.blending import BlendParams
    from pytorch3d.structures import Meshes
    from sugar_amd import synthetic as syn
    from sugar_amd.mesh_render import TexturedMeshRenderer, shade_textured
    from sugar_amd.texture import project_verts, rasterize_mesh, texture_size, uv_layout
    import make_sugar_field as mf
    dev = "cuda:0"
    W, H, views = 1920, 1080, 8
    bs = syn.make_bound_scene(a.gaussians, 4, n_per_triangle=1)
    verts, faces = bs.verts.to(dev), bs.faces.to(dev)
    T = int(faces.shape[0])
    S = texture_size(T, 10)
    verts_uv, faces_uv = uv_layout(T, 10, dev)
    tex = torch.rand(S, S, 3, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    cams = mf.p3d_cameras_like_the_reference(syn.orbit_cameras(W, H, n=views, radius=2.6)).to(dev)
    zn, zf = float(cams.znear[0]), float(cams.zfar[0])
    blend = BlendParams(background_color=(0.0, 0.0, 0.0))
    out = {"faces": T, "S": S, "width": W, "height": H, "K": 1, "views": views}

    def zbuffer(c):
        return rasterize_mesh(project_verts(cams[c], verts)[faces], (H, W), zn)
    frags = [zbuffer(c) for c in range(views)]
    covered = sum(int((f.pix_to_face >= 0).sum()) for f in frags) / views
    out["covered_pixels_per_view"] = int(covered)
    k = [0]

    def shade(mode):
        def run():
            shade_textured(frags[k[0] % views], verts_uv, faces_uv, tex, sampling_mode=mode, blend_params=blend, znear=zn, zfar=zf)
            k[0] += 1
        return run
    for mode, texel_bytes in (("bilinear", 48), ("nearest", 12)):
        t = _events(shade(mode), 100 * views)
        nbytes = int(W * H * 44 + covered * (24 + 24 + texel_bytes))
        out[f"shade_{mode}_us"] = round(t * 1e3, 2)
        out[f"shade_{mode}_bytes"] = nbytes
        out[f"shade_{mode}_time_over_bytes_at_8TBps"] = round(t * 1e-3 / (nbytes / HBM), 2)
    # the torch stand-in on the same fragments (nearest: the mode it implements)
    mesh = Meshes(verts=[verts], faces=[faces], textures=TexturesUV(maps=tex[None], faces_uvs=[faces_uv], verts_uvs=[verts_uv],
                                                                    sampling_mode="nearest"))
    shader = SoftPhongShader(device=dev, cameras=cams[0], lights=AmbientLights(device=dev), blend_params=blend)

    def torch_shader():
        f = frags[k[0] % views]
        with torch.no_grad():
            shader(Fragments(f.pix_to_face, f.zbuf, f.bary_coords, f.dists), mesh, znear=zn, zfar=zf)
        k[0] += 1
    t_torch = _events(torch_shader, 2 * views)
    out["torch_shader_nearest_ms"] = round(t_torch, 3)
    out["torch_over_hip_nearest"] = round(t_torch * 1e3 / out["shade_nearest_us"], 1)
    with torch.no_grad():
        f = frags[0]
        ref = shader(Fragments(f.pix_to_face, f.zbuf, f.bary_coords, f.dists), mesh, znear=zn, zfar=zf)[0]
    mine = shade_textured(f, verts_uv, faces_uv, tex, sampling_mode="nearest", blend_params=blend, znear=zn, zfar=zf)
    out["max_abs_diff_to_torch_shader_nearest"] = float((mine - ref).abs().max())
    out["pixels_differing_from_torch_shader_nearest"] = int((mine != ref).any(-1).sum())
    out["mesh_zbuffer_ms"] = round(_events(lambda: zbuffer(1), 10), 3)
    r = TexturedMeshRenderer(verts, faces, verts_uv, faces_uv, tex, (H, W), blend_params=blend)
    cam_list = [cams[c] for c in range(views)]

    def render():
        r.render(cam_list[k[0] % views])
        k[0] += 1
    out["render_ms"] = round(_events(render, 2 * views), 3)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
