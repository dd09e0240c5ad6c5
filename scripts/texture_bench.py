#!/usr/bin/env python
"""Timing of the refined mesh's texture extraction (sugar_amd.texture) at BASELINE config 4 size: make_bound_scene(1M, n = 1),
square_size 10 (S = 7 080), 1080p views.  Prints one JSON line:
  atlas_ms                      k_texture_atlas (init image + counter / winner clear), `TextureBaker.reset()`
  baker_construction_ms         the whole constructor: input copies, the UV layout (on the host), allocations, the atlas
  bake_view_us                  claim + apply of one 1080p view (sgr_texture_bake_view)
  mesh_zbuffer_ms               the hard K = 1 mesh z-buffer of one view (projection + clip test + sgr_rasterize_meshes)
  gaussian_render_ms            the Gaussian render of one view (the HIP drop-in rasterizer, SH degree 0 as the reference asks)
  extraction_100_views_s        atlas + 100 x (render + z-buffer + bake) + finalize, and the peak device memory of that run
Every kernel figure is also given as bytes moved / time / 8 TB/s (the MI355X's HBM peak).

    python scripts/texture_bench.py [--views 100] [--out file.json]
"""
import argparse
import json
import math
import os
import sys
import time

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
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from sugar_amd import shims
    shims.install()
    from sugar_amd import synthetic as syn
    from sugar_amd.diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    from sugar_amd.field import scaled_rotation
    from sugar_amd.texture import TextureBaker, project_verts, rasterize_mesh
    import make_sugar_field as mf
    dev = "cuda:0"
    W, H = 1920, 1080
    bs = syn.make_bound_scene(1_000_000, 4, n_per_triangle=1)
    sc = bs.scene
    verts, faces = bs.verts.to(dev), bs.faces.to(dev)
    means, scales, rots = sc.means3D.to(dev), sc.scales.to(dev), sc.rotations.to(dev)
    opac, shs = sc.opacities.to(dev), sc.shs.to(dev)
    M = scaled_rotation(rots, scales, inverse_scales=True)
    feats = shs[:, 0]
    T = int(faces.shape[0])
    gcams = syn.scattered_cameras(W, H, n=a.views, seed=1)
    pcams = mf.p3d_cameras_like_the_reference(gcams).to(dev)
    zn, zf = float(pcams.znear[0]), float(pcams.zfar[0])
    out = {"faces": T, "gaussians": int(means.shape[0]), "width": W, "height": H, "square_size": 10}

    def render(c):
        cam = gcams[c]
        st = GaussianRasterizationSettings(H, W, cam.tanfovx, cam.tanfovy, torch.zeros(3, device=dev), 1.0, cam.viewmatrix.to(dev),
                                           cam.projmatrix.to(dev), 0, cam.campos.to(dev), False, False)
        img, _ = GaussianRasterizer(st)(means3D=means, means2D=torch.zeros_like(means), opacities=opac, shs=shs[:, :1].contiguous(),
                                        scales=scales, rotations=rots)
        return img.permute(1, 2, 0).clamp(min=0, max=1)

    def zbuffer(c):
        return rasterize_mesh(project_verts(pcams[c], verts)[faces], (H, W), zn)

    b = TextureBaker(verts, faces, means, M, feats, 1, 10)
    S = b.S
    out["S"] = S
    t = _events(b.reset, 10)
    out["atlas_ms"] = round(t, 4)
    out["baker_construction_ms"] = round(_events(lambda: TextureBaker(verts, faces, means, M, feats, 1, 10), 3), 3)
    atlas_bytes = S * S * (12 + 4 + 8) + T * (12 + 24 + 12 + 36 + 12)
    out["atlas_bytes"] = atlas_bytes
    out["atlas_frac_of_8TBps"] = round(atlas_bytes / (t * 1e-3) / HBM, 3)
    frag = [zbuffer(c) for c in range(4)]
    rgb = [render(c) for c in range(4)]
    covered = sum(int((f.zbuf > 0).sum()) for f in frag) / 4
    k = [0]

    def bake():
        b.bake_view(frag[k[0] % 4], rgb[k[0] % 4], zn, zf)
        k[0] += 1
    t = _events(bake, 40)
    out["bake_view_us"] = round(t * 1e3, 2)
    # two passes over the fragments (8 + 12 + 4 + 4 bytes per pixel each), the UV rows of covered pixels (24 B, twice), one 8-byte
    # atomic per covered pixel, rgb + texel read-modify-write for the winners (upper bound: every covered pixel)
    bake_bytes = int(2 * W * H * 28 + covered * (2 * 24 + 8 + 8 + 12 + 12 + 12 + 8))
    out["bake_view_bytes"] = bake_bytes
    out["bake_view_frac_of_8TBps"] = round(bake_bytes / (t * 1e-3) / HBM, 3)
    out["covered_pixels_per_view"] = int(covered)
    out["mesh_zbuffer_ms"] = round(_events(lambda: zbuffer(1), 10), 3)
    out["gaussian_render_ms"] = round(_events(lambda: render(1), 10), 3)
    del frag, rgb, b
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    b = TextureBaker(verts, faces, means, M, feats, 1, 10)
    for c in range(a.views):
        b.bake_view(zbuffer(c), render(c), zn, zf)
    res = b.result()
    torch.cuda.synchronize()
    out["extraction_views"] = a.views
    out["extraction_s"] = round(time.perf_counter() - t0, 3)
    out["extraction_peak_mem_gb"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 3)
    out["visited_texels"] = int((b.counter > 0).sum())
    out["texture_finite"] = bool(torch.isfinite(res).all())
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
