#!/usr/bin/env python
"""Times of the level-set route -- sampling from every camera, then the local implicit surface of sugar_amd.point_surface -- on the GPU
(profiles/point_surface.json).

The scene is make_bound_scene(1M, opaque=True), seed 7, seen by 100 orbit cameras at 1920 x 1080; 10M pixels are sampled over all
cameras at the level 0.3 and the foreground cloud is meshed on linspace(-1, 1, 512) x extent with a radius of 3 spacings and K = 16 --
the foreground pass of `extract.extract_mesh_level_sets` with its defaults.  Every stage is timed between two HIP events (summed over
the chunks of the sweep where a stage runs once per chunk), after one warm run at a small size; the figure is the median of 5 runs.

  sampling        the loop over the cameras of `extract.sample_level_set_cloud` (depth render, pixel pick, k-NN, level crossings)
  outliers        `point_surface.statistical_outlier_mask` on the foreground cloud (k-NN of the cloud on itself)
  brick_marking   sgr_point_surface_mark + sgr_sparse_sweep_compact (+ the NaN fill of the volume and the count's read)
  knn             the k-NN of the brick points, all chunks
  evaluation      sgr_sparse_sweep_points + sgr_point_surface_eval + sgr_sparse_sweep_scatter, all chunks (pack included)
  marching_cubes  `marching_cubes(volume, 0.0)`
  face_drop       the spurious-vertex kernel + `decimate.remove_vertices_by_mask`
  finish          grid_to_world, the weights at the vertices (k-NN + evaluation), vertex normals
and `mesh_total` is `mesh_from_oriented_points` as a whole, `route_total` one call of `extract_mesh_level_sets` (foreground only).
The file also holds the active-brick fraction, the peak memory, and the vertex and face counts next to those of the marching-cubes
route on the same scene (profiles/sparse_sweep.json, leg sparse_512_fg) when that file is present.

    python scripts/point_surface_bench.py [--out profiles/point_surface.json] [--gaussians N --cameras C --width W --height H
                                           --n-points N --resolution R --repeats 5]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sugar_amd import decimate, extract, marching_cubes as mc, point_surface as ps, synthetic as syn  # noqa: E402
from sugar_amd._call import call, ptr as p  # noqa: E402
from sugar_amd.knn import knn_points  # noqa: E402

DEV = "cuda:0"
LEVEL = 0.3
K = 16
RADIUS_CELLS = 3.0


class Stages:
    """HIP-event pairs per stage; `ms()` sums a stage's pairs after one synchronisation"""

    def __init__(self):
        self.pairs = {}

    def __call__(self, name):
        return _Span(self.pairs.setdefault(name, []))

    def ms(self):
        torch.cuda.synchronize()
        return {k: sum(a.elapsed_time(b) for a, b in v) for k, v in self.pairs.items()}


class _Span:
    def __init__(self, pairs):
        self.pairs = pairs

    def __enter__(self):
        self.t0 = torch.cuda.Event(enable_timing=True)
        self.t0.record()

    def __exit__(self, *exc):
        t1 = torch.cuda.Event(enable_timing=True)
        t1.record()
        self.pairs.append((self.t0, t1))


def staged_mesh(pts, nrm, X, radius, st, points_per_pass=2_000_000):
    """the steps of point_surface.mesh_from_oriented_points, one by one under the stage timers; returns (verts, faces, info)"""
    n = X.numel()
    N = int(pts.shape[0])
    nb = (n + ps.BRICK - 1) // ps.BRICK
    with st("brick_marking"):
        flags = torch.empty((nb ** 3 + 15) // 16 * 16, dtype=torch.uint8, device=DEV)
        meta = torch.empty(4, dtype=torch.int32, device=DEV)
        bricks = torch.empty(nb ** 3, dtype=torch.int32, device=DEV)
        call("sgr_point_surface_mark", DEV, N, p(pts), radius, n, n, n, p(X), p(X), p(X), p(flags), p(meta))
        call("sgr_sparse_sweep_compact", DEV, n, n, n, p(X), p(X), p(X), 0, 0.0, 0.0, p(flags), p(bricks), p(meta))
        volume = torch.full((n, n, n), float("nan"), dtype=torch.float32, device=DEV)
        n_active = meta.tolist()[0]
    with st("evaluation"):
        packed = ps._pack(pts, nrm)
    chunk = max(1, points_per_pass // ps.BRICK ** 3)
    q_buf = torch.empty(min(chunk, max(n_active, 1)) * ps.BRICK ** 3, 3, dtype=torch.float32, device=DEV)
    v_buf = torch.empty(q_buf.shape[0], dtype=torch.float32, device=DEV)
    for b0 in range(0, n_active, chunk):
        b1 = min(b0 + chunk, n_active)
        m = (b1 - b0) * ps.BRICK ** 3
        q, val = q_buf[:m], v_buf[:m]
        with st("evaluation"):
            call("sgr_sparse_sweep_points", DEV, n, n, n, p(X), p(X), p(X), p(bricks), b0, b1, p(q))
        with st("knn"):
            idx = knn_points(q[None], pts[None], K=K).idx[0]
        with st("evaluation"):
            call("sgr_point_surface_eval", DEV, m, K, p(q), p(idx), N, p(packed), radius, p(val), None)
            call("sgr_sparse_sweep_scatter", DEV, n, n, n, p(bricks), b0, b1, p(val), p(volume))
    with st("marching_cubes"):
        verts_index, faces = mc.marching_cubes(volume, 0.0)
    mc_counts = (int(verts_index.shape[0]), int(faces.shape[0]))
    with st("face_drop"):
        if faces.shape[0]:
            verts_index, faces = decimate.remove_vertices_by_mask(verts_index, faces, ps.spurious_vertices(verts_index, volume), unreferenced=True)
    with st("finish"):
        verts = extract.grid_to_world(verts_index, X, X, X)
        weights = torch.empty(verts.shape[0], dtype=torch.float32, device=DEV)
        ps._eval(verts.contiguous(), pts, packed, radius, K, torch.empty_like(weights), weights)
        normals = mc.vertex_normals(verts, faces) if verts.shape[0] else verts
    return verts, faces, dict(active_bricks=n_active, total_bricks=nb ** 3, mc_vertices=mc_counts[0], mc_faces=mc_counts[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "point_surface.json"))
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--cameras", type=int, default=100)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--n-points", type=int, default=10_000_000)
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("point_surface_bench: no GPU; times are measured on the device or not at all")
    sc = syn.make_bound_scene(a.gaussians, 7, opaque=True).scene
    model = [t.to(DEV).contiguous() for t in (sc.means3D, sc.scales, sc.rotations, sc.opacities)]
    dc = sc.shs[:, 0, :].contiguous().to(DEV)
    extent = float(model[0].abs().max()) * 1.05
    cams = syn.orbit_cameras(a.width, a.height, n=a.cameras)
    small = syn.orbit_cameras(640, 360, n=4)
    res = dict(device=torch.cuda.get_device_name(0), gaussians=int(model[0].shape[0]), scene="make_bound_scene(opaque=True), seed 7",
               cameras=a.cameras, image=[a.width, a.height], n_total_points=a.n_points, resolution=a.resolution, level=LEVEL, K=K,
               radius_cells=RADIUS_CELLS, extent=extent, repeats=a.repeats, timing="HIP events; median of the repeats, ms")

    def run(cameras, n_points, resolution):
        st = Stages()
        with st("sampling"):
            cloud, cloud_n = extract.sample_level_set_cloud(*model, cameras, LEVEL, n_points, K, 0)
        fg = cloud.abs().max(dim=1).values < extent
        pts, nrm = cloud[fg].contiguous(), cloud_n[fg].contiguous()
        with st("outliers"):
            keep = ps.statistical_outlier_mask(pts, 20, 20.0)
        pts, nrm = pts[keep].contiguous(), nrm[keep].contiguous()
        X = torch.linspace(-1, 1, resolution, device=DEV) * extent
        radius = float(torch.tensor(RADIUS_CELLS * 2.0 * extent / (resolution - 1), dtype=torch.float32))
        if pts.shape[0] < K:
            raise SystemExit(f"point_surface_bench: the sampler found {int(pts.shape[0])} points, fewer than K = {K}; nothing to mesh")
        verts, faces, info = staged_mesh(pts, nrm, X, radius, st)
        with st("mesh_total"):
            mesh = ps.mesh_from_oriented_points(pts, nrm, X, X, X, radius=radius, K=K)
        info.update(sampled_points=int(cloud.shape[0]), foreground_points=int(fg.sum()), cloud_points=int(pts.shape[0]),
                    vertices=int(verts.shape[0]), faces=int(faces.shape[0]),
                    staged_equals_mesh_from_oriented_points=bool(torch.equal(mesh["verts"], verts) and torch.equal(mesh["faces"], faces)))
        return st.ms(), info

    run(small, 400_000, 64)                                                   # warm: code objects, the allocator
    torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats()
    runs = []
    for _ in range(a.repeats):
        ms, info = run(cams, a.n_points, a.resolution)
        runs.append(ms)
        print(json.dumps(ms), flush=True)
    res["stages_ms"] = {k: statistics.median(r[k] for r in runs) for k in runs[0]}
    res["stages_ms_all_runs"] = runs
    res.update(info)
    res["active_brick_fraction"] = info["active_bricks"] / info["total_bricks"]
    res["peak_memory_mib"] = torch.cuda.max_memory_allocated() / 2 ** 20
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    mesh = extract.extract_mesh_level_sets(*model, dc, cams, extent, surface_level=LEVEL, n_total_points=a.n_points, resolution=a.resolution,
                                           radius_cells=RADIUS_CELLS, K=K, background=False)
    t1.record(); torch.cuda.synchronize()
    res["route_total_ms"] = t0.elapsed_time(t1)
    res["route_vertices"], res["route_faces"] = int(mesh["verts"].shape[0]), int(mesh["faces"].shape[0])
    other = os.path.join(ROOT, "profiles", "sparse_sweep.json")
    if os.path.exists(other) and a.resolution == 512:
        leg = json.load(open(other)).get("sparse_512_fg")
        if isinstance(leg, dict):
            res["marching_cubes_route_sparse_512_fg"] = {k: leg[k] for k in ("ms", "vertices", "faces", "active_bricks", "total_bricks") if k in leg}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "stages_ms_all_runs"}, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
