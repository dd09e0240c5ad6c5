#!/usr/bin/env python
"""Times of the marching-cubes extraction on the GPU (profiles/marching_cubes.json).

  * marching cubes alone on a 512^3 analytic torus and on the 512^3 density grid of make_bound_scene(1M, opaque=True): the count call
    (classify + the two scans), the emit call (vertices + faces), vertex normals -- HIP events, median of `--reps` runs -- and the
    algorithmic traffic of the classify pass (4 B read + 2 B written per point) against 8 TB/s;
  * the density sweep's split between the grid-point kernel, the k-NN and the density kernel (events around each, one sweep);
  * the whole foreground + background extraction and its peak memory.

Per-KERNEL times come from running this script with `--mc-only` under `rocprofv3 --kernel-trace --stats`; `--kernel-stats FILE`
copies the marching-cubes kernels of that run's results database into the JSON.  `--out` MERGES into an existing file, so the stages can be
run one at a time (`--only torus,scene,extract`); `--heartbeat FILE` appends a line a minute while the long extraction runs.

    python scripts/marching_cubes_bench.py [--out profiles/marching_cubes.json] [--mc-only] [--only extract] [--resolution 512]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sugar_amd import _lib, extract, field, marching_cubes as mc, synthetic as syn  # noqa: E402
from sugar_amd.knn import knn_points  # noqa: E402

DEV = "cuda:0"
HBM_BYTES_PER_S = 8e12


def timed(fn, reps):
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); out = fn(); b.record(); torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), out


def torus(n):
    h = 1.0 / (n - 1)
    ax = torch.arange(n, dtype=torch.float64, device=DEV) * h
    c = (0.5 + np.sqrt(2.0) / 100, 0.5 + np.sqrt(3.0) / 100, 0.5 + np.pi / 1000)
    R, r = 0.27 + np.sqrt(5.0) / 100, 0.11 + np.sqrt(7.0) / 300
    q = torch.sqrt((ax[:, None] - c[0]) ** 2 + (ax[None, :] - c[1]) ** 2) - R
    vol = torch.empty(n, n, n, dtype=torch.float32, device=DEV)
    for i0 in range(0, n, 64):
        vol[i0:i0 + 64] = (0.3 + r - torch.sqrt(q[i0:i0 + 64, :, None] ** 2 + (ax[None, None, :] - c[2]) ** 2)).float()
    return vol


def mc_times(vol, level, reps):
    mc.marching_cubes(vol, level)                                     # warm
    t_count, (state, counts) = timed(lambda: mc.mc_count(vol, level), reps)
    V, F_ = counts.tolist()
    t_emit, (verts, faces) = timed(lambda: mc.mc_emit(state, V, F_), reps)
    t_norm, _ = timed(lambda: mc.vertex_normals(verts, faces), reps) if V else (0.0, None)
    N = vol.numel()
    out = dict(shape=list(vol.shape), vertices=V, faces=F_, count_ms=t_count, emit_ms=t_emit, vertex_normals_ms=t_norm,
               count_algorithmic_bytes=6 * N, count_share_of_8TBps=6 * N / HBM_BYTES_PER_S / (t_count * 1e-3),
               emit_algorithmic_bytes=2 * N + 12 * V + 24 * F_,
               emit_share_of_8TBps=(2 * N + 12 * V + 24 * F_) / HBM_BYTES_PER_S / (t_emit * 1e-3))
    return out


def sweep_split(X, pts, B, st, K=16, ppp=2_000_000):
    """one sweep with events around the three launches of every slab"""
    lib = _lib.load()
    n1 = X.numel()
    N = n1 ** 3
    packed = field._pack(lib, pts, B.reshape(-1, 9).contiguous(), st)
    buf = torch.empty(min(ppp, N), 3, device=DEV); opac = torch.empty(min(ppp, N), K, device=DEV); dens = torch.empty(min(ppp, N), device=DEV)
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    from sugar_amd._call import ptr as p
    Bm = B.reshape(-1, 9).contiguous()
    ev = []
    for start in range(0, N, ppp):
        n = min(ppp, N - start)
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        e[0].record()
        lib.sgr_grid_points(n1, n1, n1, p(X), p(X), p(X), start, n, p(buf), stream())
        e[1].record()
        idx = knn_points(buf[None, :n], pts[None], K=K).idx[0]
        e[2].record()
        lib.sgr_density_field_forward(n, K, p(buf), p(idx), p(pts), p(Bm), p(st), 1.0, p(opac), p(dens), p(packed), stream())
        e[3].record()
        ev.append(e)
    torch.cuda.synchronize()
    tot = [sum(e[i].elapsed_time(e[i + 1]) for e in ev) for i in range(3)]
    return dict(points=N, gaussians=int(pts.shape[0]), K=K, grid_points_ms=tot[0], knn_ms=tot[1], density_ms=tot[2])


def kernel_stats(path):
    """the kernels of this path in a rocprofv3 kernel trace (the rocpd sqlite database it writes): name -> calls, average / min / max ns"""
    import sqlite3
    cur = sqlite3.connect(path).cursor()
    cols = [r[1] for r in cur.execute("pragma table_info(kernels)")]
    name_col = "name" if "name" in cols else [c for c in cols if "name" in c][0]
    out = {}
    for n, c, avg, mn, mx in cur.execute(f"select {name_col}, count(*), avg(end-start), min(end-start), max(end-start) from kernels group by {name_col}"):
        if "k_mc_" in n or "k_vertex_normals" in n or "k_grid_points" in n:
            out[n.split("::")[-1].split("(")[0]] = dict(calls=c, average_ns=avg, min_ns=mn, max_ns=mx)
    return out


def heartbeat(path):
    import threading
    import time
    stop = threading.Event()

    def beat():
        t0 = time.time()
        while not stop.wait(60.0):
            with open(path, "a") as f:
                f.write(f"running {time.time() - t0:.0f} s\n")
    threading.Thread(target=beat, daemon=True).start()
    return stop


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--mc-only", action="store_true")
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="torus,scene,extract", help="stages to run: torus, scene (sweep split + its marching cubes), extract")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--heartbeat", default=None)
    a = ap.parse_args()
    only = set(a.only.split(",")) if not a.mc_only else {"torus"}
    res = {}
    if a.out and os.path.exists(a.out):
        res = json.load(open(a.out))
    res.update(device=torch.cuda.get_device_name(0), resolution=a.resolution)

    def save():                                   # after every stage: a stage that is cut short keeps the earlier ones
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
    if a.kernel_stats:
        res["kernel_trace_torus"] = kernel_stats(a.kernel_stats)
    if "torus" in only:
        res["torus"] = mc_times(torus(a.resolution), 0.3, a.reps)
        print(json.dumps(res["torus"]), flush=True)
        save()
    if only & {"scene", "extract"}:
        sc = syn.make_bound_scene(a.gaussians, 7, opaque=True).scene
        pts = sc.means3D.to(DEV).contiguous()
        B = field.scaled_rotation(sc.rotations.to(DEV), sc.scales.to(DEV), True)
        st = sc.opacities.to(DEV).reshape(-1).contiguous()
        extent = float(pts.abs().max()) * 1.05
        X = torch.linspace(-1, 1, a.resolution, device=DEV) * extent
        if "scene" in only:
            res["sweep_foreground"] = sweep_split(X, pts, B, st)
            print(json.dumps(res["sweep_foreground"]), flush=True)
            torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats()
            vol = extract.density_grid(X, X, X, pts, B, st)
            torch.cuda.synchronize()
            res["sweep_foreground"]["density_grid_peak_mib"] = torch.cuda.max_memory_allocated() / 2 ** 20
            res["bound_scene"] = mc_times(vol, 0.3, a.reps)
            print(json.dumps(res["bound_scene"]), flush=True)
            save()
            del vol
        if "extract" in only:
            stop = heartbeat(a.heartbeat) if a.heartbeat else None
            torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            t, mesh = timed(lambda: extract.extract_mesh_marching_cubes(pts, sc.scales.to(DEV), sc.rotations.to(DEV), st, sc.shs[:, 0, :].to(DEV),
                                                                        extent, resolution=a.resolution, level=0.3, background=True), 1)
            res["extract_foreground_and_background"] = dict(ms=t, vertices=int(mesh["verts"].shape[0]), faces=int(mesh["faces"].shape[0]),
                                                            peak_extra_mib=(torch.cuda.max_memory_allocated() - base) / 2 ** 20)
            print(json.dumps(res["extract_foreground_and_background"]), flush=True)
            if stop is not None:
                stop.set()
    save()
    return 0


if __name__ == "__main__":
    sys.exit(main())
