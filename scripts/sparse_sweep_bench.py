#!/usr/bin/env python
"""Times of the sparse density-grid sweep against the dense one on the GPU (profiles/sparse_sweep.json).

The scene is make_bound_scene(1M, opaque=True), the grid the extractor's: linspace(-1, 1, R) * extent for the foreground, * 4 extent with
the foreground box blanked for the background.  Every leg is one sweep between two HIP events after one warm call of the same function
at a small resolution (code objects, the allocator), in this one process; `dense` is `extract.density_grid`, the path
`sweep="dense"` takes, `sparse` is `extract.density_grid_sparse`.  A leg records its time, the peak memory above what was allocated
before it, and for a sparse leg the active and total bricks; a sparse leg whose dense partner ran in the same invocation also records
whether marching cubes gives the same mesh from both volumes.

Legs are named <sweep>_<resolution>_<fg|bg>; `--legs` picks them, `--out` MERGES into an existing file so that the long dense legs can
run in invocations of their own.  The dense background at 512^3 is not a leg: it did not finish in 7 minutes when it was tried
(DESIGN.md section 13), and the file says so instead.

Per-KERNEL times: run `--legs sparse_512_fg` under `rocprofv3 --kernel-trace --stats -f csv`, then `--kernel-stats <kernel_stats.csv>` copies
the kernels of that run, grouped into the stages mark, compact, points, k-NN, density and scatter (the leg's warm call at 32^3 and
its marching cubes are in the trace too; the latter is listed as a stage of its own).

    python scripts/sparse_sweep_bench.py [--out profiles/sparse_sweep.json] [--legs sparse_256_fg,dense_256_fg,...]
"""
import argparse
import json
import os
import re
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sugar_amd import extract, field, marching_cubes as mc, synthetic as syn  # noqa: E402

DEV = "cuda:0"
LEVEL = 0.3
DEFAULT_LEGS = "sparse_256_fg,sparse_256_bg,dense_256_fg,sparse_512_fg,sparse_512_bg,dense_512_fg,dense_256_bg"
STAGES = (("mark", ("k_sparse_mark", "k_pack_gaussians")), ("compact", ("k_sparse_compact",)), ("points", ("k_sparse_points",)),
          ("density", ("k_density_",)), ("scatter", ("k_sparse_scatter",)), ("knn", ("k_knn", "k_grid_", "k_ball_")),
          ("marching_cubes_of_the_leg", ("k_mc_",)))


def kernel_stats(path):
    """the kernels of a rocprofv3 `--kernel-trace --stats -f csv` run (its <prefix>_kernel_stats.csv: Name, Calls, TotalDurationNs, ...),
    by stage of the sparse sweep; a kernel that fits no stage by name is listed under `other` (torch's fills, copies and reductions)"""
    import csv
    stages = {}
    for row in csv.DictReader(open(path)):
        own = re.search(r"\bk_[A-Za-z0-9_]+", row["Name"])                      # the library's kernels are all named k_*
        short = own.group(0) if own else re.split(r"[<(]", row["Name"].replace("void ", ""))[0]
        stage = next((s for s, keys in STAGES if any(k in short for k in keys)), "other")
        st = stages.setdefault(stage, dict(total_ms=0.0, kernels={}))
        ms = float(row["TotalDurationNs"]) / 1e6
        st["total_ms"] += ms
        k = st["kernels"].setdefault(short[:80], dict(calls=0, total_ms=0.0))
        k["calls"] += int(row["Calls"])
        k["total_ms"] += ms
    return stages


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--legs", default=DEFAULT_LEGS)
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--kernel-stats", default=None)
    a = ap.parse_args()
    res = json.load(open(a.out)) if a.out and os.path.exists(a.out) else {}

    def save():                                   # after every leg: a leg that is cut short keeps the earlier ones
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
    if a.kernel_stats:
        res["kernel_trace_sparse_512_fg"] = kernel_stats(a.kernel_stats)
        save()
        return 0
    if not torch.cuda.is_available():
        raise SystemExit("sparse_sweep_bench: no GPU; times are measured on the device or not at all")
    res.update(device=torch.cuda.get_device_name(0), gaussians=a.gaussians, level=LEVEL, scene="make_bound_scene(opaque=True), seed 7")
    res["dense_512_bg"] = "parent: unfinished after 7 min, DESIGN.md section 13; not run"
    sc = syn.make_bound_scene(a.gaussians, 7, opaque=True).scene
    pts = sc.means3D.to(DEV).contiguous()
    B = field.scaled_rotation(sc.rotations.to(DEV), sc.scales.to(DEV), True)
    st = sc.opacities.to(DEV).reshape(-1).contiguous()
    extent = float(pts.abs().max()) * 1.05
    res["extent"] = extent

    def sweep(kind, resolution, where):
        X = torch.linspace(-1, 1, resolution, device=DEV) * extent * (extract.BACKGROUND_SCALE if where == "bg" else 1.0)
        box = (-extent, extent) if where == "bg" else None
        if kind == "dense":
            return extract.density_grid(X, X, X, pts, B, st, zero_inside=box), None
        return extract.density_grid_sparse(X, X, X, pts, B, st, LEVEL, zero_inside=box, return_active=True)

    volumes = {}
    for leg in a.legs.split(","):
        kind, resolution, where = leg.split("_")
        resolution = int(resolution)
        sweep(kind, 32, where)                                                # warm
        torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        vol, mask = sweep(kind, resolution, where)
        t1.record(); torch.cuda.synchronize()
        r = dict(ms=t0.elapsed_time(t1), peak_extra_mib=(torch.cuda.max_memory_allocated() - base) / 2 ** 20)
        if mask is not None:
            r.update(active_bricks=int(mask.sum()), total_bricks=mask.numel())
        verts, faces = mc.marching_cubes(vol, LEVEL)
        r.update(vertices=int(verts.shape[0]), faces=int(faces.shape[0]))
        other = volumes.get((resolution, where))
        if other is not None:
            r["same_mesh_as_" + other[0]] = bool(torch.equal(verts, other[1]) and torch.equal(faces, other[2]))
        volumes[(resolution, where)] = (leg, verts, faces)
        del vol, mask
        res[leg] = r
        print(leg, json.dumps(r), flush=True)
        save()
    return 0


if __name__ == "__main__":
    sys.exit(main())
