#!/usr/bin/env python
"""Times of the mesh decimation on the GPU (profiles/mesh_decimate.json).

The 512 x 384 x 640 torus of tests/test_gpu_marching_cubes.py (586 284 faces) decimated to `--target` (200 000) faces: the total time
(HIP events, median of `--reps` runs), the time per round, the number of rounds, the peak extra memory, and `clean` on the result.

Per-KERNEL times come from running this script with `--reps 1` under `rocprofv3 --kernel-trace --stats` (a run of its own).

    python scripts/mesh_decimate_bench.py [--out profiles/mesh_decimate.json] [--target 200000] [--reps 5]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sugar_amd import decimate as dec, marching_cubes as mc  # noqa: E402

DEV = "cuda:0"
LEVEL = 0.3


def torus_mesh(nx=512, ny=384, nz=640):
    h = 1.0 / (nz - 1)
    ax = [torch.arange(n, dtype=torch.float64, device=DEV) * h for n in (nx, ny, nz)]
    c = (0.4 + np.sqrt(2.0) / 100, 0.29 + np.sqrt(3.0) / 100, 0.5 + np.pi / 1000)
    R, r = 0.19 + np.sqrt(5.0) / 100, 0.05 + np.sqrt(7.0) / 300
    q = torch.sqrt((ax[0][:, None] - c[0]) ** 2 + (ax[1][None, :] - c[1]) ** 2) - R
    vol = torch.empty(nx, ny, nz, dtype=torch.float32, device=DEV)
    for i0 in range(0, nx, 64):
        vol[i0:i0 + 64] = (LEVEL + r - torch.sqrt(q[i0:i0 + 64, :, None] ** 2 + (ax[2][None, None, :] - c[2]) ** 2)).float()
    verts, faces = mc.marching_cubes(vol, LEVEL)
    return verts * h, faces


def timed(fn, reps):
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); out = fn(); b.record(); torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "mesh_decimate.json"))
    ap.add_argument("--target", type=int, default=200_000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_decimate_bench: needs a GPU; nothing is measured without one")
    verts, faces = torus_mesh()
    dec.decimate(verts, faces, faces.shape[0] - 1000)                  # warm: code objects, the allocator
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ms, (v, f, info) = timed(lambda: dec.decimate(verts, faces, a.target), a.reps)
    peak = torch.cuda.max_memory_allocated() - base
    clean_ms, (cv, cf, _) = timed(lambda: dec.clean(v, f), a.reps)
    out = dict(mesh="torus 512x384x640", vertices_in=int(verts.shape[0]), faces_in=int(faces.shape[0]), target=a.target,
               vertices_out=int(v.shape[0]), faces_out=int(f.shape[0]), rounds=info["rounds"], round_limit=info["round_limit"],
               target_met=info["target_met"], decimate_ms=ms, ms_per_round=ms / max(info["rounds"], 1), reps=a.reps,
               peak_extra_mib=peak / 2 ** 20, clean_ms=clean_ms, clean_faces_out=int(cf.shape[0]), clean_vertices_out=int(cv.shape[0]),
               device=torch.cuda.get_device_name(0))
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
