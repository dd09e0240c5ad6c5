#!/usr/bin/env python
"""What the border-face peel of the refined-mesh export costs: the native peel (sugar_amd.mesh_postprocess, 5 iterations) and its
topology build, timed separately on an n x n-cell sheet at about 100k and about 2M faces; and, at about 100k faces only, the
reference's formulation of the same loop (refined_mesh.py:133-147: `knn_points` with K = 2 over the float pairs of the live faces, once
per iteration) through the 2-D `knn_points` of this package, on the same GPU.

    python scripts/mesh_postprocess_bench.py [--out profiles/mesh_postprocess.json]

Every step runs in a child process of its own under its own time limit, the k-NN route last.  A step that does not finish within its
limit is recorded as such, with the iterations it did finish; the limit is not enlarged.  Times are host-clock around work that ends in
a device synchronise, after a warm-up; the peel is also given with the bytes its two kernels must move per iteration (from the shapes).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ITERATIONS = 5
SIZES = {"100k": 224, "2M": 1000}           # cells per side: 2 n^2 faces = 100 352 and 2 000 000
LIMITS_S = {"native": 120, "knn": 150}


def sheet(n, dev):
    import torch
    i, j = torch.meshgrid(torch.arange(n, device=dev), torch.arange(n, device=dev), indexing="xy")
    a = (j * (n + 1) + i).reshape(-1)
    b, c, d = a + 1, a + n + 2, a + n + 1
    return torch.stack([torch.stack([a, b, c], -1), torch.stack([a, c, d], -1)], dim=1).reshape(-1, 3).contiguous()


def timed(fn, reps):
    import torch
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "repetitions": reps}


def step_native(n):
    import torch
    from sugar_amd.mesh_postprocess import PeelTopology, peel_border_faces
    dev = torch.device("cuda")
    faces = sheet(n, dev)
    F_ = int(faces.shape[0])
    topo = PeelTopology(faces)
    for _ in range(3):
        peel_border_faces(faces, ITERATIONS, topology=topo)
        PeelTopology(faces)
    E = topo.n_edges
    out = {"cells_per_side": n, "faces": F_, "edges": E, "iterations": ITERATIONS,
           "topology_build": timed(lambda: PeelTopology(faces), 20),
           "peel": timed(lambda: peel_border_faces(faces, ITERATIONS, topology=topo), 100),
           "peel_with_topology_build": timed(lambda: peel_border_faces(faces, ITERATIONS), 20)}
    # per iteration: the count kernel reads offsets, items and a mask byte per slot and writes a byte per edge; the test kernel reads a
    # mask byte and three edge ids per face and a count byte per slot, and writes a mask byte per face
    per_iteration = (4 * (E + 1) + 12 * F_ + 3 * F_ + E) + (F_ + 12 * F_ + 3 * F_ + F_)
    out["peel"]["algorithmic_bytes"] = ITERATIONS * per_iteration
    out["peel"]["bytes_per_second"] = ITERATIONS * per_iteration / (out["peel"]["median_ms"] * 1e-3)
    out["live_after"] = int(peel_border_faces(faces, ITERATIONS, topology=topo).sum())
    print(json.dumps(out), flush=True)


def step_knn(n):
    """the reference's loop as written; one JSON line per finished iteration, so that a run cut off at its limit leaves what it did"""
    import torch
    from sugar_amd.knn import knn_points
    from sugar_amd.mesh_postprocess import peel_border_faces
    dev = torch.device("cuda")
    new_faces = sheet(n, dev)
    warm = torch.rand(1, 5000, 2, device=dev)
    knn_points(warm, warm, K=2)                                   # loads the code objects
    edges0 = new_faces[..., None, (0, 1)].sort(dim=-1)[0]
    edges1 = new_faces[..., None, (1, 2)].sort(dim=-1)[0]
    edges2 = new_faces[..., None, (2, 0)].sort(dim=-1)[0]
    all_edges = torch.cat([edges0, edges1, edges2], dim=-2)
    face_mask = torch.ones(len(new_faces), dtype=torch.bool, device=dev)
    torch.cuda.synchronize()
    print(json.dumps({"cells_per_side": n, "faces": int(new_faces.shape[0]), "points_first_iteration": 3 * int(new_faces.shape[0])}), flush=True)
    for i in range(ITERATIONS):
        t0 = time.perf_counter()
        pts = all_edges[face_mask].view(1, -1, 2).float()
        edges_neighbors = knn_points(pts, pts, K=2)
        is_inside = (edges_neighbors.dists[0][..., 1].view(-1, 3) < 0.01).all(-1)
        face_mask[face_mask.clone()] = is_inside
        torch.cuda.synchronize()
        print(json.dumps({"iteration": i, "ms": (time.perf_counter() - t0) * 1e3, "live_after": int(face_mask.sum())}), flush=True)
    same = bool(torch.equal(face_mask, peel_border_faces(new_faces, ITERATIONS)))
    print(json.dumps({"equals_native_peel": same}), flush=True)


def run_step(name, n):
    """the step in a fresh process under its limit: (finished, its JSON lines)"""
    proc = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--step", name, "--cells", str(n)], stdout=subprocess.PIPE, text=True)
    try:
        out, _ = proc.communicate(timeout=LIMITS_S[name])
        finished = proc.returncode == 0
    except subprocess.TimeoutExpired:
        proc.kill()
        out, _ = proc.communicate()
        finished = False
    lines = [json.loads(l) for l in (out or "").splitlines() if l.startswith("{")]
    return finished, lines, proc.returncode


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_postprocess.json"))
    ap.add_argument("--step", choices=("native", "knn"), help="(internal) run one step in this process")
    ap.add_argument("--cells", type=int, default=SIZES["100k"])
    a = ap.parse_args()
    if a.step:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("mesh_postprocess_bench needs a ROCm GPU: a timing without one says nothing")
        print(json.dumps({"device": torch.cuda.get_device_name(0), "torch": torch.__version__}), flush=True)
        return {"native": step_native, "knn": step_knn}[a.step](a.cells)
    res = {"device": None, "torch": None, "limits_s": LIMITS_S,       # (this process never opens the GPU: the steps do, one at a time)
           "note": "host clock around work that ends in a device synchronise, per CALL (launch cost and torch's allocations inside); the peel "
                   "is %d iterations with the topology prebuilt; the k-NN route is the reference's loop through the 2-D knn_points, one "
                   "k-NN build per iteration over the live faces' pairs" % ITERATIONS,
           "native": {}, "knn_route": None}
    for label, n in SIZES.items():
        finished, lines, rc = run_step("native", n)
        if lines and "device" in lines[0]:
            res.update(lines[0])
        if not finished or len(lines) < 2:       # nothing more is started on a device a step did not come back from; nothing is written
            raise SystemExit(f"the native step at {label} faces did not finish (return code {rc}): no measurement")
        res["native"][label] = lines[-1]
    finished, lines, rc = run_step("knn", SIZES["100k"])
    its = [l for l in lines if "iteration" in l]
    res["knn_route"] = {**next((l for l in lines if "points_first_iteration" in l), {}), "finished_within_limit": finished,
                        "returncode": rc, "iterations": its, "total_ms": sum(l["ms"] for l in its) if finished else None,
                        **next((l for l in lines if "equals_native_peel" in l), {})}
    if finished:
        res["knn_route"]["native_peel_speedup_with_topology_build"] = (
            res["knn_route"]["total_ms"] / res["native"]["100k"]["peel_with_topology_build"]["median_ms"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
