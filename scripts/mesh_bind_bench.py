#!/usr/bin/env python
"""What the refine stage's mesh binding and normal-consistency regulariser cost per iteration, torch path against HIP path, at
synthetic.make_bound_scene(1M) with n = 1 and n = 6 Gaussians per triangle.  One GPU, one process; device events around every repetition,
the four variants alternating in blocks so that drift hits them alike:

  (a) binding_torch   the three properties forward + backward as the reference evaluates them (sugar_model.py:383-479 over the stand-in
                      Meshes / matrix_to_quaternion): what runs with the binding flag off
  (b) binding_hip     the same through sugar_amd.mesh_bind (three forward and three backward calls)
  (c) nc_torch        the stand-in pytorch3d.loss.mesh_normal_consistency on a freshly built Meshes, forward + backward (flag off)
  (d) nc_hip          the same call with the stand-in's switch on (what --patch-binding sets): a new Meshes from an int32 faces
                      Parameter every repetition, as SuGaR.surface_mesh hands it over, served by sugar_amd.mesh_bind with the cached topology

and every HIP call on its own, with its algorithmic bytes (computed from the shapes below) and the share of 8 TB/s they amount to.

    python scripts/mesh_bind_bench.py [--reps 200] [--n 1 6] [--out profiles/mesh_bind_bench.json]

Kernel-only times: run it under `rocprofv3 --kernel-trace --output-format csv` (one scene, few repetitions) and reduce the trace with
`python scripts/mesh_bind_bench.py --reduce-trace <kernel_trace.csv>`, which prints the median duration of every mesh_bind kernel.
"""
import argparse
import json
import os
import re
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 8e12
BLOCK = 20


def torch_binding(verts, faces, bary, scales, cplx, thickness, n):
    from pytorch3d.structures import Meshes
    from pytorch3d.transforms import matrix_to_quaternion
    N = torch.nn.functional.normalize
    F_ = faces.shape[0]
    points = (verts[faces][:, None] * bary[None]).sum(dim=-2).reshape(F_ * n, 3)
    scaling = torch.cat([thickness * torch.ones(len(scales), 1, device=scales.device), torch.exp(scales)], dim=-1)
    R_0 = N(Meshes(verts=[verts], faces=[faces]).faces_normals_list()[0], dim=-1)
    fv = verts[faces]
    base_R_1 = N(fv[:, 0] - fv[:, 1], dim=-1)
    base_R_2 = N(torch.cross(R_0, base_R_1, dim=-1))
    c = N(cplx, dim=-1).view(F_, n, 2)
    R_1 = c[..., 0:1] * base_R_1[:, None] + c[..., 1:2] * base_R_2[:, None]
    R_2 = -c[..., 1:2] * base_R_1[:, None] + c[..., 0:1] * base_R_2[:, None]
    R = torch.cat([R_0[:, None, ..., None].expand(-1, n, -1, -1).clone(), R_1[..., None], R_2[..., None]], dim=-1).view(-1, 3, 3)
    return points, scaling, N(matrix_to_quaternion(R), dim=-1)


def algorithmic_bytes(F_, n, V, n_pairs):
    """bytes each HIP call must move: every input read once, every output written once, scratch written and read once"""
    P = F_ * n
    face = F_ * (12 + 36)                                # the face's indices and its three vertices
    csr = 4 * (V + 1) + 4 * 3 * F_
    gather = 36 * F_ * 2 + csr + 12 * V                  # contributions written and read, the list, the vertex gradient
    return {
        "points_fwd": face + 12 * P, "scaling_fwd": (8 + 12) * P, "quaternions_fwd": face + (8 + 16) * P,
        "points_bwd": 12 * P + 12 * F_ + gather, "scaling_bwd": (12 + 8 + 8) * P, "quaternions_bwd": face + (16 + 8 + 8) * P + gather,
        "nc_fwd": n_pairs * (16 + 48), "nc_bwd": n_pairs * (16 + 48) + 48 * n_pairs * 2 + 4 * (V + 1) + 16 * n_pairs + 12 * V,
    }


def timed(fn, start, stop):
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


def summary(ms):
    qs = statistics.quantiles(ms, n=4)
    blocks = [statistics.median(ms[i:i + BLOCK]) for i in range(0, len(ms), BLOCK)]
    return {"median_ms": statistics.median(ms), "p25_ms": qs[0], "p75_ms": qs[2], "min_ms": min(ms),
            "block_medians_ms": blocks, "spread_ms": max(blocks) - min(blocks)}


def bench(n, reps, dev):
    from pytorch3d.loss import mesh_normal_consistency
    from pytorch3d.structures import Meshes
    from sugar_amd import mesh_bind, synthetic as syn
    bs = syn.make_bound_scene(1_000_000, 5, n_per_triangle=n)
    faces = bs.faces.to(dev)
    bary = torch.tensor(syn._BARY[n][0], dtype=torch.float32, device=dev)[..., None]
    thickness = torch.tensor(bs.thickness, dtype=torch.float32, device=dev)
    verts = bs.verts.to(dev).requires_grad_(True)
    scales = torch.log(bs.plane_scales).to(dev).requires_grad_(True)
    cplx = bs.complex_rot.to(dev).requires_grad_(True)
    P = faces.shape[0] * n
    g = torch.Generator().manual_seed(3)
    cots = [torch.randn(P, k, generator=g).to(dev) for k in (3, 3, 4)]
    one = torch.ones((), device=dev)
    topo = mesh_bind.MeshTopology.get(faces, verts.shape[0])
    builds = []
    real_init = mesh_bind.MeshTopology.__init__
    mesh_bind.MeshTopology.__init__ = lambda self, *a, **k: builds.append(1) or real_init(self, *a, **k)

    def backward(outs, grads):
        torch.autograd.backward(outs, grads, inputs=[verts, scales, cplx])
        verts.grad = scales.grad = cplx.grad = None

    def binding_torch():
        backward(list(torch_binding(verts, faces, bary, scales, cplx, thickness, n)), cots)

    def binding_hip():
        backward([mesh_bind.bound_points(verts, faces, bary), mesh_bind.bound_scaling(scales, thickness),
                  mesh_bind.bound_quaternions(verts, faces, cplx, n)], cots)

    def nc_torch():
        torch.autograd.backward([mesh_normal_consistency(Meshes(verts=[verts], faces=[faces]))], [one], inputs=[verts])
        verts.grad = None

    import pytorch3d.loss as p3d_loss
    faces_param = torch.nn.Parameter(faces.to(torch.int32), requires_grad=False)     # open3d's triangles are int32

    def nc_hip():
        p3d_loss.USE_HIP_NORMAL_CONSISTENCY = True
        try:
            loss = mesh_normal_consistency(Meshes(verts=[verts], faces=[faces_param]))
        finally:
            p3d_loss.USE_HIP_NORMAL_CONSISTENCY = False
        torch.autograd.backward([loss], [one], inputs=[verts])
        verts.grad = None

    variants = {"binding_torch": binding_torch, "binding_hip": binding_hip, "nc_torch": nc_torch, "nc_hip": nc_hip}
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for fn in variants.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(reps // BLOCK):
        for k, fn in variants.items():
            times[k] += [timed(fn, start, stop) for _ in range(BLOCK)]
    out = {"n_per_triangle": n, "faces": int(faces.shape[0]), "vertices": int(verts.shape[0]), "gaussians": int(P),
           "n_pairs": topo.n_pairs, "repetitions": len(times["nc_hip"]), "variants": {k: summary(v) for k, v in times.items()}}
    mesh_bind.MeshTopology.__init__ = real_init
    out["topology_builds_during_the_timed_repetitions"] = len(builds) - 1      # (one build in the warm-up: the int32 Parameter)
    v = out["variants"]
    for name, slow, fast in (("binding", "binding_torch", "binding_hip"), ("normal_consistency", "nc_torch", "nc_hip")):
        margin = v[slow]["median_ms"] - v[fast]["median_ms"]
        out[name + "_speedup"] = v[slow]["median_ms"] / v[fast]["median_ms"]
        out[name + "_faster_by_more_than_the_spread"] = bool(margin > max(v[slow]["spread_ms"], v[fast]["spread_ms"]))
    # every HIP call on its own
    calls = {}
    fwd = {"points_fwd": lambda: mesh_bind.bound_points(verts, faces, bary), "scaling_fwd": lambda: mesh_bind.bound_scaling(scales, thickness),
           "quaternions_fwd": lambda: mesh_bind.bound_quaternions(verts, faces, cplx, n),
           "nc_fwd": lambda: mesh_bind.normal_consistency(verts, faces)}
    held = {k: f() for k, f in fwd.items()}
    grads = {"points_fwd": cots[0], "scaling_fwd": cots[1], "quaternions_fwd": cots[2], "nc_fwd": one}
    wrt = {"points_fwd": [verts], "scaling_fwd": [scales], "quaternions_fwd": [verts, cplx], "nc_fwd": [verts]}
    for k, f in fwd.items():
        with torch.no_grad():
            calls[k] = [timed(f, start, stop) for _ in range(reps)]
        kb = k.replace("_fwd", "_bwd")
        calls[kb] = [timed(lambda: torch.autograd.grad(held[k], wrt[k], grads[k], retain_graph=True), start, stop) for _ in range(reps)]
    nbytes = algorithmic_bytes(int(faces.shape[0]), n, int(verts.shape[0]), topo.n_pairs)
    out["hip_calls"] = {}
    for k, ms in calls.items():
        med = statistics.median(ms)
        out["hip_calls"][k] = {"median_ms": med, "algorithmic_bytes": nbytes[k], "per_call_fraction_of_8TBps": nbytes[k] / (med * 1e-3) / HBM_BYTES_PER_S}
    return out


def reduce_trace(path):
    """{kernel: (calls, median us, min us)} of the k_bind_* / k_nc_* / k_gather_vertex rows of a rocprofv3 kernel trace, as JSON"""
    import csv
    durations = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            m = re.search(r"k_(bind_forward|bind_backward|nc_forward|nc_sum|nc_backward|gather_vertex)", row.get("Kernel_Name", ""))
            if m:
                durations.setdefault(m.group(0), []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1000.0)
    print(json.dumps({k: {"calls": len(v), "median_us": statistics.median(v), "min_us": min(v)} for k, v in sorted(durations.items())}, indent=1))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--n", type=int, nargs="+", default=[1, 6], help="Gaussians per triangle of the scenes to run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_bind_bench.json"))
    ap.add_argument("--reduce-trace", metavar="CSV", help="print the median duration per mesh_bind kernel of a rocprofv3 kernel trace")
    a = ap.parse_args()
    if a.reduce_trace:
        return reduce_trace(a.reduce_trace)
    if not torch.cuda.is_available():
        raise SystemExit("mesh_bind_bench needs a ROCm GPU: a timing without one says nothing")
    from sugar_amd import shims
    shims.install()
    dev = torch.device("cuda")
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "note": "median and quartiles over the repetitions of device-event timings (forward + backward, ms); spread_ms = range of the "
                   "medians of blocks of %d repetitions, the four variants alternating block by block; hip_calls: one call each "
                   "(PER CALL, not per kernel: launch cost, and for the backward calls autograd's dispatch and the output allocations, are inside), "
                   "bytes from the shapes" % BLOCK,
           "scenes": [bench(n, max(a.reps, BLOCK), dev) for n in a.n]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
