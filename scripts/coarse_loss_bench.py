#!/usr/bin/env python
"""Times the operations of sugar_amd.coarse_loss (csrc/coarse_loss.hip) against what the unmodified coarse trainer executes for the
same statements today, on the same GPU in the same process, at the size of a coarse-stage SDF iteration: N = 1M samples, P = 2M
Gaussians, K = 16 neighbours, a 1920 x 1080 depth map (the protocol of scripts/sdf_regulariser_bench.py).

Per operation and variant: forward and backward time (device events around the call; the backward is `torch.autograd.grad` over the
retained graph), median of --runs timed runs after --warmup untimed ones, the interquartile range as the spread.  The variants
alternate inside every run, so that a drift of the box hits them alike.  Variants:
    hip      the operation of sugar_amd.coarse_loss
    trainer  the statements of tests/coarse_loss_restatement.py in float32 with the bindings of `install_row_gathers` (the per-Gaussian
             tensors are RowGatherTensors) and `install_regulariser` (the depth lookup is sdf_regulariser.depth_lookup) in place
An operation is adopted only if the HIP forward + backward median is below the trainer variant's by more than the spread (the larger
interquartile range of the two).  For each HIP operation the bytes it must move (inputs read once, outputs written once, the scratch
tables written and read) over its median time is set against the HBM peak of 8.0 TB/s.  The composite is timed on a stand-in model of
the same size (tests/sugar_regulariser_standin.py) against the restated block, both over the same bound methods.  Inputs are seeded
and synthetic (random neighbour lists: no spatial locality, the pessimistic case for the gathers).  GPU needed.

    python scripts/coarse_loss_bench.py --out profiles/coarse_loss.json
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK_TBS = 8.0


def _stats(ms):
    q = statistics.quantiles(ms, n=4)
    return {"median_ms": statistics.median(ms), "p25_ms": q[0], "p75_ms": q[2], "min_ms": min(ms), "max_ms": max(ms), "runs": len(ms)}


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return out, a.elapsed_time(b)


def measure(variants, leaves, warmup, runs, nbytes=None):
    """variants: name -> callable returning the tuple of outputs; leaves: name -> the tensors the backward goes to (None: forward only).
    nbytes: {'forward': .., 'backward': ..} the HIP variant must move"""
    times = {v: {"forward": [], "backward": []} for v in variants}
    for r in range(warmup + runs):
        for name, fn in variants.items():
            outs, t_f = _timed(fn)
            t_b = 0.0
            if leaves is not None:
                _, t_b = _timed(lambda: torch.autograd.grad(outs, leaves[name], [torch.ones_like(o) for o in outs], allow_unused=True))
            del outs
            if r >= warmup:
                times[name]["forward"].append(t_f)
                times[name]["backward"].append(t_b)
    res = {}
    for name, t in times.items():
        total = [f + b for f, b in zip(t["forward"], t["backward"])]
        res[name] = {"forward": _stats(t["forward"]), "forward_plus_backward": _stats(total)}
        if leaves is not None:
            res[name]["backward"] = _stats(t["backward"])
    hip, other = res["hip"]["forward_plus_backward"], res["trainer"]["forward_plus_backward"]
    spread = max(hip["p75_ms"] - hip["p25_ms"], other["p75_ms"] - other["p25_ms"])
    res["verdict"] = {"speedup": other["median_ms"] / hip["median_ms"], "spread_ms": spread,
                      "adopted": bool(other["median_ms"] - hip["median_ms"] > spread)}
    if nbytes:
        res["hip"]["bytes"] = nbytes
        for phase, b in nbytes.items():
            tbs = b / (res["hip"][phase]["median_ms"] * 1e-3) / 1e12
            res["hip"][phase]["tb_per_s"] = tbs
            res["hip"][phase]["fraction_of_hbm_peak"] = tbs / HBM_PEAK_TBS
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1_000_000)
    ap.add_argument("--gaussians", type=int, default=2_000_000)
    ap.add_argument("--neighbours", type=int, default=16)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coarse_loss.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this benchmark measures nothing without one")
    from sugar_amd import coarse_loss as hip, sdf_regulariser, shims, synthetic as syn
    from sugar_amd.row_gather import as_row_gather
    from tests import coarse_loss_restatement as cl
    shims.install()
    dev = torch.device("cuda:0")
    N, P, K, W, H = a.samples, a.gaussians, a.neighbours, a.width, a.height
    g = torch.Generator(device=dev).manual_seed(7)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g)
    leaf = lambda t: t.detach().clone().requires_grad_(True)
    lookup = sdf_regulariser.depth_lookup                                     # what install_regulariser binds
    res = {"size": {"samples": N, "gaussians": P, "neighbours": K, "width": W, "height": H}, "runs": a.runs, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "inputs": "seeded synthetic; random neighbour lists",
           "hbm_peak_tb_per_s": HBM_PEAK_TBS, "ops": {}}

    def report(name, r):
        res["ops"][name] = r
        print(json.dumps({name: dict(r["verdict"], hip_ms=r["hip"]["forward_plus_backward"]["median_ms"],
                                     trainer_ms=r["trainer"]["forward_plus_backward"]["median_ms"])}), flush=True)

    # a camera at the origin looking down +z; the Gaussians and samples in a slab in front of it (5 % of the samples behind znear)
    fx, fy = 2.0 * 1.2 * W / min(W, H), 2.0 * 1.2 * H / min(W, H)
    Pm = torch.tensor([[fx, 0, 0, 0], [0, fy, 0, 0], [0, 0, 1.0, 1.0], [0, 0, -0.01, 0]], device=dev)[None]     # row vectors, w = z
    V = torch.eye(4, device=dev)[None]
    znear = torch.tensor([2.5], device=dev)
    cam_center = torch.zeros(1, 3, device=dev)
    points = leaf(torch.cat((0.9 * rnd(P, 2), 3.0 + 0.3 * rnd(P, 1)), -1))
    quats = torch.nn.functional.normalize(rnd(P, 4), dim=-1)
    scaling = torch.exp(0.5 * rnd(P, 3) - 4.0)
    idx = torch.randint(P, (N,), device=dev, generator=g)
    knn_idx = torch.randint(P, (P, K), device=dev, generator=g)
    image = leaf(3.0 + 0.1 * rnd(H, W, 3))
    depth = image[..., 0]                                                     # the stride-3 view of an [H,W,3] render
    samples = leaf(points.detach()[idx] + 0.02 * rnd(N, 3))
    extent = 4.0

    # ---- surface band (forward only)
    report("surface_band", measure(
        {"hip": lambda: hip.surface_band(points, quats, scaling, V, cam_center, Pm, depth, 2.0),
         "trainer": lambda: cl.surface_band(points.detach(), quats, scaling, V, cam_center, Pm, depth.detach(), 2.0, lookup=lookup)[:2]},
        None, a.warmup, a.runs, {"forward": P * (12 + 16 + 12 + 4 + 1 + 16)}))           # + four taps of 4 bytes

    # ---- estimation losses, both modes
    std = hip.surface_band(points, quats, scaling, V, cam_center, Pm, depth, 2.0)[1]
    sdf, density, beta = leaf(0.1 * rnd(N).abs()), leaf(torch.rand(N, device=dev, generator=g) * 0.9), leaf(0.02 + 0.01 * rnd(N).abs())
    for mode, fields, leaves in (("sdf", dict(sdf=sdf), [samples, sdf, image]), ("density", dict(density=density, beta=beta), [samples, density, beta, image])):
        kw = dict(mode=mode, scale=extent / 10., clamp_max=10. * extent, with_surface=True, **fields)
        n_field = len(fields)
        report("estimation_" + mode, measure(
            {"hip": lambda: hip.estimation_losses(samples, depth, V, Pm, znear, **kw)[:2],
             "trainer": lambda: cl.estimation_losses(samples, depth, V, Pm, znear, lookup=lookup, **kw)[:2]},
            {"hip": leaves, "trainer": leaves}, a.warmup, a.runs,
            {"forward": N * (12 + 4 * n_field + 16), "backward": N * (12 + 4 * n_field + 16 + 12 + 4 * n_field + 16) + H * W * 4}))

    # ---- better normal, through_normal_only on (the trainers' default) and off
    normals = leaf(torch.nn.functional.normalize(rnd(P, 3), dim=-1))
    min_scaling = scaling.min(dim=-1)[0]
    opac = torch.rand(N, K, device=dev, generator=g) * 0.1
    for only in (True, False):
        width = 3 if only else 6
        leaves = [normals] if only else [normals, points, samples]
        pair = K * (8 + 12 + 12 + 4 + 4)                                      # per sample: the neighbour index, its normal, centre, min_scaling, opacity
        entries = N * (K + 1)
        report("better_normal_" + ("normal_only" if only else "full"), measure(
            {"hip": lambda: (hip.better_normal_loss(samples, idx, knn_idx, normals, points, min_scaling, opac, only),),
             "trainer": lambda: (cl.better_normal_loss(samples, idx, knn_idx, as_row_gather(normals), as_row_gather(points), min_scaling, opac, only),)},
            {"hip": leaves, "trainer": leaves}, a.warmup, a.runs,
            {"forward": N * (12 + 8 + 12 + pair),
             "backward": N * (12 + 8 + 12 + pair) + 2 * entries * (8 + 4 * width) + 4 * entries * 8 + P * 4 * width + (0 if only else N * 12)}))
    del normals, opac, sdf, density, beta, samples

    # ---- the composite on a stand-in model of this size against the restated block, over the same bound methods
    from tests.sugar_regulariser_standin import make_module
    from tests.golden.make_sugar_field import p3d_cameras_like_the_reference
    cams = syn.orbit_cameras(W, H)
    state = {"state_points": 0.5 * torch.randn(P, 3).numpy(), "state_scales": (0.5 * torch.randn(P, 3) - 4.0).numpy(),
             "state_quaternions": torch.randn(P, 4).numpy(), "stateall_densities": torch.randn(P, 1).numpy(),
             "state_sh_coordinates_dc": np.zeros((P, 1, 3), np.float32), "state_sh_coordinates_rest": np.zeros((P, 0, 3), np.float32),
             "state_knn_idx": knn_idx.cpu().numpy(), "W": W, "H": H}
    model = make_module(patch_sugar=True, patch_gathers=True).SuGaR(state, dev, cams, p3d_cameras_like_the_reference(cams).to(dev))
    fov_camera = model.nerfmodel.training_cameras.p3d_cameras[3]
    visible = torch.ones(P, dtype=torch.bool, device=dev)
    options = dict(close_gaussian_threshold=1e9, n_samples_for_sdf_regularization=N, cameras_spatial_extent=extent, density_factor=1. / 16.)
    params = [model._points, model._scales, model._quaternions, model.all_densities, image]
    terms = ("sdf_estimation_loss", "sdf_better_normal_loss")

    def block(fn, **more):
        torch.manual_seed(5)
        out = fn(model, fov_camera, depth, visible, **options, **more)
        return tuple(out[k] for k in terms)
    report("composite", measure({"hip": lambda: block(hip.regulariser_terms), "trainer": lambda: block(cl.regulariser_terms, lookup=lookup)},
                                {"hip": params, "trainer": params}, a.warmup, a.runs))

    res["adopted"] = {k: r["verdict"]["adopted"] for k, r in res["ops"].items()}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: {v: r[v]["forward_plus_backward"]["median_ms"] for v in ("hip", "trainer")} for k, r in res["ops"].items()}))
    print(json.dumps({"adopted": res["adopted"]}))


if __name__ == "__main__":
    main()
