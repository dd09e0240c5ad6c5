#!/usr/bin/env python
"""Times the four operations of the SDF regulariser (csrc/sdf_regulariser.hip, the field in csrc/field.hip) against the torch compositions they replace, on the same GPU in the same
process, at the size of a coarse-stage SDF iteration: N = 1M samples, P = 2M Gaussians, K = 16 neighbours, a 1920 x 1080 depth map.

Per operation and variant: forward and backward time (device events around the call; the backward is `torch.autograd.grad` over the
retained graph), median of --runs timed runs after --warmup untimed ones, with the quartiles and extremes as the spread.  The variants
of an operation alternate inside every run, so that a drift of the box hits them alike.  Variants:
    hip      the autograd Function of sugar_amd.sdf_regulariser
    torch    the formulas of tests/sdf_regulariser_restatement.py in float32 (what the reference's tensor code amounts to)
    grid_sample (depth lookup only)   the projection as tensor ops, then torch's own grid_sample: the call the method replaces
    present  (sdf field only)         the binding of `sugar_patch.install` today: HIP density field + the tail as tensor ops
An operation counts as faster only if the HIP forward + backward median is below every other variant's by more than the spread (the
larger interquartile range of the two).  Inputs are seeded and synthetic (random neighbour lists: no spatial locality, the
pessimistic case for the gathers).  GPU needed.

    python scripts/sdf_regulariser_bench.py --out profiles/sdf_regulariser.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def measure(variants, leaves, warmup, runs):
    """variants: name -> callable returning the tuple of differentiable outputs; leaves: the tensors the backward goes to"""
    times = {v: {"forward": [], "backward": []} for v in variants}
    weights = {}
    for r in range(warmup + runs):
        for name, fn in variants.items():
            outs, t_f = _timed(fn)
            if name not in weights:
                weights[name] = [torch.randn_like(o) for o in outs]
            _, t_b = _timed(lambda: torch.autograd.grad(outs, leaves[name], weights[name], allow_unused=True))
            del outs
            if r >= warmup:
                times[name]["forward"].append(t_f)
                times[name]["backward"].append(t_b)
    res = {}
    for name, t in times.items():
        total = [f + b for f, b in zip(t["forward"], t["backward"])]
        res[name] = {"forward": _stats(t["forward"]), "backward": _stats(t["backward"]), "forward_plus_backward": _stats(total)}
    hip = res["hip"]["forward_plus_backward"]
    verdict = {}
    for name in res:
        if name == "hip":
            continue
        other = res[name]["forward_plus_backward"]
        spread = max(hip["p75_ms"] - hip["p25_ms"], other["p75_ms"] - other["p25_ms"])
        verdict[name] = {"speedup": other["median_ms"] / hip["median_ms"], "spread_ms": spread,
                         "hip_faster_by_more_than_the_spread": bool(other["median_ms"] - hip["median_ms"] > spread)}
    res["verdict"] = verdict
    res["hip_faster_than_every_variant"] = all(v["hip_faster_by_more_than_the_spread"] for v in verdict.values())
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sdf_regulariser.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this benchmark measures nothing without one")
    from sugar_amd import field, sdf_regulariser as hip
    from tests import sdf_regulariser_restatement as rs
    dev = torch.device("cuda:0")
    N, P, K, W, H = a.samples, a.gaussians, a.neighbours, a.width, a.height
    g = torch.Generator(device=dev).manual_seed(7)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g)
    leaf = lambda t: t.detach().clone().requires_grad_(True)
    points = leaf(rnd(P, 3))
    quats = leaf(torch.nn.functional.normalize(rnd(P, 4), dim=-1))
    scaling = leaf(torch.exp(0.5 * rnd(P, 3) - 4.0))
    strengths = leaf(torch.sigmoid(rnd(P, 1)))
    idx = torch.randint(P, (N,), device=dev, generator=g)
    noise = rnd(N, 3)
    knn_idx = torch.randint(P, (P, K), device=dev, generator=g)
    res = {"size": {"samples": N, "gaussians": P, "neighbours": K, "width": W, "height": H}, "runs": a.runs, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "inputs": "seeded synthetic; random neighbour lists",
           "ops": {}}

    # ---- sample transform
    per_gaussian = [points, quats, scaling]
    res["ops"]["sample_transform"] = measure(
        {"hip": lambda: (hip.sample_transform(points, quats, scaling, idx, noise, 1.5),),
         "torch": lambda: (rs.sample_transform(points, quats, scaling, idx, noise, 1.5),)},
        {"hip": per_gaussian, "torch": per_gaussian}, a.warmup, a.runs)
    print(json.dumps({"sample_transform": res["ops"]["sample_transform"]["verdict"]}), flush=True)

    # ---- smallest axis
    res["ops"]["smallest_axis"] = measure(
        {"hip": lambda: (hip.smallest_axis(quats, scaling)[0],), "torch": lambda: (rs.smallest_axis(quats, scaling)[0],)},
        {"hip": [quats], "torch": [quats]}, a.warmup, a.runs)
    print(json.dumps({"smallest_axis": res["ops"]["smallest_axis"]["verdict"]}), flush=True)

    # ---- depth lookup: the stride-3 view of an [H,W,3] render, camera-space points in and around the frustum
    image = leaf(3.0 + rnd(H, W, 3))
    fx, fy = 2.0 * 1.2 * W / min(W, H), 2.0 * 1.2 * H / min(W, H)
    Pm = torch.tensor([[fx, 0, 0, 0], [0, fy, 0, 0], [0, 0, 1.0, 1.0], [0, 0, -0.01, 0]], device=dev)[None]     # row vectors, w = z
    cam_pts = leaf(torch.cat((0.9 * rnd(N, 2), 3.0 + 0.3 * rnd(N, 1)), -1))
    m = float(min(H, W))

    def with_grid_sample():
        proj = torch.cat((cam_pts, torch.ones_like(cam_pts[:, :1])), -1) @ Pm[0]
        ndc = proj[:, :2] / proj[:, 3:4]
        grid = torch.stack((-m / W * ndc[:, 0], -m / H * ndc[:, 1]), -1).view(1, -1, 1, 2)
        return (torch.nn.functional.grid_sample(image[..., 0][None, None], grid, mode="bilinear", padding_mode="border",
                                                align_corners=False)[0, 0, :, 0],)
    lookup_leaves = [image, cam_pts]
    res["ops"]["depth_lookup"] = measure(
        {"hip": lambda: (hip.depth_lookup(Pm, image[..., 0], cam_pts),),
         "torch": lambda: (rs.depth_lookup(Pm, image[..., 0], cam_pts),), "grid_sample": with_grid_sample},
        {"hip": lookup_leaves, "torch": lookup_leaves, "grid_sample": lookup_leaves}, a.warmup, a.runs)
    print(json.dumps({"depth_lookup": res["ops"]["depth_lookup"]["verdict"]}), flush=True)

    # ---- sdf field: samples around their Gaussians, the inverse-scaled rotations and min_scaling as leaves
    with torch.no_grad():
        x0 = rs.sample_transform(points, quats, scaling, idx, noise, 1.0)
        B0 = field.scaled_rotation(quats, scaling, True)
        nbr = knn_idx[idx]
        nbr[:, 0] = idx                                   # the sample's own Gaussian leads its list, as in a k-NN table
    x, B, min_scaling = leaf(x0), leaf(B0), leaf(scaling.detach().min(dim=-1)[0])
    field_leaves = [x, points, B, strengths, min_scaling]

    def present():
        o, d = field.density_field(x, nbr, points, B, strengths, 0.2)
        dn = torch.where(d >= 1., d / (d.detach() + 1e-12), d)
        beta = min_scaling[nbr].mean(dim=1)
        sdf = beta * (torch.sqrt(-2. * torch.log(dn.clamp(min=1e-16))) - 0.0)
        return o, d.clone(), beta, sdf
    res["ops"]["sdf_field"] = measure(
        {"hip": lambda: hip.sdf_field(x, nbr, points, B, strengths, min_scaling, 0.2, 1.0, 1e-16),
         "torch": lambda: rs.sdf_field(x, nbr, points, B, strengths, min_scaling, 0.2, 1.0, 1e-16), "present": present},
        {"hip": field_leaves, "torch": field_leaves, "present": field_leaves}, a.warmup, a.runs)
    print(json.dumps({"sdf_field": res["ops"]["sdf_field"]["verdict"]}), flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: {v: r[v]["forward_plus_backward"]["median_ms"] for v in r if isinstance(r[v], dict) and "forward" in r[v]}
                      for k, r in res["ops"].items()}))


if __name__ == "__main__":
    main()
