#!/usr/bin/env python
"""Measures what the native coarse-SDF trainer adds (sugar_amd.coarse_draw, coarse_loss.opacity_entropy, coarse_train.CoarseTrainer)
against what runs for the same work today, on the same GPU in the same session:

  draw_samples      at P = 2M Gaussians (half of them masked), N = 1M samples, against the torch statements it replaces
                    (sugar_patch.sample_points_in_gaussians' draws: the masked scaling, `torch.multinomial` over the compacted
                    ones, `arange(P)[mask][idx]`, `randn`)
  opacity_entropy   forward + backward at P = 2M against the trainer's torch statements (coarse_sdf.py:543-551)
  iteration time    after 9 000 at 2M Gaussians / 64 cameras of 1920 x 1080: `CoarseTrainer` against the unmodified coarse_sdf.py with
                    every binding (what scripts/run_reference_trainer.py --patch-losses --patch-optimizer --patch-gathers
                    --patch-densifier --patch-regulariser runs), both from 7 000 to --stop-at on the same synthetic dataset
                    (oracle/reference_trainer.write_dataset); their losses at 9 050, 9 100, 9 150 and 9 200 side by side (informative:
                    the draws differ by design)

The two operations: device events around the call, median of --runs timed runs after --warmup untimed ones, the interquartile range
as the spread, the variants alternating inside every run (the protocol of scripts/coarse_loss_bench.py).  An operation is adopted
only if its median is below the torch statements' by more than the spread (the larger interquartile range of the two).  The
iteration time is host time between iteration starts over 9 050 .. --stop-at (every SDF iteration of either loop waits for the device
once, so the stamps follow the device); for `CoarseTrainer` the median and interquartile range of the single iterations are given
too.  The two loops run one after the other in one process, `CoarseTrainer` first, or the reference first with --reference-first:
the pair of orders shows what the position in the process is worth.  GPU needed; the iteration-time part needs the reference's sources as `build()` stages them (--skip-trainers leaves it out).

    python scripts/coarse_train_bench.py --out profiles/coarse_train.json
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

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


def measure(variants, warmup, runs):
    """variants: name -> callable; alternating inside every run"""
    times = {v: [] for v in variants}
    for r in range(warmup + runs):
        for name, fn in variants.items():
            out, t = _timed(fn)
            del out
            if r >= warmup:
                times[name].append(t)
    res = {name: _stats(t) for name, t in times.items()}
    hip, other = res["hip"], res["torch"]
    spread = max(hip["p75_ms"] - hip["p25_ms"], other["p75_ms"] - other["p25_ms"])
    res["verdict"] = {"speedup": other["median_ms"] / hip["median_ms"], "spread_ms": spread,
                      "adopted": bool(other["median_ms"] - hip["median_ms"] > spread)}
    return res


def bench_ops(a, res):
    from sugar_amd import coarse_draw, coarse_loss
    dev = torch.device("cuda:0")
    P, N = a.gaussians, a.samples
    g = torch.Generator(device=dev).manual_seed(7)
    mask = torch.rand(P, device=dev, generator=g) < 0.5
    scaling = torch.exp(0.5 * torch.randn(P, 3, device=dev, generator=g) - 4.0)
    calls = [0]

    def hip_draw():
        calls[0] += 1
        return coarse_draw.draw_samples(mask, N, 7, calls[0])

    def torch_draw():                                                          # sugar_patch.sample_points_in_gaussians' draws
        with torch.no_grad():
            masked = scaling[mask]
            areas = torch.ones_like(masked[..., 0]).abs()
            cum_probs = areas / areas.sum(dim=-1, keepdim=True)
            random_indices = torch.multinomial(cum_probs, num_samples=N, replacement=True)
            valid_indices = torch.arange(P, device=dev)[mask]
            random_indices = valid_indices[random_indices]
            return random_indices, torch.randn_like(scaling.new_empty(random_indices.shape + (3,)))
    res["ops"]["draw_samples"] = measure({"hip": hip_draw, "torch": torch_draw}, a.warmup, a.runs)
    res["ops"]["draw_samples"]["bytes_moved"] = P * (1 + 1) + int(mask.sum()) * 4 + N * (4 + 20)      # the mask twice, ids, a gather + outputs

    opac = torch.sigmoid(2.0 * torch.randn(P, 1, device=dev, generator=g))
    visible = torch.rand(P, device=dev, generator=g) < 0.6
    factor = torch.tensor(0.1, device=dev)

    def hip_entropy():
        o = opac.clone().requires_grad_(True)
        return torch.autograd.grad(factor * coarse_loss.opacity_entropy(o, visible), o)

    def torch_entropy():
        o = opac.clone().requires_grad_(True)
        vis_opacities = o[visible]
        value = (- vis_opacities * torch.log(vis_opacities + 1e-10) - (1 - vis_opacities) * torch.log(1 - vis_opacities + 1e-10)).mean()
        return torch.autograd.grad(factor * value, o)
    res["ops"]["opacity_entropy"] = measure({"hip": hip_entropy, "torch": torch_entropy}, a.warmup, a.runs)
    for name, r in res["ops"].items():
        print(json.dumps({name: dict(r["verdict"], hip_ms=r["hip"]["median_ms"], torch_ms=r["torch"]["median_ms"])}), flush=True)


def _rate(stamps, first, lo, hi):
    a, b = lo - first, min(hi - first, len(stamps) - 1)
    return float((b - a) / (stamps[b] - stamps[a])) if b > a else None


def bench_trainers(a, res):
    from PIL import Image
    import numpy as np
    from oracle import reference_trainer as rt
    from sugar_amd import coarse_train, io as sio, sugar_patch
    from sugar_amd.coarse_model import CoarseModel
    from tests import ref_env
    work = tempfile.mkdtemp(prefix="coarse_train_bench_")
    try:
        data = rt.write_dataset(work, P=a.gaussians, n_cams=a.cameras, W=a.width, H=a.height)
        size = {"gaussians": a.gaussians, "cameras": a.cameras, "width": a.width, "height": a.height, "stop_at": a.stop_at}

        def run_native():
            # ---- CoarseTrainer
            cams, names = sio.cameras_from_json(os.path.join(data.checkpoint_path, "cameras.json"))
            images = []
            for name in names:
                with Image.open(os.path.join(data.scene_path, "images", name + ".png")) as im:
                    images.append(torch.from_numpy(np.asarray(im.convert("RGB"), dtype=np.uint8).astype(np.float32) / np.float32(255.0)))
            ply = os.path.join(data.checkpoint_path, "point_cloud", "iteration_7000", "point_cloud.ply")
            model = CoarseModel.from_gaussian_ply(ply, cams, device="cuda:0", seed=0)
            trainer = coarse_train.CoarseTrainer(model, cams, images, num_iterations=a.stop_at, n_samples_for_sdf_regularization=a.samples)
            stamps, losses = [], []
            step = trainer.step

            def stamped(iteration, camera_index, **kw):
                stamps.append(time.time())
                return step(iteration, camera_index, **kw)
            trainer.step = stamped
            t0 = time.time()
            trainer.run(7000, a.stop_at, seed=0, log=lambda line, *rest: losses.append(line))
            torch.cuda.synchronize()
            stamps.append(time.time())
            single = [1e3 * (stamps[i + 1] - stamps[i]) for i in range(9050 - 7001, len(stamps) - 1)]
            native = {"wall_s": time.time() - t0, "iterations_run": len(stamps) - 1, "gaussians_after_pruning": model.n_points,
                      "it_per_s_before_9000": _rate(stamps, 7001, 7050, 8950), "it_per_s_after_9000": _rate(stamps, 7001, 9050, a.stop_at + 1),
                      "iteration_ms_after_9050": _stats(single) if len(single) >= 2 else None,
                      "losses": [[int(m.group(2)), float(m.group(1))] for m in map(rt.LOSS_LINE.search, losses) if m],
                      "n_masked_last": trainer.n_masked}
            res["trainers"]["coarse_trainer"] = native
            print(json.dumps({"coarse_trainer": {k: native[k] for k in ("it_per_s_before_9000", "it_per_s_after_9000", "gaussians_after_pruning")}}),
                  flush=True)
            del trainer, model, images
            torch.cuda.empty_cache()
            return native

        def run_reference():
            # ---- the unmodified coarse_sdf.py with every binding
            sm = ref_env.import_sugar_model()
            sugar_patch.install_regulariser(sm)
            try:
                ref = rt.run(data, os.path.join(work, "out"), stop_at=a.stop_at, patch_sugar=True, patch_losses=True, patch_optimizer=True,
                             patch_gathers=True, patch_densifier=True, log_path=os.path.join(work, "reference_console.log"))
            finally:
                sugar_patch.uninstall_regulariser(sm)
            ref.pop("profile_table", None)
            ref.pop("log", None)
            res["trainers"]["reference_all_bindings"] = ref
            return ref

        res["trainers"] = {"size": size, "order": ["reference_all_bindings", "coarse_trainer"] if a.reference_first else
                           ["coarse_trainer", "reference_all_bindings"]}
        if a.reference_first:
            ref, native = run_reference(), run_native()
        else:
            native, ref = run_native(), run_reference()
        by_it = lambda rows: {int(i): float(v) for i, v in rows}
        mine, theirs = by_it(native["losses"]), by_it(ref["losses"])
        res["trainers"]["losses_side_by_side"] = {str(i): {"coarse_trainer": mine.get(i), "reference_all_bindings": theirs.get(i)}
                                                  for i in (9050, 9100, 9150, 9200)}
        if native["it_per_s_after_9000"] and ref.get("it_per_s_after_9000"):
            res["trainers"]["speedup_after_9000"] = native["it_per_s_after_9000"] / ref["it_per_s_after_9000"]
        print(json.dumps({"reference_all_bindings": {k: ref.get(k) for k in ("it_per_s_before_9000", "it_per_s_after_9000",
                                                                               "gaussians_after_pruning")},
                          "losses": res["trainers"]["losses_side_by_side"]}), flush=True)
    finally:
        shutil.rmtree(work, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1_000_000)
    ap.add_argument("--gaussians", type=int, default=2_000_000)
    ap.add_argument("--cameras", type=int, default=64)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--stop-at", type=int, default=9200)
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reference-first", action="store_true", help="run the reference trainer before CoarseTrainer (the other order of the pair)")
    ap.add_argument("--skip-ops", action="store_true")
    ap.add_argument("--skip-trainers", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coarse_train.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this benchmark measures nothing without one")
    res = {"size": {"samples": a.samples, "gaussians": a.gaussians}, "runs": a.runs, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "ops": {}}

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    if not a.skip_ops:
        bench_ops(a, res)
        res["adopted"] = {k: r["verdict"]["adopted"] for k, r in res["ops"].items()}
        write()
    if not a.skip_trainers:
        bench_trainers(a, res)
    write()
    print(json.dumps({"adopted": res.get("adopted"), "speedup_after_9000": res.get("trainers", {}).get("speedup_after_9000")}))


if __name__ == "__main__":
    main()
