#!/usr/bin/env python
"""Measures the native density regulariser (coarse_loss.projection_estimation_losses, CoarseTrainer(regulariser='density')) against
what runs for the same work today, on the same GPU in the same session:

  projection term   forward + backward of the estimation term of coarse_density.py:651-691 (mode 'density') at N = 1M samples /
                    P = 2M Gaussians, against the torch statements it replaces with the row-gather binding on the points and the
                    normals (sugar_amd.row_gather: what the unmodified trainer runs under `install_row_gathers`).  Bytes moved over
                    the median time as a share of the HBM peak (--hbm-peak-gbs): by count a sample reads 12 (x) + 8 (idx) + 24
                    (two gathered rows) + 8 (density, beta) = 52 B forward; the backward reads them again, writes 24 B per sample
                    (dfield, dbeta, dsamples, dest), and the fold re-reads 24 B per sample and writes 24 B per Gaussian.
  iteration time    after 9 000 at 2M Gaussians / 64 cameras of 1920 x 1080 / 1M samples: `CoarseTrainer(regulariser='density')`
                    against the unmodified coarse_density.py with every binding, both from 7 000 to --stop-at on the same synthetic
                    dataset (oracle/reference_trainer.write_dataset)

The protocol is scripts/coarse_train_bench.py's: device events, --warmup untimed runs, the median of --runs timed runs with the
variants alternating inside every run, the interquartile range as the spread; the two loops one after the other in one process,
the native one first, or the reference first with --reference-first.  GPU needed; the iteration-time part needs the reference's
sources as `build()` stages them (--skip-trainers leaves it out).

    python scripts/coarse_density_bench.py --out profiles/coarse_density.json
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from coarse_train_bench import _rate, _stats, measure  # noqa: E402


def term_inputs(P, N, dev, seed=7):
    g = torch.Generator(device=dev).manual_seed(seed)
    points = 0.6 * torch.nn.functional.normalize(torch.randn(P, 3, device=dev, generator=g), dim=-1)
    normals = torch.nn.functional.normalize(torch.randn(P, 3, device=dev, generator=g), dim=-1)
    idx = torch.randint(0, P, (N,), device=dev, generator=g)
    x = points[idx] + 0.01 * torch.randn(N, 3, device=dev, generator=g)
    density = 0.05 + 0.9 * torch.rand(N, device=dev, generator=g)
    beta = 0.005 + 0.01 * torch.rand(N, device=dev, generator=g)
    return x, idx, points, normals, density, beta


def torch_term(x, idx, points, normals, density, beta):
    """coarse_density.py:655-656, :684-691 as the trainer writes them; `points` / `normals` may be RowGatherTensors"""
    own_normals = normals[idx]
    estimation = ((x - points[idx]) * own_normals).sum(dim=-1)
    target = torch.exp(-0.5 * estimation.pow(2) / beta.pow(2))
    return (density - target).abs().mean()


def bench_term(a, res):
    from sugar_amd import coarse_loss
    from sugar_amd.row_gather import as_row_gather
    dev = torch.device("cuda:0")
    P, N = a.gaussians, a.samples
    x, idx, points, normals, density, beta = term_inputs(P, N, dev)
    factor = torch.tensor(0.2, device=dev)

    def leaves():
        return [t.clone().requires_grad_(True) for t in (x, density, beta, points, normals)]

    def hip():
        lx, ld, lb, lp, ln = ls = leaves()
        est, _ = coarse_loss.projection_estimation_losses(lx, idx, lp, ln, density=ld, beta=lb)
        return torch.autograd.grad(factor * est, ls)

    def torch_statements():
        lx, ld, lb, lp, ln = ls = leaves()
        return torch.autograd.grad(factor * torch_term(lx, idx, as_row_gather(lp), as_row_gather(ln), ld, lb), ls)
    got = [g.clone() for g in hip()]
    want = [g.clone() for g in torch_statements()]
    res["ops"]["projection_term"] = r = measure({"hip": hip, "torch": torch_statements}, a.warmup, a.runs)
    r["agreement"] = [float((u - v).norm() / v.norm().clamp_min(1e-30)) for u, v in zip(got, want)]
    moved = N * 52 + N * (52 + 24) + N * 24 + P * 24 + 2 * P * 12            # forward | per-sample backward | fold | the leaves' clones
    r["bytes_moved"] = moved
    r["share_of_hbm_peak"] = moved / (r["hip"]["median_ms"] * 1e-3) / (a.hbm_peak_gbs * 1e9)
    print(json.dumps({"projection_term": dict(r["verdict"], hip_ms=r["hip"]["median_ms"], torch_ms=r["torch"]["median_ms"],
                                              share_of_hbm_peak=r["share_of_hbm_peak"])}), flush=True)


def bench_trainers(a, res):
    from PIL import Image
    import numpy as np
    from oracle import reference_trainer as rt
    from sugar_amd import coarse_train, io as sio, sugar_patch
    from sugar_amd.coarse_model import CoarseModel
    from tests import ref_env
    work = tempfile.mkdtemp(prefix="coarse_density_bench_")
    try:
        data = rt.write_dataset(work, P=a.gaussians, n_cams=a.cameras, W=a.width, H=a.height)
        size = {"gaussians": a.gaussians, "cameras": a.cameras, "width": a.width, "height": a.height, "stop_at": a.stop_at}

        def run_native():
            cams, names = sio.cameras_from_json(os.path.join(data.checkpoint_path, "cameras.json"))
            images = []
            for name in names:
                with Image.open(os.path.join(data.scene_path, "images", name + ".png")) as im:
                    images.append(torch.from_numpy(np.asarray(im.convert("RGB"), dtype=np.uint8).astype(np.float32) / np.float32(255.0)))
            ply = os.path.join(data.checkpoint_path, "point_cloud", "iteration_7000", "point_cloud.ply")
            model = CoarseModel.from_gaussian_ply(ply, cams, device="cuda:0", seed=0)
            trainer = coarse_train.CoarseTrainer(model, cams, images, num_iterations=a.stop_at, n_samples_for_sdf_regularization=a.samples,
                                                 regulariser="density")
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
            res["trainers"]["coarse_trainer_density"] = native
            print(json.dumps({"coarse_trainer_density": {k: native[k] for k in ("it_per_s_before_9000", "it_per_s_after_9000",
                                                                                 "gaussians_after_pruning")}}), flush=True)
            del trainer, model, images
            torch.cuda.empty_cache()
            return native

        def run_reference():
            sm = ref_env.import_sugar_model()
            sugar_patch.install_regulariser(sm)
            try:
                ref = rt.run(data, os.path.join(work, "out"), stop_at=a.stop_at, patch_sugar=True, patch_losses=True, patch_optimizer=True,
                             patch_gathers=True, patch_densifier=True, trainer="coarse_density",
                             log_path=os.path.join(work, "reference_console.log"))
            finally:
                sugar_patch.uninstall_regulariser(sm)
            ref.pop("profile_table", None)
            ref.pop("log", None)
            res["trainers"]["reference_all_bindings"] = ref
            return ref

        res["trainers"] = {"size": size, "order": ["reference_all_bindings", "coarse_trainer_density"] if a.reference_first else
                           ["coarse_trainer_density", "reference_all_bindings"]}
        if a.reference_first:
            ref, native = run_reference(), run_native()
        else:
            native, ref = run_native(), run_reference()
        if native["it_per_s_after_9000"] and ref.get("it_per_s_after_9000"):
            res["trainers"]["speedup_after_9000"] = native["it_per_s_after_9000"] / ref["it_per_s_after_9000"]
        print(json.dumps({"reference_all_bindings": {k: ref.get(k) for k in ("it_per_s_before_9000", "it_per_s_after_9000",
                                                                               "gaussians_after_pruning")}}), flush=True)
    finally:
        shutil.rmtree(work, ignore_errors=True)


def parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1_000_000)
    ap.add_argument("--gaussians", type=int, default=2_000_000)
    ap.add_argument("--cameras", type=int, default=64)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--stop-at", type=int, default=9200)
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--hbm-peak-gbs", type=float, default=8000.0, help="the HBM peak the share is given against (MI355X: 8 TB/s)")
    ap.add_argument("--reference-first", action="store_true", help="run the reference trainer before CoarseTrainer (the other order of the pair)")
    ap.add_argument("--skip-term", action="store_true")
    ap.add_argument("--skip-trainers", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coarse_density.json"))
    return ap


def main(argv=None):
    a = parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this benchmark measures nothing without one")
    res = {"size": {"samples": a.samples, "gaussians": a.gaussians}, "runs": a.runs, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "ops": {}}

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    if not a.skip_term:
        bench_term(a, res)
        write()
    if not a.skip_trainers:
        bench_trainers(a, res)
    write()
    print(json.dumps({"projection_term": res["ops"].get("projection_term", {}).get("verdict"),
                      "speedup_after_9000": res.get("trainers", {}).get("speedup_after_9000")}))


if __name__ == "__main__":
    main()
