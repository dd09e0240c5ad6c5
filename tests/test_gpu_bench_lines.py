"""`bench.py` on a small scene: a plain run prints the headline and nothing that needs a run of its own; `--full` goes on
behind the timed region and adds the per-stage times, the rooflines, the CPU baseline and the legs' figures."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--gaussians", "20000", "--steps", "3", "--warmup", "1", "--preroll", "8"]
CONTRACT = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("stages_ms", "ms_fwd_bwd", "roofline", "cpu_baseline", "densify_stats_variant", "fast_alpha_variant", "after_training",
             "many_cameras_shuffled", "ms_fwd_bwd_api", "list_write_pass")


def _line(args, timeout):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout.decode()[-3000:]
    return json.loads(lines[0])


def _check_headline(d):
    for k in CONTRACT:
        assert k in d, k
    assert d["metric"] == "train_step_images_per_sec" and d["unit"] == "images/s" and d["dtype"] == "f32"
    assert d["higher_is_better"] is True and d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["ms_per_step"] > 0 and d["value"] == pytest.approx(1e3 / d["ms_per_step"], rel=1e-9)
    assert "forwards_repeated" in d and "host_enqueue_ms_per_step" in d


@pytest.mark.gpu
def test_plain_run_prints_the_headline_only():
    d = _line(SMALL, timeout=300)
    _check_headline(d)
    assert not [k for k in FULL_ONLY if k in d]
    assert "instances_per_view" not in d["config"]


@pytest.mark.gpu
def test_full_run_adds_the_other_measurements():
    d = _line(SMALL + ["--full", "--drift-steps", "4", "--cameras", "4", "--reference-loop-steps", "2", "--no-eight-thread-baseline"],
              timeout=900)
    _check_headline(d)
    assert not [k for k in FULL_ONLY if k not in d]
    assert d["roofline"]["launch_ms"] > 0 and d["config"]["instances_per_view"] > 0
    assert d["cpu_baseline"]["value"] > 0 and "eight_threads" not in d["cpu_baseline"]
    assert d["after_training"]["untimed_steps_before"] == 4 and d["many_cameras_shuffled"]["cameras"] == 4
