"""`bench.py --dump-outputs DIR`: the writer of the timed step's outputs, on CPU tensors of the metric workload's sizes --
float32 / float64 files, 64 MB at most in all, and the same seeded sample of a large array from one run to the next."""
import os

import numpy as np
import torch


def _arrays(P=1_000_000, W=1920, H=1080):
    g = torch.Generator().manual_seed(0)
    return {"image": torch.rand(3, H, W, generator=g), "radii": torch.randint(0, 60, (P,), dtype=torch.int32, generator=g),
            "loss": torch.tensor([0.25]), "grad_xyz": torch.randn(P, 3, generator=g), "exp_avg_features": torch.randn(P, 16, 3, generator=g),
            "grad_opacity": torch.randn(P, 1, generator=g), "grad_scaling": torch.randn(P, 3, generator=g),
            "exp_avg_sq_rotation": torch.randn(P, 4, generator=g), "int_counts": torch.arange(1000, dtype=torch.int64)}


def test_dump_outputs_bounded_typed_and_repeatable(tmp_path):
    import bench
    arrays = _arrays()
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    bench.dump_outputs(str(tmp_path / "b"), arrays)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(k + ".npy" for k in arrays)
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= 64_000_000
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype in (np.float32, np.float64), n
        assert np.array_equal(a, b), n
    # small arrays are written whole and exactly; integers as float64
    assert np.array_equal(np.load(tmp_path / "a" / "loss.npy"), np.array([0.25], dtype=np.float32))
    lv = np.load(tmp_path / "a" / "int_counts.npy")
    assert lv.dtype == np.float64 and np.array_equal(lv, np.arange(1000))
    # a large array is cut to a sample of its own elements
    r = np.load(tmp_path / "a" / "radii.npy")
    assert r.dtype == np.float64 and 0 < r.size < arrays["radii"].numel()
    assert np.isin(r, arrays["radii"].numpy()).all()
