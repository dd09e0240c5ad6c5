"""CPU tests of the sparse density-grid sweep (sugar_amd.extract.density_grid_sparse): the activation rule, restated in float64 by
tests/sparse_sweep_restatement.py, leaves no point that marching cubes reads outside the active bricks -- checked against a float64
density this file computes itself with scipy's k-d tree on the committed fixture -- and the argument checks that need no GPU."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sparse_sweep_restatement as ssr  # noqa: E402

FX = np.load(os.path.join(HERE, "golden", "sugar_mcgrid.npz"))
GRIDS = ssr.fixture_grids(FX)
LEVELS = (0.3, 0.05)
GAUSSIANS = (FX["points"], FX["inv_scaled_rot"], FX["strengths"])


@functools.lru_cache(maxsize=None)
def _density(grid):
    return ssr.density_float64(*GRIDS[grid], *GAUSSIANS)


def test_the_axes_of_the_test_grids_ascend():
    for name, axes in GRIDS.items():
        for a in axes:
            assert a.dtype == np.float32 and np.all(np.diff(a) > 0), name
    assert [a.size for a in GRIDS["box37x29x43"]] == [37, 29, 43]
    x, y, z = GRIDS["box37x29x43"]
    assert np.ptp(np.diff(x)) > 1e-3 and np.ptp(np.diff(y)) > 1e-3 and np.ptp(np.diff(z)) > 1e-3   # non-uniform


def test_the_float64_density_agrees_with_the_fixture():
    d = _density("fixture40")
    assert np.allclose(d, FX["density"], rtol=2e-3, atol=2e-5)


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("grid", list(GRIDS))
def test_rule_covers_every_needed_point(grid, level):
    """inflation 1.0, the bare rule: every inside point and each of its six neighbours lies in an active brick"""
    d = _density(grid)
    mask = ssr.brick_mask(*GRIDS[grid], *GAUSSIANS, level, inflation=1.0)
    assert mask.shape == tuple(ssr.n_bricks(n) for n in d.shape)
    active = ssr.point_mask(mask, d.shape)
    need = ssr.needed_points(d, level)
    assert need.any() and not (need & ~active).any()
    assert float(d[~active].max(initial=0.0)) < level
    assert not mask.all() or grid == "fixture40"


def test_active_bricks_of_the_wide_grid():
    """the rule as built (inflation 1.01) activates 11 of 125 bricks at level 0.3 and 13 at 0.05; the bare rule (inflation 1.0) one brick
    fewer at 0.3; the cap of the GPU test (16) holds for the restatement at inflation 1.02 too"""
    assert int(ssr.brick_mask(*GRIDS["wide40"], *GAUSSIANS, 0.3).sum()) == 11
    assert int(ssr.brick_mask(*GRIDS["wide40"], *GAUSSIANS, 0.05).sum()) == 13
    m100 = ssr.brick_mask(*GRIDS["wide40"], *GAUSSIANS, 0.3, inflation=1.0)
    m101 = ssr.brick_mask(*GRIDS["wide40"], *GAUSSIANS, 0.3)
    m102 = ssr.brick_mask(*GRIDS["wide40"], *GAUSSIANS, 0.3, inflation=1.02)
    assert int(m100.sum()) == 10
    assert m102.size == 125 and int(m102.sum()) <= 16
    assert not (m100 & ~m101).any() and not (m101 & ~m102).any()


def test_zero_inside_drops_only_bricks_wholly_inside():
    """on the 40^3 grid at +-3.6 a brick spans 7 x 0.185 = 1.29: none fits into the box (-0.5, 0.5), which therefore drops nothing; the box
    (-0.9, 0.9) -- the foreground box of a background pass over +-4 x 0.9 -- holds the central brick (points 16 .. 23, +-0.646)"""
    full = ssr.brick_mask(*GRIDS["wide40"], *GAUSSIANS, 0.3)
    assert np.array_equal(ssr.brick_mask(*GRIDS["wide40"], *GAUSSIANS, 0.3, zero_inside=(-0.5, 0.5)), full)
    cut = ssr.brick_mask(*GRIDS["wide40"], *GAUSSIANS, 0.3, zero_inside=(-0.9, 0.9))
    dropped = full & ~cut
    assert np.argwhere(dropped).tolist() == [[2, 2, 2]] and not (cut & ~full).any()
    x = GRIDS["wide40"][0]
    inside = (x > np.float32(-0.9)) & (x < np.float32(0.9))
    pts = ssr.point_mask(dropped, (40, 40, 40))
    assert (pts <= (inside[:, None, None] & inside[None, :, None] & inside[None, None, :])).all()


def _cpu_args():
    t = lambda k: torch.from_numpy(FX[k])
    return [t("X"), t("Y"), t("Z"), t("points"), t("inv_scaled_rot"), t("strengths")]


def test_cpu_tensors_raise():
    from sugar_amd.extract import density_grid_sparse, extract_mesh_marching_cubes
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        density_grid_sparse(*_cpu_args(), 0.3)
    P = 32
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        extract_mesh_marching_cubes(torch.zeros(P, 3), torch.ones(P, 3), torch.ones(P, 4), torch.ones(P), torch.zeros(P, 3), 1.0,
                                    resolution=16, sweep="sparse")


@pytest.mark.parametrize("level", [0.0, -0.3, float("inf"), float("nan")])
def test_bad_level_raises_before_any_library_call(level, monkeypatch):
    from sugar_amd import _lib
    from sugar_amd.extract import density_grid_sparse
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was loaded"))
    with pytest.raises(ValueError, match="level"):
        density_grid_sparse(*_cpu_args(), level)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_non_ascending_axis_raises_before_any_library_call(axis, monkeypatch):
    from sugar_amd import _lib
    from sugar_amd.extract import density_grid_sparse
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was loaded"))
    args = _cpu_args()
    a = args[axis].clone(); a[7] = a[6]                                     # a repeated point: ascending, but not strictly
    args[axis] = a
    with pytest.raises(ValueError, match="strictly ascending"):
        density_grid_sparse(*args, 0.3)
    args[axis] = torch.flip(args[axis], dims=[0])
    with pytest.raises(ValueError, match="strictly ascending"):
        density_grid_sparse(*args, 0.3)


def test_bad_sweep_raises_before_any_library_call(monkeypatch):
    from sugar_amd import _lib
    from sugar_amd.extract import extract_mesh_marching_cubes
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was loaded"))
    P = 32
    with pytest.raises(ValueError, match="sweep"):
        extract_mesh_marching_cubes(torch.zeros(P, 3), torch.ones(P, 3), torch.ones(P, 4), torch.ones(P), torch.zeros(P, 3), 1.0,
                                    resolution=16, sweep="brick")


def test_command_line_offers_the_sweep(capsys):
    from sugar_amd import extract
    with pytest.raises(SystemExit):
        extract.main(["cloud.ply", "--out", "mesh.ply", "--sweep", "brick"])
    assert "--sweep" in capsys.readouterr().err
