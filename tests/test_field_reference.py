"""The chunked float64 restatement of the density field and level-set sampler (oracle/sugar_field_torch.py), which the GPU tests
use as their reference at trainer scale, checked on the CPU against the unchunked restatement and float64 autograd."""
import pytest
import torch

from oracle import sugar_field_torch as ref


def _case(N=700, P=90, K=8, seed=3):
    g = torch.Generator().manual_seed(seed)
    centers = torch.randn(P, 3, generator=g, dtype=torch.float64)
    B = torch.randn(P, 3, 3, generator=g, dtype=torch.float64) * 1.5
    strengths = torch.rand(P, 1, generator=g, dtype=torch.float64)
    strengths[::11] = 0.
    nb = torch.randint(0, P, (N, K), generator=g)
    nb[nb >= P - 5] = 0                                          # five Gaussians nobody references
    nb[5, 1] = nb[5, 0]                                          # a neighbour twice in a row
    x = centers[nb[:, 0]] + 0.6 * torch.randn(N, 3, generator=g, dtype=torch.float64)
    x[7] = centers[nb[7, 0]]                                     # q = 0
    x[9] = 1e5                                                   # q > 1e8: opacity 0
    return g, x, nb, centers, B, strengths


@pytest.mark.parametrize("factor", [1.0, 1.3])
def test_chunked_density_field_equals_the_restatement_and_autograd(factor):
    g, x, nb, centers, B, strengths = _case()
    N, K = nb.shape
    go = torch.randn(N, K, generator=g, dtype=torch.float64); gd = torch.randn(N, generator=g, dtype=torch.float64)
    xr, cr, Br, sr = (t.clone().requires_grad_(True) for t in (x, centers, B, strengths))
    o, d = ref.density_field(xr, nb, cr, Br, sr, factor)
    ((o * go).sum() + (d * gd).sum()).backward()
    whole = ref.density_field_chunked(x, nb, centers, B, strengths, factor, go, gd)
    for chunk in (K * 37, 1 << 30):
        r = ref.density_field_chunked(x, nb, centers, B, strengths, factor, go, gd, chunk=chunk)
        close = lambda a, b: float((a - b).abs().max()) <= 1e-12 * max(1., float(b.abs().max()))
        assert close(r["opacities"], o.detach()) and close(r["densities"], d.detach())
        assert close(r["dx"], xr.grad) and close(r["dcenters"], cr.grad)
        assert close(r["dB"], Br.grad) and close(r["dstrengths"], sr.grad[:, 0])
        for k in ("opacities", "densities", "dx", "dcenters", "dB", "dstrengths"):
            assert close(r[k], whole[k]) and close(r[k + "_mag"], whole[k + "_mag"]), k
            assert bool((r[k].abs() <= r[k + "_mag"]).all()), k
    # one gradient at a time (the C ABI's optional pointers)
    only_o = ref.density_field_chunked(x, nb, centers, B, strengths, factor, go, None)
    only_d = ref.density_field_chunked(x, nb, centers, B, strengths, factor, None, gd)
    for k in ("dx", "dcenters", "dB", "dstrengths"):
        assert torch.allclose(only_o[k] + only_d[k], whole[k], rtol=1e-12, atol=1e-12)
    # the edges the GPU tests rely on: exactly zero for q > 1e8, strength 0 and unreferenced Gaussians
    assert float(whole["opacities"][9].abs().max()) == 0. and float(whole["dx"][9].abs().max()) == 0.
    unused = torch.ones(centers.shape[0], dtype=torch.bool); unused[nb.reshape(-1)] = False
    assert float(whole["dB"][unused].abs().sum()) == 0. and int(unused.sum()) > 0


def test_chunked_density_field_with_no_samples():
    _, _, _, centers, B, strengths = _case()
    r = ref.density_field_chunked(torch.zeros(0, 3, dtype=torch.float64), torch.zeros(0, 16, dtype=torch.int64), centers, B,
                                  strengths, 1.0, torch.zeros(0, 16, dtype=torch.float64), torch.zeros(0, dtype=torch.float64))
    assert r["densities"].shape == (0,) and r["opacities"].shape == (0, 16)
    assert float(r["dcenters"].abs().max()) == 0. and r["dB"].shape == (centers.shape[0], 3, 3)


@pytest.mark.parametrize("n_range,factor,range_size", [(21, 1.0, 3.0), (32, 1.7, 0.25), (2, 1.0, 3.0)])
def test_chunked_level_set_equals_the_restatement(n_range, factor, range_size):
    g, x, nb, centers, B, strengths = _case(N=500, K=6, seed=8)
    strengths = strengths * 2.5
    cam = torch.tensor([4.0, -1.0, 2.0], dtype=torch.float64)
    gstd = 0.3 + torch.rand(centers.shape[0], generator=g, dtype=torch.float64)
    world = centers[nb[:, 0]] + 0.2 * torch.randn(500, 3, generator=g, dtype=torch.float64)
    levels = (0.1, 0.3, 0.5)
    r0 = ref.level_set_points(world, nb, cam, centers, B, strengths, gstd, levels, n_range, range_size, factor)
    whole = ref.level_set_points_chunked(world, nb, cam, centers, B, strengths, gstd, levels, n_range, range_size, factor)
    r = ref.level_set_points_chunked(world, nb, cam, centers, B, strengths, gstd, levels, n_range, range_size, factor,
                                     chunk=6 * n_range * 29)
    assert torch.equal(r["densities"], whole["densities"]) or float((r["densities"] - whole["densities"]).abs().max()) < 1e-12
    assert bool((r["densities"].abs() <= r["densities_mag"] + 1e-12).all())
    n_valid = 0
    for L in levels:
        a, b = r["levels"][L], r0[L]
        assert torch.equal(a["valid"], b["valid"]) and torch.equal(a["valid"], whole["levels"][L]["valid"])
        v = a["valid"]
        n_valid += int(v.sum())
        assert float((a["points"][v] - b["intersection_points"]).abs().sum()) < 1e-12
        assert float((a["normals"][v] - b["normals"]).abs().sum()) < 1e-12
        assert bool((a["grad"].abs() <= a["grad_mag"]).all())
        # the crossing the reference picked: first sample above, the one before it not
        f = a["first"][v]
        d = r["densities"][v]
        assert bool((d.gather(1, f[:, None])[:, 0] > L).all()) and bool((d.gather(1, f[:, None] - 1)[:, 0] <= L).all())
    assert n_valid > 20
