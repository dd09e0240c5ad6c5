"""GPU pins of the coarse loop's entropy term (sugar_amd.coarse_loss.opacity_entropy over csrc/coarse_loss.hip) against the trainer's
statement, sugar_trainers/coarse_sdf.py:543-551, written out below in torch and run on the CPU in float64 (the truth) and in float32
(the yard: what the unmodified trainer's arithmetic loses):

  * value and gradient at P in {1, 257, 70 000}: the scalar within max(4 x yard, 2 float32 ulp) relative, the gradient norm-wise
    within max(4 x yard, 1e-7) -- the bars of tests/test_gpu_coarse_loss.py;
  * opacities of exactly 0, 1, 0.5, 1e-12 and 1 - 2^-24: finite, and within the same bars;
  * invisible rows' gradient exactly zero; no visible row: NaN and an all-zero gradient; the same bits from run to run; [P,1] and [P]
    give the same bits; forward and backward make no host synchronisation.
Each check prints its distance, its bar and its ratio to the yard."""
import pytest
import torch

from sugar_amd import coarse_loss
from tests import coarse_loss_restatement as cl
from tests import sdf_regulariser_restatement as rs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR = 1e-7
TWO_ULP = 2.0 * 2.0 ** -23
UPSTREAM = 0.1                                                                   # the trainer's entropy_regularization_factor


def restated(opacities, visible, dtype):
    """coarse_sdf.py:545-551 on the CPU in `dtype`: (value, gradient w.r.t. the opacities) under the upstream factor"""
    o = opacities.to(dtype).clone().requires_grad_(True)
    vis_opacities = o[visible]                                                                               # :545
    value = (- vis_opacities * torch.log(vis_opacities + 1e-10)
             - (1 - vis_opacities) * torch.log(1 - vis_opacities + 1e-10)).mean()                            # :548-551
    (UPSTREAM * value).backward()
    return value.detach(), o.grad


def on_device(opacities, visible):
    o = opacities.to(DEV).clone().requires_grad_(True)
    value = coarse_loss.opacity_entropy(o, visible.to(DEV))
    assert value.dim() == 0 and value.device.type == "cuda" and value.dtype == torch.float32
    (UPSTREAM * value).backward()
    return value.detach(), o.grad


def _check(what, got, want, yard):
    got, want = torch.as_tensor(got).detach().cpu(), torch.as_tensor(want).detach().cpu()
    scalar = want.dim() == 0
    d = cl.scalar_distance(got, want) if scalar else rs.distance(got, want)
    bar = max(4.0 * float(yard), TWO_ULP if scalar else FLOOR)
    print(f"{what:40s} distance {d:.3e}   bar {bar:.3e}   yard {float(yard):.3e}   ratio-to-yard {d / max(float(yard), 1e-30):.2f}")
    assert torch.isfinite(got).all(), what
    assert d <= bar, (what, d, bar)


def _case(what, opacities, visible):
    want_v, want_g = restated(opacities, visible, torch.float64)
    f32_v, f32_g = restated(opacities, visible, torch.float32)
    got_v, got_g = on_device(opacities, visible)
    assert got_g.shape == opacities.shape
    _check(f"{what} value", got_v, want_v, cl.scalar_distance(f32_v, want_v))
    _check(f"{what} gradient", got_g, want_g, rs.distance(f32_g, want_g))
    assert not got_g.cpu()[~visible].any()                                       # invisible rows: exactly zero
    return got_v, got_g


@pytest.mark.parametrize("P", [1, 257, 70_000])
def test_value_and_gradient_match_the_float64_statement(P):
    g = torch.Generator().manual_seed(P)
    opacities = torch.sigmoid(3.0 * torch.randn(P, 1, generator=g))
    visible = torch.rand(P, generator=g) < 0.6
    visible[0] = True
    got = _case(f"P={P}", opacities, visible)
    again = on_device(opacities, visible)
    flat = on_device(opacities.reshape(-1), visible)
    assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1])       # the same bits from run to run
    assert torch.equal(got[0], flat[0]) and torch.equal(got[1].reshape(-1), flat[1])


def test_edge_opacities_are_finite_and_match():
    edges = torch.tensor([0.0, 1.0, 0.5, 1e-12, 1.0 - 2.0 ** -24]).reshape(-1, 1)
    assert float(edges[4]) < 1.0
    value, grad = _case("edges", edges, torch.ones(5, dtype=torch.bool))
    assert torch.isfinite(value) and torch.isfinite(grad).all()
    # each row on its own, so that none hides behind a larger one in the norm.  One row's float32 error is a single draw, not a yard,
    # so the bar comes from the format: the row's gradient is a sum of four terms, the largest of magnitude
    # m = max(|log(o + 1e-10)|, |log(1 - o + 1e-10)|, 1) times the upstream factor / 5; two accurate logf (<= 1 ulp each) and six
    # individually rounded operations (<= 1/2 ulp each, of values no larger than m) stay within 8 ulp of m.
    o = edges.double().reshape(-1)
    m = torch.maximum(torch.maximum(torch.log(o + 1e-10).abs(), torch.log(1 - o + 1e-10).abs()), torch.ones(5, dtype=torch.float64))
    want = restated(edges, torch.ones(5, dtype=torch.bool), torch.float64)[1].reshape(-1)
    err, bar = (grad.cpu().double().reshape(-1) - want).abs(), 8 * 2.0 ** -24 * (UPSTREAM / 5) * m
    for row in range(5):
        print(f"edge {float(edges[row]):.9g}: gradient {float(grad[row]):+.9e}   error {float(err[row]):.3e}   bar {float(bar[row]):.3e}")
    assert (err <= bar).all(), (err, bar)


def test_no_visible_row_gives_nan_and_a_zero_gradient():
    for P in (1, 257):
        opacities = torch.rand(P, 1, generator=torch.Generator().manual_seed(1))
        value, grad = on_device(opacities, torch.zeros(P, dtype=torch.bool))
        assert torch.isnan(value) and grad.shape == (P, 1) and not grad.any()
        assert torch.isnan(restated(opacities, torch.zeros(P, dtype=torch.bool), torch.float64)[0])


def test_argument_checks():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        coarse_loss.opacity_entropy(torch.rand(4, 1), torch.ones(4, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="bool"):
        coarse_loss.opacity_entropy(torch.rand(4, 1, device=DEV), torch.ones(4, device=DEV))
    with pytest.raises(RuntimeError, match="bool"):
        coarse_loss.opacity_entropy(torch.rand(5, 1, device=DEV), torch.ones(4, dtype=torch.bool, device=DEV))


def test_forward_and_backward_make_no_host_synchronisation():
    P = 70_000
    g = torch.Generator().manual_seed(5)
    opacities, visible = torch.rand(P, 1, generator=g).to(DEV), (torch.rand(P, generator=g) < 0.5).to(DEV)
    factor = torch.tensor(UPSTREAM, device=DEV)

    def both():
        o = opacities.clone().requires_grad_(True)
        (factor * coarse_loss.opacity_entropy(o, visible)).backward()
        return o.grad
    first = both(); torch.cuda.synchronize()                                     # (warm: code objects, the allocator)
    torch.cuda.set_sync_debug_mode("error")
    try:
        second = both()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(first, second) and second[visible].any()
