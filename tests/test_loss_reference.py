"""CPU tests of the float64 reference of the L1 + D-SSIM loss (oracle/loss_reference.py) over the case table of tests/loss_cases.py:
the analytic gradient against float64 autograd, |grad| <= grad_mag, and the conditions tests/test_gpu_loss_pixels.py relies on (the
yardsticks' normalised errors exist and are finite).  Run with -s for the yardstick distributions and the window distance."""
import numpy as np
import pytest
import torch

from oracle import loss_reference as lr
from tests import loss_cases as lc

SHAPES = [s for s, _ in lc.SHAPES]
ids = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s)


def test_the_case_table():
    assert len(set(SHAPES)) == len(SHAPES) == 16 and all(why for _, why in lc.SHAPES)
    assert sum(c * h * w for c, h, w in SHAPES) < 300_000
    w = lr.window_taps()
    assert w.dtype == torch.float32 and w.shape == (11,) and abs(float(w.double().sum()) - 1) < 1e-7 and torch.equal(w, w.flip(0))
    # the divisor: torch's float32 sum of the eleven values is their sum rounded once (what csrc/loss.hip's make_window() divides by)
    gauss = torch.Tensor([np.exp(-(x - 5) ** 2 / 4.5) for x in range(11)])
    assert float(gauss.sum()) == float(np.float32(gauss.double().sum())) == float(np.float32(3.7592328))
    assert torch.equal(w, gauss / gauss.sum())
    img, gt = lc.images((4, 57, 65), "impulse")
    assert img.sum() == 4 and img[0, 27, 31] == 1 and gt[3, 28, 32] == 0.7 and int((gt != 0).sum()) == 4
    img, gt = lc.images((3, 5, 7), "impulse")
    assert img[0, 4, 6] == 1 and gt[0, 4, 6] == 0.7
    img, gt = lc.images((3, 29, 33), "equal")
    assert torch.equal(img[..., :16], gt[..., :16]) and not (img[..., 16:] == gt[..., 16:]).any()
    img, gt = lc.images((3, 29, 33), "range")
    assert img.min() < -0.5 and img.max() > 1.5 and 0 <= gt.min() and gt.max() <= 1
    img, gt = lc.images((3, 29, 33), "flat")
    assert (img - 0.97).abs().max() <= 1.001e-3 and (gt - 0.95).abs().max() <= 1.001e-3


@pytest.mark.parametrize("family", lc.FAMILIES)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_analytic_gradient_against_float64_autograd(shape, family):
    img, gt = lc.images(shape, family)
    for lam in lc.LAMBDAS:
        for g in (1.0, -2.5):
            ref = lc.reference(shape, family, lam, g)["ref"]
            auto = lr.autograd_ref(img, gt, lc.f32(lam), g)
            top = np.abs(ref["grad"]).max()
            assert np.abs(ref["grad"] - auto).max() <= 1e-11 * top, (lam, g)
            assert np.isfinite(ref["grad"]).all() and np.isfinite(ref["grad_mag"]).all()
            assert (np.abs(ref["grad"]) <= ref["grad_mag"] * (1 + 1e-12)).all(), (lam, g)
            assert not ref["grad"][ref["grad_mag"] == 0].any(), (lam, g)
            assert abs(ref["loss"] - ((1 - lc.f32(lam)) * ref["l1_mean"] + lc.f32(lam) * (1 - ref["ssim_mean"]))) < 1e-15
    assert ref["l1_mean"] == float((img.double() - gt.double()).abs().mean())


def test_the_black_part_of_the_impulse_images_has_no_gradient():
    ref = lc.reference((3, 96, 128), "impulse", 0.2)["ref"]
    dark = ref["grad_mag"] == 0
    # (the means reach 5 pixels from an impulse, the windowed partials 5 more)
    assert not dark[:, 17:38, 21:42].any() and not dark[:, 18:39, 22:43].any()
    assert dark[:, :17].all() and dark[:, 39:].all() and dark[:, :, :21].all() and dark[:, :, 43:].all()
    assert dark.mean() > 0.95


@pytest.mark.parametrize("family", lc.FAMILIES)
def test_the_yardsticks_have_a_finite_distribution_on_every_case(family):
    """what the GPU test's bars are made of: for both yardsticks err = |yard - ref64| / grad_mag over the pixels with grad_mag > 0 is
    finite, exists unless the image has no such pixel, and the yardsticks are exactly 0 where grad_mag == 0 (asserted by pixel_err)"""
    for lam in lc.LAMBDAS[1:]:
        for g in (1.0, -2.5):
            worst = {}
            for shape in SHAPES:
                ref = lc.reference(shape, family, lam, g)["ref"]
                ea, eb = lc.yardstick_err(shape, family, lam, g)
                assert len(ea) == len(eb) == int((ref["grad_mag"] > 0).sum())
                assert len(ea) > 0 or not ref["grad_mag"].any()
                assert np.isfinite(ea).all() and np.isfinite(eb).all()
                if g == 1.0:
                    print(lc.describe(lc.label(shape, family, lam) + " yardstick (a) 2-D window, autograd", ea))
                    print(lc.describe(lc.label(shape, family, lam) + " yardstick (b) separable pairs    ", eb))
                y_max, y_med, _, _, pooled = lc.yardstick_bar(shape, family, lam, g)
                assert (y_max > 0 and y_med > 0) or not len(ea)
                assert pooled == (len(ea) < lc.MIN_PIXELS)
                for k, e in (("a", ea), ("b", eb)):
                    if len(e):
                        worst[k] = (max(worst.get(k, (0, 0))[0], e.max()), max(worst.get(k, (0, 0))[1], np.median(e)))
            print(f"{family} lam {lam:g} g {g:g}: over the shapes, (a) max {worst['a'][0]:.3e} largest median {worst['a'][1]:.3e}; "
                  f"(b) max {worst['b'][0]:.3e} largest median {worst['b'][1]:.3e}")
    le = lc.family_loss_err(family)
    print(f"{family}: largest |yardstick - ref64| of loss {le['loss']:.3e} l1_mean {le['l1_mean']:.3e} ssim_mean {le['ssim_mean']:.3e}")
    assert all(np.isfinite(v) for v in le.values())


# The distance between the two definitions of the window, both evaluated in float64: the reference's [11, 11] window is the outer
# product of the eleven taps ROUNDED to float32, the kernels (and l1_ssim_ref) apply the eleven taps twice.  Figures printed by this
# test when it was written (the largest over the shapes, lambda = 1): of the gradient in units of grad_mag, in units of max|grad|, and of
# the loss.  They can only change if someone changes the window; the test allows twice the recorded distance.
WINDOW_DISTANCE = {
    "noise": (1.655e-08, 3.678e-08, 3.392e-09),
    "flat": (7.981e-09, 1.456e-05, 5.934e-09),
    "equal": (5.297e-08, 5.822e-08, 1.006e-08),
    "range": (2.929e-08, 3.081e-08, 3.178e-09),
    "impulse": (4.464e-08, 6.641e-09, 6.324e-11),
}


@pytest.mark.parametrize("family", lc.FAMILIES)
def test_distance_between_the_separable_and_the_rounded_2d_window(family):
    worst = np.zeros(3)
    for shape in SHAPES:
        img, gt = lc.images(shape, family)
        sep = lc.reference(shape, family, 1.0)["ref"]
        two = lr.l1_ssim_ref(img, gt, 1.0, window="2d")
        diff = np.abs(two["grad"] - sep["grad"])
        live = sep["grad_mag"] > 0
        worst = np.maximum(worst, [(diff[live] / sep["grad_mag"][live]).max() if live.any() else 0.0,
                                   diff.max() / max(np.abs(sep["grad"]).max(), 1e-300), abs(two["loss"] - sep["loss"])])
        assert not diff[~live].any()
    print(f"{family}: 2-D rounded window against separable, float64: gradient {worst[0]:.3e} of grad_mag, {worst[1]:.3e} of max|grad|; "
          f"loss {worst[2]:.3e}")
    assert (worst <= 2 * np.asarray(WINDOW_DISTANCE[family])).all(), (worst, WINDOW_DISTANCE[family])
