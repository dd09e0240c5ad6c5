"""The case table of the loss tests (tests/test_loss_reference.py on the CPU, tests/test_gpu_loss_pixels.py on the GPU): shapes,
image families, lambdas, and for every case the float64 reference (oracle/loss_reference.py) with the two float32 yardsticks, computed
once and shared (nobody writes into what `reference` returns)."""
import functools

import numpy as np
import torch

from oracle import loss_reference as lr

# (C, H, W): the smallest shapes that reach each structure of the kernels of csrc/loss.hip as they stand (forward tiles of 32 x 28,
# backward tiles of 32 x 32, 42 staged columns, tiles handed to the eight XCDs in eighths of the tile order)
SHAPES = [
    ((1, 1, 1), "loss[2] is the one pixel's S"),
    ((3, 5, 7), "smaller than the halo; planes of 35 floats: not 16-byte aligned"),
    ((1, 11, 11), "the window itself"),
    ((1, 6, 42), "the staged width of 42"),
    ((1, 7, 43), "one past the staged width"),
    ((1, 28, 32), "exactly one forward tile"),
    ((3, 29, 33), "one past a forward tile in each axis"),
    ((1, 27, 31), "one short of a forward tile in each axis"),
    ((1, 32, 32), "exactly one backward tile (two forward tile rows)"),
    ((1, 33, 32), "one row past the backward's tile height"),
    ((4, 57, 65), "forward 3 tile rows, backward 2; 36 forward tiles (no multiple of 8), 24 backward tiles"),
    ((3, 65, 43), "3 x 2 tiles in both kernels, the second tile column 11 wide; odd plane size"),
    ((1, 56, 128), "exactly 8 forward tiles"),
    ((3, 28, 96), "9 forward tiles: two per XCD slot, seven padding workgroups"),
    ((8, 28, 32), "one tile per XCD"),
    ((3, 96, 128), "the size of the trainer test"),
]
FAMILIES = ("noise", "flat", "equal", "range", "impulse")
LAMBDAS = (0.0, 0.2, 1.0)
GRAD_LOSSES = (None, 1.0, -2.5)   # NULL, a device scalar 1.0, -2.5
MIN_PIXELS = 64                   # below this a case has no distribution of its own: its yardstick is the family's at all shapes


def f32(v):
    """the value a float argument has after the C ABI (lambda = 0.2 is no float32)"""
    return float(np.float32(v))


@functools.lru_cache(maxsize=None)
def images(shape, family):
    """-> (image, target): float32 CPU tensors [C, H, W], seeded by shape and family"""
    C, H, W = shape
    g = torch.Generator().manual_seed(100003 * FAMILIES.index(family) + 7919 * C + 131 * H + W)
    rand = lambda: torch.rand(*shape, generator=g)
    if family == "noise":       # (as tests/test_gpu_loss.py)
        img = rand()
        gt = (img + 0.2 * torch.randn(*shape, generator=g)).clamp(0, 1)
    elif family == "flat":      # a converged render over sky or a wall: bright, nearly constant
        img = 0.97 + 1e-3 * (2 * rand() - 1)
        gt = 0.95 + 1e-3 * (2 * rand() - 1)
    elif family == "equal":     # left half: target == image (sign 0, S = 1); right half: independent noise
        img, gt = rand(), rand()
        gt[..., : W // 2] = img[..., : W // 2]
    elif family == "range":     # a render outside [0, 1], negatives included
        img = 0.3 + 0.8 * torch.randn(*shape, generator=g)
        gt = rand()
    elif family == "impulse":   # one pixel each, a row and a column apart, on the first tile seam of both kernels
        img, gt = torch.zeros(shape), torch.zeros(shape)
        img[:, min(27, H - 1), min(31, W - 1)] = 1.0
        gt[:, min(28, H - 1), min(32, W - 1)] = 0.7
    else:
        raise KeyError(family)
    return img.contiguous(), gt.contiguous()


@functools.lru_cache(maxsize=None)
def reference(shape, family, lam, grad_loss=1.0):
    """-> dict(ref=l1_ssim_ref, a=yardstick_autograd, b=yardstick_separable) at lambda = float32(lam)"""
    img, gt = images(shape, family)
    lam = f32(lam)
    return dict(ref=lr.l1_ssim_ref(img, gt, lam, grad_loss), a=lr.yardstick_autograd(img, gt, lam, grad_loss),
                b=lr.yardstick_separable(img, gt, lam, grad_loss))


def pixel_err(got, ref):
    """err = |got - ref64| / grad_mag over the pixels with grad_mag > 0 (flat array); where grad_mag == 0 the value must be 0 (as a
    value: its sign is free)"""
    got = np.asarray(got, np.float64)
    mag = ref["grad_mag"]
    live = mag > 0
    assert not got[~live].any(), ("pixels whose gradient is exactly zero must be exactly zero", np.argwhere(~live & (got != 0))[:8])
    return np.abs(got - ref["grad"])[live] / mag[live]


@functools.lru_cache(maxsize=None)
def yardstick_err(shape, family, lam, grad_loss=1.0):
    """-> (pixel errors of yardstick (a), of yardstick (b))"""
    r = reference(shape, family, lam, grad_loss)
    return pixel_err(r["a"]["grad"], r["ref"]), pixel_err(r["b"]["grad"], r["ref"])


@functools.lru_cache(maxsize=None)
def pooled_yardstick_err(family, lam, grad_loss=1.0):
    """the family at all shapes"""
    errs = [yardstick_err(shape, family, lam, grad_loss) for shape, _ in SHAPES]
    return np.concatenate([e[0] for e in errs]), np.concatenate([e[1] for e in errs])


def yardstick_bar(shape, family, lam, grad_loss=1.0):
    """Y = the larger of the two yardsticks -> (Y's worst pixel, Y's median, the two error arrays, pooled or not)"""
    ea, eb = yardstick_err(shape, family, lam, grad_loss)
    pooled = len(ea) < MIN_PIXELS
    if pooled:
        ea, eb = pooled_yardstick_err(family, lam, grad_loss)
    if not len(ea):
        return 0.0, 0.0, ea, eb, pooled
    return max(ea.max(), eb.max()), max(np.median(ea), np.median(eb)), ea, eb, pooled


@functools.lru_cache(maxsize=None)
def family_loss_err(family):
    """the largest |yardstick - ref64| of loss, l1_mean, ssim_mean over the family: all shapes, lambda 0.2 and 1, both yardsticks"""
    worst = dict(loss=0.0, l1_mean=0.0, ssim_mean=0.0)
    for shape, _ in SHAPES:
        for lam in LAMBDAS[1:]:
            r = reference(shape, family, lam)
            for k in worst:
                worst[k] = max(worst[k], abs(r["a"][k] - r["ref"][k]), abs(r["b"][k] - r["ref"][k]))
    return worst


def describe(name, err):
    if not len(err):
        return f"{name}: no pixels"
    return f"{name}: pixels {len(err)} max {err.max():.3e} median {np.median(err):.3e} p99 {np.quantile(err, 0.99):.3e}"


def label(shape, family, lam, grad_loss=1.0):
    s = "x".join(str(v) for v in shape) + f"-{family}-lam{lam:g}"
    return s if grad_loss == 1.0 else s + f"-g{grad_loss:g}"
