"""float64 reference of the fused L1 + D-SSIM loss (sugar_amd/csrc/loss.hip), per pixel, and two float32 yardsticks on the CPU.

    loss = (1 - lambda) * mean|x - y| + lambda * (1 - mean SSIM(x, y))        sugar_utils/loss_utils.py:17-63

The operation restated here is the one the kernels state: zero padding of 5 (conv2d(padding=5)), the eleven FLOAT32 values of
gaussian(11, 1.5) / sum taken exactly as they are, and the window applied SEPARABLY, along the rows and then along the columns.  The
reference's own window is the outer product of those eleven values rounded to float32 (create_window: `_1D.mm(_1D.t()).float()`); in
float64 the two definitions are a different operation by a few float32 roundings of the window, `window="2d"` evaluates that one
(tests/test_loss_reference.py keeps the distance on record).

    mu1 = G*x, mu2 = G*y, E2 = G*(x^2 + y^2), E12 = G*(xy)
    A = 2 mu1 mu2 + C1, B = 2 (E12 - mu1 mu2) + C2, C = mu1^2 + mu2^2 + C1, D = E2 - mu1^2 - mu2^2 + C2,  S = A B / (C D)
    dS/dE[x^2] = -S / D,   dS/dE[xy] = 2 A / (C D),   dS/dmu1 = 2 mu2 (B - A) / (C D)  -  2 mu1 S (D - C) / (C D)
    grad = g / N * ( (1 - lambda) sign(x - y) - lambda ( G*dS/dmu1 + 2 x G*dS/dE[x^2] + y G*dS/dE[xy] ) )      (G is symmetric)

`grad_mag` is the same expression with every term replaced by its absolute value, down to the two terms of dS/dmu1 (the convention of
oracle/sugar_field_torch.py's `*_mag`): the scale a float32 evaluation of the gradient can be held to, pixel by pixel.

Yardsticks (neither is the code under test): (a) `yardstick_autograd`: the reference's formulation in float32 through autograd
(sugar_amd.train_step.photometric_loss: 2-D window, five convolutions); (b) `yardstick_separable`: the separable pair formulation
({x, y}, {x^2 + y^2, xy}) and the analytic gradient evaluated in float32 with true division."""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

C1, C2 = 0.01 ** 2, 0.03 ** 2
HALF = 5


def window_taps() -> torch.Tensor:
    """the eleven float32 values of loss_utils.py:23-25"""
    gauss = torch.Tensor([math.exp(-(x - HALF) ** 2 / float(2 * 1.5 ** 2)) for x in range(2 * HALF + 1)])
    return gauss / gauss.sum()


def window_2d() -> torch.Tensor:
    """create_window's [11, 11] float32 window (loss_utils.py:28-32)"""
    w = window_taps().unsqueeze(1)
    return w.mm(w.t()).float()


def _separable(w):
    n = len(w)

    def conv(a):
        H, W = a.shape[-2:]
        p = F.pad(a, (HALF, HALF, HALF, HALF))
        rows = sum(w[k] * p[..., :, k:k + W] for k in range(n))     # along each row
        return sum(w[k] * rows[..., k:k + H, :] for k in range(n))  # down each column
    return conv


def _full_window(w2):
    def conv(a):
        ch = a.shape[0]
        return F.conv2d(a[None], w2.expand(ch, 1, *w2.shape).contiguous(), padding=HALF, groups=ch)[0]
    return conv


def _ssim_terms(x, y, conv):
    mu1, mu2 = conv(x), conv(y)
    e2, e12 = conv(x * x + y * y), conv(x * y)
    m11, m22, m12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    a = 2 * m12 + C1
    b = 2 * (e12 - m12) + C2
    c = m11 + m22 + C1
    d = (e2 - m11 - m22) + C2
    return mu1, mu2, a, b, c, d, a * b / (c * d)


def forward(x, y, lam, conv):
    """(loss, l1 mean, ssim mean) as tensors of x's type; differentiable"""
    s = _ssim_terms(x, y, conv)[-1]
    l1, ssim = (x - y).abs().mean(), s.mean()
    return (1.0 - lam) * l1 + lam * (1.0 - ssim), l1, ssim


def _evaluate(x, y, lam, g, conv, with_mag):
    n = x.numel()
    mu1, mu2, a, b, c, d, s = _ssim_terms(x, y, conv)
    cd = c * d
    t1, t2 = 2 * mu2 * (b - a) / cd, 2 * mu1 * s * (d - c) / cd
    ds1, ds12 = -s / d, 2 * a / cd
    sgn = torch.sign(x - y)
    l1, ssim = (x - y).abs().mean(), s.mean()
    out = dict(loss=(1.0 - lam) * l1 + lam * (1.0 - ssim), l1_mean=l1, ssim_mean=ssim,
               grad=(g / n) * ((1.0 - lam) * sgn - lam * (conv(t1 - t2) + 2 * x * conv(ds1) + y * conv(ds12))))
    if with_mag:
        out["grad_mag"] = (abs(g) / n) * ((1.0 - lam) * sgn.abs() + lam * (conv(t1.abs() + t2.abs()) + 2 * x.abs() * conv(ds1.abs())
                                                                       + y.abs() * conv(ds12.abs())))
    return out


def _numpy(out):
    return {k: (v.detach().numpy().astype(np.float64) if v.dim() else float(v.detach())) for k, v in out.items()}


def _inputs(img, gt):
    assert img.dtype == torch.float32 and gt.dtype == torch.float32 and img.shape == gt.shape and img.dim() == 3
    return img.detach().cpu(), gt.detach().cpu()


def l1_ssim_ref(img, gt, lam, grad_loss=1.0, window="separable"):
    """float32 images [C, H, W], evaluated in float64 -> dict(loss, l1_mean, ssim_mean: floats; grad, grad_mag: float64 [C, H, W])"""
    img, gt = _inputs(img, gt)
    conv = _separable(window_taps().double()) if window == "separable" else _full_window(window_2d().double())
    with torch.no_grad():
        return _numpy(_evaluate(img.double(), gt.double(), float(lam), float(grad_loss), conv, True))


def autograd_ref(img, gt, lam, grad_loss=1.0):
    """float64 autograd through a float64 forward of the same separable formulation (the check of the analytic gradient)"""
    img, gt = _inputs(img, gt)
    x = img.double().requires_grad_(True)
    loss = forward(x, gt.double(), float(lam), _separable(window_taps().double()))[0]
    (float(grad_loss) * loss).backward()
    return x.grad.numpy()


def yardstick_autograd(img, gt, lam, grad_loss=1.0):
    """(a) the reference's formulation in float32: 2-D window, five convolutions, autograd"""
    from sugar_amd.train_step import l1_loss, ssim
    img, gt = _inputs(img, gt)
    x = img.clone().requires_grad_(True)
    l1, s = l1_loss(x, gt), ssim(x, gt)
    loss = (1.0 - lam) * l1 + lam * (1.0 - s)
    (float(grad_loss) * loss).backward()
    return _numpy(dict(loss=loss, l1_mean=l1, ssim_mean=s, grad=x.grad))


def yardstick_separable(img, gt, lam, grad_loss=1.0):
    """(b) the separable pair formulation and the analytic gradient, every operation in float32, true division"""
    img, gt = _inputs(img, gt)
    with torch.no_grad():
        return _numpy(_evaluate(img, gt, float(lam), float(grad_loss), _separable(window_taps()), False))
