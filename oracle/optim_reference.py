"""float64 restatements of the optimiser side of the train step, element by element, with condition magnitudes, and two float32 CPU
yardsticks per operation (the convention of oracle/loss_reference.py):

    Adam                    sugar_amd/csrc/adam.hip          k_adam, k_adam_multi                 torch.optim.Adam, gaussian_model.py:152-166
    SH gradient over views  sugar_amd/csrc/sh_adam.hip       k_sh_grad_from_views, k_sh_adam_*    backward.cu:47-97 per view, summed
    activations             sugar_amd/csrc/activations.hip   k_activations_fwd / _bwd             gaussian_model.py:92-117

Inputs are the float32 arrays a kernel gets; every restatement computes in float64 from them.  A condition magnitude is the restated
expression with every term replaced by its absolute value: the scale a float32 evaluation can be held to, element by element
(err = |got - ref64| / magnitude, in units of which 2^-24 is one float32 rounding).

Yardsticks (neither is the code under test): (a) `*_f32`: numpy float32, every operation rounded once in the order the kernel writes
it, no contraction; (b) what the kernel replaces: torch.optim.Adam(foreach=False) on CPU float32, torch float32 ops with autograd for
the activations, the float32 run of the SH restatement."""
from __future__ import annotations

import math

import numpy as np
import torch

from oracle.torch_cpu_rasterizer import SH_C0, SH_C1, SH_C2, SH_C3

NORM_EPS = 1e-12   # F.normalize


def intended_double(x) -> float:
    """sgr_common.h::sgr_intended_double: the shortest decimal that rounds to the float32 `x` (0.999 from 0.999f), as a double"""
    x = np.float32(x)
    for digits in range(1, 10):
        d = float("%.*g" % (digits, float(x)))
        if np.float32(d) == x:
            return d
    return float(x)


# ---- Adam ----------------------------------------------------------------------------------------------------------------------
def segment_lr(n, segments):
    """-> float32 [n]: the learning rate of every element of a flat buffer under a segment table of (begin, end, lr_a, lr_b, period,
    split): lr_a where (e - begin) % period < split, lr_b elsewhere; 0 outside every segment; the last listed segment that holds an
    element wins (adam.hip::seg_of); a period <= 0 counts as 1 (sgr_adam_launch)"""
    lr = np.zeros(n, np.float32)
    for begin, end, lr_a, lr_b, period, split in segments:
        lo, hi = max(int(begin), 0), min(int(end), n)
        if hi <= lo:
            continue
        e = np.arange(lo, hi, dtype=np.int64)
        phase = (e - int(begin)) % (int(period) if period > 0 else 1)
        lr[lo:hi] = np.where(phase < split, np.float32(lr_a), np.float32(lr_b))
    return lr


def _coefficients(beta1, beta2, step):
    b1, b2 = intended_double(beta1), intended_double(beta2)
    return b1, b2, 1.0 - b1, 1.0 - b2, 1.0 - b1 ** step, math.sqrt(1.0 - b2 ** step)


def _gradient64(g, grad_scale, extra):
    g = np.array(g, np.float64)
    if extra is not None and len(extra):
        g.reshape(-1)[: len(extra)] += np.asarray(extra, np.float64).reshape(-1)
    return g * float(np.float32(grad_scale))


def adam_step(p, g, m, v, lr_per_element, beta1, beta2, eps, step, grad_scale=1.0, extra=None, g_mag=None):
    """One torch.optim.Adam step in float64: g' = (g + extra) * grad_scale (extra covers the first len(extra) elements),
    m' = b1 m + (1 - b1) g', v' = b2 v + (1 - b2) g'^2, delta = lr / (1 - b1^t) * m' / (sqrt(v') / sqrt(1 - b2^t) + eps), p' = p - delta,
    the betas as intended doubles, `1 - beta` and `1 - beta ** t` formed in double as torch forms them.

    -> (p', m', v', mags): mags = dict(m=|b1 m| + |(1 - b1) g'|, v=v', p=|p| + |delta|, delta=|delta|, p_cond=|p| + delta with m' replaced by
    its magnitude).

    g_mag: the gradient is itself a sum of float32 terms whose absolute values add up to g_mag (the SH gradient over views, consumed
    without being stored): a float32 evaluation is then off by a rounding of g_mag, not of |g|, so |g'| is replaced by g_mag in the
    magnitudes of m' and v', and delta's gains the size of its response: |d delta / d m'| (1 - b1) g_mag through the numerator and
    |d delta / d sqrt(v')| sqrt(1 - b2) g_mag through the denominator (sqrt(a + (1 - b2) g^2) moves by at most sqrt(1 - b2) |dg|)."""
    p, m, v = (np.asarray(a, np.float64) for a in (p, m, v))
    lr = np.asarray(lr_per_element, np.float64)
    b1, b2, omb1, omb2, bc1, bc2_sqrt = _coefficients(beta1, beta2, step)
    eps = float(np.float32(eps))
    gg = _gradient64(g, grad_scale, extra)
    m1 = b1 * m + omb1 * gg
    v1 = b2 * v + omb2 * gg * gg
    denom = np.sqrt(v1) / bc2_sqrt + eps
    delta = lr / bc1 * (m1 / denom)
    p1 = p - delta
    ga = np.abs(gg) if g_mag is None else np.asarray(g_mag, np.float64) * abs(float(np.float32(grad_scale)))
    mags = dict(m=np.abs(b1 * m) + omb1 * ga, v=b2 * v + omb2 * ga * ga, delta=np.abs(delta))
    if g_mag is not None:
        mags["delta"] = mags["delta"] + lr / bc1 * (omb1 * ga / denom + np.abs(m1) / denom ** 2 * math.sqrt(omb2) * ga / bc2_sqrt)
    mags["p"] = np.abs(p) + mags["delta"]
    # where b1 m and (1 - b1) g' cancel, |delta| is far below what a rounding of m' moves it by: the update with its numerator's two
    # terms made absolute is the scale on which delta is well conditioned
    mags["p_cond"] = np.abs(p) + np.maximum(mags["delta"], lr / bc1 * (mags["m"] / denom))
    return p1, m1, v1, mags


def adam_step_f32(p, g, m, v, lr_per_element, beta1, beta2, eps, step, grad_scale=1.0, extra=None):
    """yardstick (a): adam.hip's update in numpy float32, operation by operation in its written order, the coefficients rounded to
    float32 where sgr_adam_launch rounds them -> (p', m', v') float32"""
    f = np.float32
    p, g, m, v, lr = (np.asarray(a, f) for a in (p, g, m, v, lr_per_element))
    _, _, omb1, omb2, bc1, bc2_sqrt = (f(c) for c in _coefficients(beta1, beta2, step))
    b1, b2, eps = f(beta1), f(beta2), f(eps)
    gg = g.copy()
    with np.errstate(all="ignore"):
        if extra is not None and len(extra):
            gg.reshape(-1)[: len(extra)] += np.asarray(extra, f).reshape(-1)
        gg = gg * f(grad_scale)
        m1 = b1 * m + omb1 * gg
        v1 = b2 * v + omb2 * gg * gg
        denom = np.sqrt(v1) / bc2_sqrt + eps
        p1 = p - (lr / bc1) * (m1 / denom)
    assert p1.dtype == m1.dtype == v1.dtype == f
    return p1, m1, v1


def adam_step_torch(p, g, m, v, lr_per_element, beta1, beta2, eps, step, grad_scale=1.0, extra=None):
    """yardstick (b): torch.optim.Adam(foreach=False) on CPU float32, one parameter group per distinct learning rate (the update is
    elementwise: which tensor an element sits in changes nothing), its state set to (step - 1, m, v) -> (p', m', v') float32"""
    f = np.float32
    p, m, v, lr = (np.asarray(a, f).reshape(-1) for a in (p, m, v, lr_per_element))
    gg = np.array(g, f).reshape(-1)
    with np.errstate(all="ignore"):
        if extra is not None and len(extra):
            gg[: len(extra)] += np.asarray(extra, f).reshape(-1)
        gg = gg * f(grad_scale)
    out = [a.copy() for a in (p, m, v)]
    for rate in np.unique(lr):
        idx = np.flatnonzero(lr == rate)
        t = lambda a: torch.from_numpy(a[idx].copy())
        param = t(p).requires_grad_(True)
        param.grad = t(gg)
        opt = torch.optim.Adam([param], lr=float(rate), betas=(intended_double(beta1), intended_double(beta2)), eps=float(f(eps)),
                               foreach=False)
        opt.state[param] = dict(step=torch.tensor(float(step - 1)), exp_avg=t(m), exp_avg_sq=t(v))
        opt.step()
        st = opt.state[param]
        for dst, src in zip(out, (param.detach(), st["exp_avg"], st["exp_avg_sq"])):
            dst[idx] = src.numpy()
    return tuple(a.reshape(np.shape(g)) for a in out)


# ---- the SH gradient summed over views -----------------------------------------------------------------------------------------
def sh_basis(D, d):
    """the (D + 1)^2 basis values of the reference's eval_sh (forward.cu:20-69) at the unit directions d [P, 3] -> [P, (D + 1)^2]"""
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    b = [torch.full_like(x, SH_C0)]
    if D > 0:
        b += [-SH_C1 * y, SH_C1 * z, -SH_C1 * x]
    if D > 1:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        b += [SH_C2[0] * xy, SH_C2[1] * yz, SH_C2[2] * (2 * zz - xx - yy), SH_C2[3] * xz, SH_C2[4] * (xx - yy)]
    if D > 2:
        b += [SH_C3[0] * y * (3 * xx - yy), SH_C3[1] * xy * z, SH_C3[2] * y * (4 * zz - xx - yy),
              SH_C3[3] * z * (2 * zz - 3 * xx - 3 * yy), SH_C3[4] * x * (4 * zz - xx - yy), SH_C3[5] * z * (xx - yy),
              SH_C3[6] * x * (xx - 3 * yy)]
    return torch.stack(b, dim=1)


def sh_grad_from_views(means, campos, dcolor, D, M, dtype=torch.float64):
    """dL/dsh [P, M, 3] = sum over the views v of basis_k(normalize(mean - campos[v])) * dcolor[v, :, c] (the per-view SH backward,
    backward.cu:47-97, with the colour gradients already masked); coefficients k >= (D + 1)^2 get 0, and a view in which all three
    colour gradients of a Gaussian are exactly 0 is skipped for it.  means [P, 3], campos [V, 3], dcolor [V, P, 3], torch tensors.

    -> (grad, mag): mag = sum over the views of |basis_k| |dcolor_c|.  dtype=torch.float32 is the float32 yardstick (b)."""
    means, campos, dcolor = (torch.as_tensor(a).to(dtype) for a in (means, campos, dcolor))
    P = means.shape[0]
    grad, mag = torch.zeros(P, M, 3, dtype=dtype), torch.zeros(P, M, 3, dtype=dtype)
    for v in range(dcolor.shape[0]):
        live = (dcolor[v] != 0).any(dim=1)
        d = means[live] - campos[v][None]
        B = sh_basis(D, d / d.norm(dim=1, keepdim=True))
        term = B[:, :, None] * dcolor[v][live][:, None, :]
        grad[live, : B.shape[1]] += term
        mag[live, : B.shape[1]] += term.abs()
    return grad, mag


def sh_grad_from_views_f32(means, campos, dcolor, D, M):
    """yardstick (a): sh_adam.hip::sh_grad_sum_over_views in numpy float32, operation by operation in its written order -> [P, M, 3]"""
    f = np.float32
    means, campos, dcolor = (np.asarray(a, f) for a in (means, campos, dcolor))
    C1, C2, C3 = f(SH_C1), [f(c) for c in SH_C2], [f(c) for c in SH_C3]
    P = means.shape[0]
    acc = np.zeros((P, M, 3), f)
    for v in range(dcolor.shape[0]):
        live = (dcolor[v] != 0).any(axis=1)
        g = dcolor[v][live]
        dx, dy, dz = (means[live, i] - campos[v, i] for i in range(3))
        length = np.sqrt(dx * dx + dy * dy + dz * dz)
        x, y, z = dx / length, dy / length, dz / length
        b = [np.full_like(x, f(SH_C0))]
        if D > 0:
            b += [-C1 * y, C1 * z, -C1 * x]
        if D > 1:
            xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
            b += [C2[0] * xy, C2[1] * yz, C2[2] * (f(2) * zz - xx - yy), C2[3] * xz, C2[4] * (xx - yy)]
        if D > 2:
            b += [C3[0] * y * (f(3) * xx - yy), C3[1] * xy * z, C3[2] * y * (f(4) * zz - xx - yy),
                  C3[3] * z * (f(2) * zz - f(3) * xx - f(3) * yy), C3[4] * x * (f(4) * zz - xx - yy), C3[5] * z * (xx - yy),
                  C3[6] * x * (xx - f(3) * yy)]
        B = np.stack(b, axis=1)
        assert B.dtype == f
        acc[live, : B.shape[1]] += B[:, :, None] * g[:, None, :]
    return acc


def sh_colors(D, sh, means, campos):
    """eval_sh before its clamp (oracle/torch_cpu_rasterizer.py::eval_sh_unclamped, what test_sh_direction_elsewhere's reference
    evaluates) at normalize(mean - campos[v]) -> [V, P, 3]; differentiable in sh and in means"""
    from oracle.torch_cpu_rasterizer import eval_sh_unclamped
    out = []
    for v in range(campos.shape[0]):
        d = means - campos[v][None]
        out.append(eval_sh_unclamped(D, sh, d / d.norm(dim=1, keepdim=True)))
    return torch.stack(out)


def sh_direction_term(means, campos, dcolor, D, sh, dtype=torch.float64):
    """dL/dmean through the view direction, summed over the views: autograd of sum(dcolor * sh_colors) in the means -> [P, 3] numpy
    (dtype=torch.float32: its float32 yardstick)"""
    means, campos, dcolor, sh = (torch.as_tensor(a).to(dtype) for a in (means, campos, dcolor, sh))
    if D == 0:   # (the colour does not depend on the direction)
        return np.zeros(tuple(means.shape), np.float64 if dtype == torch.float64 else np.float32)
    means = means.clone().requires_grad_(True)
    (sh_colors(D, sh, means, campos) * dcolor).sum().backward()
    return means.grad.numpy()


# ---- activations ---------------------------------------------------------------------------------------------------------------
def activations_fwd(scaling_raw, rotation_raw, opacity_raw):
    """exp, v / max(|v|, 1e-12), sigmoid in float64 -> dict(scales [P, 3], rotations [P, 4], opacities [P, 1]) and `mags`, each result's
    own magnitude"""
    s, q, o = (np.asarray(a, np.float64) for a in (scaling_raw, rotation_raw, opacity_raw))
    with np.errstate(over="ignore"):
        out = dict(scales=np.exp(s), rotations=q / np.maximum(np.sqrt((q * q).sum(1, keepdims=True)), NORM_EPS),
                   opacities=1.0 / (1.0 + np.exp(-o)))
    return out, {k: np.abs(a) for k, a in out.items()}


def activations_bwd(scaling_raw, rotation_raw, opacity_raw, d_scales, d_rotations, d_opacities):
    """The gradients with respect to the raw parameters in float64: g exp(x); (g - n (n . g)) / |v| above the clamp of F.normalize and
    g / 1e-12 below it; g s (1 - s).  mags: |g_i| / |v| + |n_i| sum_j |n_j g_j| / |v| for the normalise, the result's own for the
    others"""
    s, q, o, gs, gq, go = (np.asarray(a, np.float64) for a in (scaling_raw, rotation_raw, opacity_raw, d_scales, d_rotations, d_opacities))
    norm = np.sqrt((q * q).sum(1, keepdims=True))
    above = norm > NORM_EPS
    safe = np.where(above, norm, 1.0)
    n = q / safe
    with np.errstate(over="ignore", invalid="ignore"):
        sig = 1.0 / (1.0 + np.exp(-o))
        out = dict(scaling=gs * np.exp(s), rotation=np.where(above, (gq - n * (n * gq).sum(1, keepdims=True)) / safe, gq / NORM_EPS),
                   opacity=go * sig * (1.0 - sig))
    mags = {k: np.abs(a) for k, a in out.items()}
    mags["rotation"] = np.where(above, (np.abs(gq) + np.abs(n) * np.abs(n * gq).sum(1, keepdims=True)) / safe, np.abs(gq) / NORM_EPS)
    return out, mags


def activations_f32(scaling_raw, rotation_raw, opacity_raw, d_scales=None, d_rotations=None, d_opacities=None):
    """yardstick (a): activations.hip in numpy float32, operation by operation in its written order -> (forward dict, backward dict or
    None)"""
    f = np.float32
    s, q, o = (np.asarray(a, f) for a in (scaling_raw, rotation_raw, opacity_raw))
    with np.errstate(all="ignore"):
        e = np.exp(s)
        qx, qy, qz, qw = (q[:, i:i + 1] for i in range(4))
        norm = np.sqrt(qx * qx + qy * qy + qz * qz + qw * qw)
        inv = f(1) / np.maximum(norm, f(NORM_EPS))
        sig = f(1) / (f(1) + np.exp(-o))
        fwd = dict(scales=e, rotations=q * inv, opacities=sig)
        if d_scales is None:
            return fwd, None
        gs, gq, go = (np.asarray(a, f) for a in (d_scales, d_rotations, d_opacities))
        above = norm > f(NORM_EPS)
        inv_n = f(1) / np.where(above, norm, f(1))
        n = q * inv_n
        dot = n[:, 0:1] * gq[:, 0:1] + n[:, 1:2] * gq[:, 1:2] + n[:, 2:3] * gq[:, 2:3] + n[:, 3:4] * gq[:, 3:4]
        bwd = dict(scaling=gs * e, rotation=np.where(above, (gq - n * dot) * inv_n, gq * f(1e12)), opacity=go * sig * (f(1) - sig))
    assert all(a.dtype == f for a in list(fwd.values()) + list(bwd.values()))
    return fwd, bwd


def activations_torch(scaling_raw, rotation_raw, opacity_raw, d_scales=None, d_rotations=None, d_opacities=None, dtype=torch.float32):
    """yardstick (b): torch.exp, F.normalize, torch.sigmoid and their autograd (gaussian_model.py:92-117) on the CPU -> (forward dict,
    backward dict or None) as numpy; dtype=torch.float64 is the autograd check of the restatement"""
    s, q, o = (torch.as_tensor(np.asarray(a)).to(dtype).requires_grad_(True) for a in (scaling_raw, rotation_raw, opacity_raw))
    outs = (torch.exp(s), torch.nn.functional.normalize(q), torch.sigmoid(o))
    fwd = {k: a.detach().numpy() for k, a in zip(("scales", "rotations", "opacities"), outs)}
    if d_scales is None:
        return fwd, None
    grads = tuple(torch.as_tensor(np.asarray(a)).to(dtype) for a in (d_scales, d_rotations, d_opacities))
    torch.autograd.backward(outs, grads)
    return fwd, dict(scaling=s.grad.numpy(), rotation=q.grad.numpy(), opacity=o.grad.numpy())
