"""Pure-PyTorch, autograd-differentiable CPU restatement of the rasterizer -- TEST INFRASTRUCTURE.

Independent check of the hand-derived backward (DGR/cuda_rasterizer/backward.cu) and the "PyTorch-CPU
autograd rasterize" numerics reference of BASELINE config 1.  The discrete parts (tile lists, their
depth order) are taken from the C oracle (oracle/cpu_rasterizer.c); everything differentiable is
recomputed here from the raw inputs with torch ops, so autograd yields d(image)/d(inputs) without
using any of the reference's analytic gradient formulas.

Reference semantics reproduced on purpose (they are not "mathematically clean", but they are what
DGR computes -- SURVEY.md appendix A.5/A.6):
  * no gradient through the power>0 / alpha<1/255 / T<1e-4 tests (piecewise constant);
  * min(0.99, .) is straight-through in the backward (backward.cu:499-554 applies the unclamped formula);
  * when t.x/t.z is clamped to 1.3*tanfov the clamped value is treated as a constant
    (x_grad_mul, backward.cu:175-176,262-264);
  * means2D gradient is reported in NDC-scaled units (x 0.5*W, 0.5*H; backward.cu:460-461,545-546).
"""
from __future__ import annotations

import torch

SH_C0 = 0.28209479177387814
SH_C1 = 0.4886025119029199
SH_C2 = [1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396]
SH_C3 = [-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154,
         -0.4570457994644658, 1.445305721320277, -0.5900435899266435]


def eval_sh_unclamped(deg, shs, dirs):
    """DGR/cuda_rasterizer/forward.cu:20-69: the colour + 0.5 BEFORE its clamp at 0; shs [P,M,3], dirs [P,3] normalised."""
    x, y, z = dirs[:, 0:1], dirs[:, 1:2], dirs[:, 2:3]
    r = SH_C0 * shs[:, 0]
    if deg > 0:
        r = r - SH_C1 * y * shs[:, 1] + SH_C1 * z * shs[:, 2] - SH_C1 * x * shs[:, 3]
        if deg > 1:
            xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
            r = (r + SH_C2[0] * xy * shs[:, 4] + SH_C2[1] * yz * shs[:, 5] + SH_C2[2] * (2 * zz - xx - yy) * shs[:, 6]
                 + SH_C2[3] * xz * shs[:, 7] + SH_C2[4] * (xx - yy) * shs[:, 8])
            if deg > 2:
                r = (r + SH_C3[0] * y * (3 * xx - yy) * shs[:, 9] + SH_C3[1] * xy * z * shs[:, 10]
                     + SH_C3[2] * y * (4 * zz - xx - yy) * shs[:, 11] + SH_C3[3] * z * (2 * zz - 3 * xx - 3 * yy) * shs[:, 12]
                     + SH_C3[4] * x * (4 * zz - xx - yy) * shs[:, 13] + SH_C3[5] * z * (xx - yy) * shs[:, 14]
                     + SH_C3[6] * x * (xx - 3 * yy) * shs[:, 15])
    return r + 0.5


def eval_sh_color(deg, shs, dirs):
    """DGR/cuda_rasterizer/forward.cu:20-71; shs [P,M,3], dirs [P,3] normalised."""
    return torch.clamp_min(eval_sh_unclamped(deg, shs, dirs), 0.0)


def quat_to_rotmat(q):
    """Standard rotation matrix of a (real-first, un-normalised as given) quaternion; forward.cu:127-138."""
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = torch.stack([
        1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
        2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
        2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)
    return R


def cov3d_from_scale_rot(scales, mod, rots):
    R = quat_to_rotmat(rots)
    S = (mod * scales)
    RS = R * S[:, None, :]
    return RS @ RS.transpose(1, 2)  # R S^2 R^T


def unpack_cov6(c6):
    P = c6.shape[0]
    S = c6.new_zeros(P, 3, 3)
    S[:, 0, 0] = c6[:, 0]; S[:, 0, 1] = c6[:, 1]; S[:, 0, 2] = c6[:, 2]
    S[:, 1, 0] = c6[:, 1]; S[:, 1, 1] = c6[:, 3]; S[:, 1, 2] = c6[:, 4]
    S[:, 2, 0] = c6[:, 2]; S[:, 2, 1] = c6[:, 4]; S[:, 2, 2] = c6[:, 5]
    return S


def preprocess(means3D, *, shs=None, colors_precomp=None, scales=None, rotations=None, cov3D_precomp=None, viewmatrix,
               projmatrix, campos, W, H, tanfovx, tanfovy, sh_degree=3, scale_modifier=1.0, clamp_as_constant=True,
               detach_direction=False):
    """The differentiable per-Gaussian part (forward.cu preprocessCUDA): projection, J, cov2D + 0.3, conic, SH colour.
    -> dict: p_proj [P,3], cov2 (a, b, c) [P,3], det [P], conic [P,3], color_unclamped [P,3] (None with colors_precomp), color [P,3].
    clamp_as_constant=False lets the gradient pass to t.x / t.y as if they had not been clamped (x_grad_mul = y_grad_mul = 1 in
    backward.cu's terms): NOT what the reference computes, kept so that a test can show its scene tells the two apart.
    detach_direction: the view direction is a constant of the colour (SGR_MODE_SH_DIR_ELSEWHERE's dL_dmean3D)."""
    dt = means3D.dtype
    V = viewmatrix.to(dt); PM = projmatrix.to(dt); campos = campos.to(dt)
    P = means3D.shape[0]
    ones = torch.ones(P, 1, dtype=dt)
    hom = torch.cat([means3D, ones], dim=1)
    p_view = hom @ V[:, :3]
    p_hom = hom @ PM
    p_w = 1.0 / (p_hom[:, 3:4] + 0.0000001)
    p_proj = p_hom[:, :3] * p_w

    Sigma = unpack_cov6(cov3D_precomp) if cov3D_precomp is not None else cov3d_from_scale_rot(scales, scale_modifier, rotations)
    fx = W / (2.0 * tanfovx); fy = H / (2.0 * tanfovy)
    tz = p_view[:, 2]
    limx, limy = 1.3 * tanfovx, 1.3 * tanfovy
    txtz, tytz = p_view[:, 0] / tz, p_view[:, 1] / tz
    in_x = (txtz >= -limx) & (txtz <= limx)
    in_y = (tytz >= -limy) & (tytz <= limy)
    tx = torch.where(in_x, p_view[:, 0], (txtz.clamp(-limx, limx) * tz).detach())
    ty = torch.where(in_y, p_view[:, 1], (tytz.clamp(-limy, limy) * tz).detach())
    if not clamp_as_constant:  # the clamped value, the gradient of the unclamped one (x_grad_mul = y_grad_mul = 1)
        tx, ty = p_view[:, 0] + (tx - p_view[:, 0]).detach(), p_view[:, 1] + (ty - p_view[:, 1]).detach()
    zero = torch.zeros_like(tz)
    J = torch.stack([fx / tz, zero, -(fx * tx) / (tz * tz), zero, fy / tz, -(fy * ty) / (tz * tz)], dim=1).reshape(P, 2, 3)
    Rw2c = V[:3, :3].transpose(0, 1)  # p_view = Rw2c @ p + t
    A = J @ Rw2c
    cov2 = A @ Sigma @ A.transpose(1, 2)
    a = cov2[:, 0, 0] + 0.3; b = cov2[:, 0, 1]; c = cov2[:, 1, 1] + 0.3
    det = a * c - b * b
    conic = torch.stack([c / det, -b / det, a / det], dim=1)

    if colors_precomp is not None:
        pre, col = None, colors_precomp
    else:
        d = means3D - campos[None]
        d = d / d.norm(dim=1, keepdim=True)
        pre = eval_sh_unclamped(sh_degree, shs, d.detach() if detach_direction else d)
        col = torch.clamp_min(pre, 0.0)
    return dict(p_proj=p_proj, cov2=torch.stack([a, b, c], dim=1), det=det, conic=conic, color_unclamped=pre, color=col,
                in_x=in_x, in_y=in_y)


def preprocess_backward_ref(record, sums, *, means3D, shs=None, colors_precomp=None, scales=None, rotations=None,
                            cov3D_precomp=None, viewmatrix, projmatrix, campos, W, H, tanfovx, tanfovy, sh_degree=3,
                            scale_modifier=1.0, raw=False, detach_direction=False, clamp_as_constant=True, eps_term=True):
    """float64 restatement of the backward preprocess (backward.cu preprocessCUDA + computeCov2DCUDA) through autograd, fed like the
    kernel: the forward's record of every Gaussian and the nine sums of the blend backward.

      record   dict of float32 values as the forward left them: opacity [P] (activated), conic [P,3], clamped [P,3] (bool: the
               colour channel was clamped at 0), radii [P] (int)
      sums     [P,9]: {r, g, b, S0} {Sx, Sy, Sxx, Sxy} Syy
      raw      scales are log scales, rotations un-normalised quaternions (torch.nn.functional.normalize, eps 1e-12), the opacity
               a logit: the gradients are those of the raw parameters (dL_dopacity = S0 op (1 - op), op from the record)

    The finishing step of the blend backward (backward.cu:538-554), evaluated in float64 from the float32 record:
      g_mean2D = -(op 0.5 W)(cx Sx + cy Sy), -(op 0.5 H)(cz Sy + cy Sx);  g_conic = -0.5 op (Sxx, Sxy, Syy);  g_color = (r, g, b)
    then the gradient of
      g_mean2D . p_proj.xy + g_conic.x A + 2 g_conic.y B + g_conic.z C + sum(not clamped * g_color * colour before its clamp)
    with the conic cotangents scaled by det^2 / (det^2 + 1e-7) (the reference divides by denom^2 + 1e-7; eps_term=False leaves the
    factor out).  Rows with radius <= 0 are zero in every output.  dL_dscale is, as in the reference, the derivative with respect to
    scale_modifier * scale (backward.cu:295-325 never multiplies by the modifier): autograd's, divided by scale_modifier.
    -> dict of float64 numpy arrays: mean2D [P,2], mean2D_mag [P,2], conic [P,3], conic_mag [P,3] (the sums of the magnitudes of the
       terms: what float32 rounding of the finishing step scales with), opacity [P], color [P,3] (clamp-masked when shs are used),
       mean3D [P,3], and scale [P,3] + rot [P,4] or cov3D [P,6], sh [P,M,3] or colors_precomp [P,3]."""
    import numpy as np
    def f64(t):
        if t is None:
            return None
        return t.detach().double() if torch.is_tensor(t) else torch.as_tensor(np.asarray(t, dtype=np.float64))
    P = np.asarray(record["radii"]).shape[0]
    vis = torch.as_tensor(np.asarray(record["radii"]) > 0)
    n = int(vis.sum())
    op = f64(np.asarray(record["opacity"], dtype=np.float32).reshape(-1))[vis]
    cn = f64(np.asarray(record["conic"], dtype=np.float32))[vis]
    keep = ~torch.as_tensor(np.asarray(record["clamped"]).astype(bool))[vis]
    S = f64(np.asarray(sums, dtype=np.float32).reshape(P, 9))[vis]
    Sx, Sy = S[:, 4], S[:, 5]
    t_x = torch.stack([cn[:, 0] * Sx, cn[:, 1] * Sy], dim=1); t_y = torch.stack([cn[:, 2] * Sy, cn[:, 1] * Sx], dim=1)
    kx, ky = (op * 0.5 * W)[:, None], (op * 0.5 * H)[:, None]
    g_mean2D = torch.stack([-(kx * t_x).sum(1), -(ky * t_y).sum(1)], dim=1)
    mean2D_mag = torch.stack([(kx * t_x).abs().sum(1), (ky * t_y).abs().sum(1)], dim=1)
    g_conic = -0.5 * op[:, None] * S[:, 6:9]
    g_color = S[:, 0:3]

    leaves = {}
    def leaf(name, t):
        if t is None:
            return None
        leaves[name] = f64(t)[vis].clone().requires_grad_(True)
        return leaves[name]
    kw = dict(viewmatrix=f64(viewmatrix), projmatrix=f64(projmatrix), campos=f64(campos), W=W, H=H, tanfovx=tanfovx, tanfovy=tanfovy,
              sh_degree=sh_degree, scale_modifier=scale_modifier, clamp_as_constant=clamp_as_constant, detach_direction=detach_direction)
    m = leaf("mean3D", means3D)
    if cov3D_precomp is not None:
        kw["cov3D_precomp"] = leaf("cov3D", cov3D_precomp)
    else:
        s, q = leaf("scale", scales), leaf("rot", rotations)
        kw["scales"] = torch.exp(s) if raw else s
        kw["rotations"] = torch.nn.functional.normalize(q, dim=1, eps=1e-12) if raw else q
    if colors_precomp is not None:
        kw["colors_precomp"] = leaf("colors_precomp", colors_precomp)
    else:
        kw["shs"] = leaf("sh", shs)
    out = {}
    if n:
        pp = preprocess(m, **kw)
        det = pp["det"].detach()
        gc = g_conic * (det * det / (det * det + 0.0000001))[:, None] if eps_term else g_conic
        L = (g_mean2D * pp["p_proj"][:, :2]).sum() + (gc[:, 0] * pp["conic"][:, 0] + 2.0 * gc[:, 1] * pp["conic"][:, 1]
                                                      + gc[:, 2] * pp["conic"][:, 2]).sum()
        if colors_precomp is not None:
            L = L + (g_color * pp["color"]).sum()
        else:
            L = L + (keep * g_color * pp["color_unclamped"]).sum()
        grads = torch.autograd.grad(L, list(leaves.values()), allow_unused=True)
    else:
        grads = [None] * len(leaves)

    def full(t, *shape):
        o = np.zeros((P,) + shape)
        if t is not None and n:
            o[vis.numpy()] = t.detach().numpy().reshape((n,) + shape)
        return o
    for (name, lf), g in zip(leaves.items(), grads):
        out[name] = full(g, *lf.shape[1:])
    if "scale" in out:
        out["scale"] /= scale_modifier
    out["mean2D"] = full(g_mean2D, 2); out["mean2D_mag"] = full(mean2D_mag, 2)
    out["conic"] = full(g_conic, 3); out["conic_mag"] = full(g_conic.abs(), 3)
    out["opacity"] = full(S[:, 3] * op * (1.0 - op) if raw else S[:, 3])
    out["color"] = full(g_color if colors_precomp is not None else g_color * keep, 3)
    return out


def render(means3D, means2D, opacities, *, shs=None, colors_precomp=None, scales=None, rotations=None,
           cov3D_precomp=None, viewmatrix, projmatrix, campos, bg, W, H, tanfovx, tanfovy, sh_degree=3,
           scale_modifier=1.0, point_list, ranges, radii):
    """Differentiable image [3,H,W].  point_list / ranges / radii come from the C oracle."""
    dt = means3D.dtype
    bg = bg.to(dt)
    pp = preprocess(means3D, shs=shs, colors_precomp=colors_precomp, scales=scales, rotations=rotations,
                    cov3D_precomp=cov3D_precomp, viewmatrix=viewmatrix, projmatrix=projmatrix, campos=campos, W=W, H=H,
                    tanfovx=tanfovx, tanfovy=tanfovy, sh_degree=sh_degree, scale_modifier=scale_modifier)
    p_proj, conic, col = pp["p_proj"], pp["conic"], pp["color"]
    WH = torch.tensor([W, H], dtype=dt)
    pix = ((p_proj[:, :2] + means2D[:, :2] + 1.0) * WH - 1.0) * 0.5

    op = opacities.reshape(-1)
    out = torch.zeros(3, H, W, dtype=dt)
    n_contrib = torch.zeros(H, W, dtype=torch.int64)
    gx = (W + 15) // 16
    pl = torch.as_tensor(point_list.astype("int64"))
    for tile in range(ranges.shape[0]):
        r0, r1 = int(ranges[tile, 0]), int(ranges[tile, 1])
        tx0, ty0 = (tile % gx) * 16, (tile // gx) * 16
        xs = torch.arange(tx0, min(tx0 + 16, W)); ys = torch.arange(ty0, min(ty0 + 16, H))
        if len(xs) == 0 or len(ys) == 0:
            continue
        yy, xx = torch.meshgrid(ys, xs, indexing="ij")
        pxf = xx.reshape(-1).to(dt); pyf = yy.reshape(-1).to(dt)
        npx = pxf.shape[0]
        if r1 == r0:
            out[:, yy.reshape(-1), xx.reshape(-1)] = bg[:, None].expand(3, npx)
            continue
        ids = pl[r0:r1]
        dx = pix[ids, 0][None, :] - pxf[:, None]
        dy = pix[ids, 1][None, :] - pyf[:, None]
        cn = conic[ids]
        power = -0.5 * (cn[:, 0][None] * dx * dx + cn[:, 2][None] * dy * dy) - cn[:, 1][None] * dx * dy
        raw = op[ids][None] * torch.exp(power.clamp_max(0.0))
        alpha = raw + (torch.clamp_max(raw, 0.99) - raw).detach()  # straight-through min(0.99, .)
        valid = (power <= 0) & (alpha.detach() >= 1.0 / 255.0)
        a_eff = torch.where(valid, alpha, torch.zeros_like(alpha))
        with torch.no_grad():
            one_m = 1.0 - a_eff
            T_incl = torch.cumprod(one_m, dim=1)  # test_T after each entry
            stop = valid & (T_incl < 0.0001)
            n = a_eff.shape[1]
            idx = torch.arange(n)[None].expand_as(stop)
            first_stop = torch.where(stop, idx, torch.full_like(idx, n)).min(dim=1).values
            keep = idx < first_stop[:, None]
            contrib_pos = torch.where(valid & keep, idx + 1, torch.zeros_like(idx)).max(dim=1).values
        a_eff = torch.where(keep, a_eff, torch.zeros_like(a_eff))
        one_m = 1.0 - a_eff
        T_incl = torch.cumprod(one_m, dim=1)
        T_excl = torch.cat([torch.ones(npx, 1, dtype=dt), T_incl[:, :-1]], dim=1)
        wgt = a_eff * T_excl
        Cc = wgt @ col[ids]  # [npx,3]
        T_fin = T_incl[:, -1]
        res = Cc + T_fin[:, None] * bg[None]
        out[:, yy.reshape(-1), xx.reshape(-1)] = res.transpose(0, 1)
        n_contrib[yy.reshape(-1), xx.reshape(-1)] = contrib_pos
    return out, n_contrib
