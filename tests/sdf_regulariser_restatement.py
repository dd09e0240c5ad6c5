"""TEST INFRASTRUCTURE: the four operations of csrc/sdf_regulariser.hip written out as plain torch, from their formulas (not from the
reference's lines), in whatever dtype the inputs have: float64 for the parity tests (tests/test_gpu_sdf_regulariser.py, the `yard_*`
distances of tests/golden/make_sdf_regulariser.py), float32 as the torch composition scripts/sdf_regulariser_bench.py times.
Gradients come from autograd.

    sample transform   x_n = mu_i + rot(q_i, f * s_i (.) eps_n),  i = idx[n];  rot(q, v) = vec(q (x) (0, v) (x) conj(q)), q as given
    smallest axis      n_p = column j of R(q_p),  j = argmin_j s_p[j] (lowest j on ties),  R = I + 2 / |q|^2 * M(q)
    depth lookup       c = [x y z 1] * Pm,  ndc = c.xy / c.w,  g = -min(H, W) / (W, H) * ndc,  i = ((g + 1) * (W, H) - 1) / 2, clamped to
                       the image with a zero derivative where the clamp is active, bilinear taps
    sdf field          o = f * strength * exp(-|B^T (x - mu)|^2 / 2) (the squared norm clamped to [0, 1e8]),  density = sum_k o,
                       d' = density < 1 ? density : density / (density + 1e-12) (constant denominator),  beta = mean_k min_scaling[nbr_k],
                       sdf = beta * (sqrt(-2 ln max(d', clamp)) - sqrt(-2 ln min(threshold, 1)))
"""
import math

import torch


def distance(a, b) -> float:
    """norm-wise relative distance |a - b| / |b| over the entries where b is finite, in float64"""
    a = torch.as_tensor(a).detach().cpu().double().reshape(-1)
    b = torch.as_tensor(b).detach().cpu().double().reshape(-1)
    ok = torch.isfinite(b)
    return float((a[ok] - b[ok]).norm() / b[ok].norm().clamp_min(1e-30))


def _hamilton(a, b):
    aw, ax, ay, az = a.unbind(-1)
    bw, bx, by, bz = b.unbind(-1)
    return torch.stack((aw * bw - ax * bx - ay * by - az * bz,
                        aw * bx + ax * bw + ay * bz - az * by,
                        aw * by - ax * bz + ay * bw + az * bx,
                        aw * bz + ax * by - ay * bx + az * bw), -1)


def rotate(q, v):
    """vector part of q (x) (0, v) (x) conj(q); q is NOT normalised"""
    V = torch.cat((torch.zeros_like(v[..., :1]), v), -1)
    conj = q * q.new_tensor([1.0, -1.0, -1.0, -1.0])
    return _hamilton(_hamilton(q, V), conj)[..., 1:]


def sample_transform(points, quaternions, scaling, idx, noise, factor):
    return points[idx] + rotate(quaternions[idx], factor * scaling[idx] * noise)


def rotation_matrix(q):
    r, i, j, k = q.unbind(-1)
    t = 2.0 / (q * q).sum(-1)
    M = torch.stack((-(j * j + k * k), i * j - k * r, i * k + j * r,
                     i * j + k * r, -(i * i + k * k), j * k - i * r,
                     i * k - j * r, j * k + i * r, -(i * i + j * j)), -1).reshape(q.shape[:-1] + (3, 3))
    return torch.eye(3, dtype=q.dtype, device=q.device) + t[..., None, None] * M


def smallest_axis(quaternions, scaling):
    """(axis[P,3], j[P]); the lowest j wins on ties"""
    s = scaling.detach()
    j = torch.zeros(s.shape[0], dtype=torch.int64, device=s.device)
    m = s[:, 0]
    for c in (1, 2):
        lower = s[:, c] < m
        j = torch.where(lower, torch.full_like(j, c), j)
        m = torch.where(lower, s[:, c], m)
    R = rotation_matrix(quaternions)
    return R.gather(2, j[:, None, None].expand(-1, 3, 1))[..., 0], j


def _clamped_pixel(g, size):
    i = ((g + 1.0) * size - 1.0) / 2.0
    zero = torch.zeros_like(i)            # constants: no derivative where the clamp is active
    return torch.where(i <= 0, zero, torch.where(i >= size - 1, zero + (size - 1), i))


def lookup_pixels(projection, points, H, W):
    """(ix, iy) after the clamp, and the mask of the points whose pixel was clamped (outside the image)"""
    Pm = projection.reshape(4, 4).to(points.dtype)
    c = torch.cat((points, torch.ones_like(points[:, :1])), -1) @ Pm
    ndc = c[:, :2] / c[:, 3:4]
    m = float(min(H, W))
    ix = _clamped_pixel(-m / W * ndc[:, 0], W)
    iy = _clamped_pixel(-m / H * ndc[:, 1], H)
    outside = (ix <= 0) | (ix >= W - 1) | (iy <= 0) | (iy >= H - 1)
    return ix, iy, outside


def depth_lookup(projection, depth, points):
    """depth: [H, W] (any strides); points: [M, 3] in camera space"""
    H, W = depth.shape
    depth = depth.to(points.dtype)
    ix, iy, _ = lookup_pixels(projection, points, H, W)
    x0, y0 = ix.detach().floor().long(), iy.detach().floor().long()
    x1, y1 = x0 + 1, y0 + 1
    wx1, wy1 = ix - x0, iy - y0
    wx0, wy0 = x1 - ix, y1 - iy
    flat = depth.reshape(-1)

    def tap(y, x):
        inside = ((x < W) & (y < H)).to(points.dtype)        # a tap past the last row / column carries no value (its weight is 0 there)
        return flat[y.clamp(max=H - 1) * W + x.clamp(max=W - 1)] * inside
    return tap(y0, x0) * wx0 * wy0 + tap(y0, x1) * wx1 * wy0 + tap(y1, x0) * wx0 * wy1 + tap(y1, x1) * wx1 * wy1


def sdf_field(x, nbr_idx, centers, inv_scaled_rot, strengths, min_scaling, density_factor=1.0, density_threshold=1.0,
              opacity_min_clamp=1e-16):
    """(neighbor_opacities[N,K], density[N], beta[N], sdf[N])"""
    P = centers.shape[0]
    B = inv_scaled_rot.reshape(P, 3, 3)[nbr_idx]                               # [N,K,3,3]
    d = x[:, None] - centers[nbr_idx]                                          # [N,K,3]
    w = (B * d[..., :, None]).sum(-2)                                          # w_j = sum_i B[i][j] d_i
    q = (w * w).sum(-1).clamp(min=0.0, max=1e8)
    o = density_factor * strengths.reshape(P)[nbr_idx] * torch.exp(-0.5 * q)
    density = o.sum(-1)
    dprime = torch.where(density < 1.0, density, density / (density.detach() + 1e-12))
    beta = min_scaling.reshape(P)[nbr_idx].mean(-1)
    offset = math.sqrt(-2.0 * math.log(min(density_threshold, 1.0)))
    sdf = beta * (torch.sqrt(-2.0 * torch.log(dprime.clamp(min=opacity_min_clamp))) - offset)
    return o, density, beta, sdf
