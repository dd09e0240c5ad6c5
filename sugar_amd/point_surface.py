"""A triangle mesh from an oriented point cloud, on the device: a LOCAL implicit surface (implicit moving least squares, IMLS) evaluated
in the 8 x 8 x 8-point bricks near the cloud (csrc/point_surface.hip; C ABI: sgr_point_surface_* in include/sugar_raster.h) and meshed
by sugar_amd.marching_cubes.  It stands where the reference calls open3d's Poisson reconstruction on the level-set points of every
training camera (sugar_extractors/coarse_mesh.py:372-418), and it is NOT Poisson reconstruction: there is no global solve, every grid
value depends on the K nearest cloud points only, and it fills no hole -- a region without points stays open.  There is no `open3d`
module here.

  implicit_at(x, points, normals, radius, K=16)                    -> (value[N], weight[N])
  implicit_grid(X, Y, Z, points, normals, radius, K=16, ...)       -> volume[nx,ny,nz], NaN where undefined
  mesh_from_oriented_points(points, normals, X, Y, Z, ...)         -> dict(verts, faces, normals, weights[, colors])
  statistical_outlier_mask(points, nb_neighbors=20, std_ratio=20.) -> bool[N], the points to keep

The rules (the kernel file states them in full; tests/point_surface_restatement.py restates them in numpy): with h = radius / 2 and the
K nearest cloud points p_k (normals n_k, towards lower density) of a query x, in float32,
    f(x) = - sum_k w_k <x - p_k, n_k> / sum_k w_k,   w_k = exp(-|x - p_k|^2 / h^2),   weight(x) = sum_k w_k,
defined iff the nearest of them lies within `radius` (value NaN, weight 0 otherwise); f <= 0 is inside.  Marching cubes counts NaN as
outside and so walls off the band's inside against undefined grid points; those faces are recognised exactly (a vertex between a
finite and a non-finite grid point) and dropped.  GPU tensors only: CPU tensors raise."""
from __future__ import annotations

import math

import torch

from . import _lib
from ._call import call, need_gpu, ptr as p
from . import decimate as _decimate
from . import marching_cubes as _mc
from .knn import knn_points

BRICK = 8    # points per brick edge (csrc/sparse_sweep.hip)
MAX_K = 32


def _cloud(what, points, normals, K):
    need_gpu(what, points=points, normals=normals)
    if points.dim() != 2 or points.shape[1] != 3 or normals.shape != points.shape:
        raise ValueError(f"{what}: points and normals must both be [N,3]")
    K, N = int(K), int(points.shape[0])
    if not 1 <= K <= MAX_K:
        raise ValueError(f"{what}: K must be in [1, {MAX_K}]")
    if K > N:
        raise ValueError(f"{what}: K = {K} exceeds the {N} cloud points")
    return points.detach().to(torch.float32).contiguous(), normals.detach().to(torch.float32).contiguous(), K, N


def _radius(what, radius):
    radius = float(radius)
    if not (math.isfinite(radius) and radius > 0):
        raise ValueError(f"{what}: radius must be finite and positive")
    return radius


def _pack(pts, nrm):
    """the 32-byte records (px, py, pz, nx), (ny, nz, 0, 0): a neighbour is two 16-byte loads"""
    packed = torch.empty(pts.shape[0], 8, dtype=torch.float32, device=pts.device)
    call("sgr_point_surface_pack", pts.device, int(pts.shape[0]), p(pts), p(nrm), p(packed))
    return packed


def _eval(x, pts, packed, radius, K, value, weight):
    n = int(x.shape[0])
    if n:
        idx = knn_points(x[None], pts[None], K=K).idx[0]
        call("sgr_point_surface_eval", x.device, n, K, p(x), p(idx), int(pts.shape[0]), p(packed), radius, p(value), p(weight))


def implicit_at(x, points, normals, radius, K: int = 16):
    """(value[N], weight[N]) float32 of the implicit at the queries x[N,3]: value NaN and weight 0 where no cloud point lies within
    `radius`.  The same kernel, and bit for bit the same values, as `implicit_grid` at the same points.  No host synchronisation."""
    pts, nrm, K, _ = _cloud("implicit_at", points, normals, K)
    need_gpu("implicit_at", x=x)
    if x.dim() != 2 or x.shape[1] != 3:
        raise ValueError("implicit_at: x must be [N,3]")
    radius = _radius("implicit_at", radius)
    _lib.load()
    q = x.detach().to(torch.float32).contiguous()
    value = torch.empty(q.shape[0], dtype=torch.float32, device=q.device)
    weight = torch.empty_like(value)
    _eval(q, pts, _pack(pts, nrm), radius, K, value, weight)
    return value, weight


def _axis(t, name, device):
    if not torch.is_tensor(t) or t.dim() != 1 or t.numel() < 1:
        raise ValueError(f"implicit_grid: {name} must be a 1-D tensor")
    if not t.is_cuda and t.numel() > 1 and not bool((t[1:] > t[:-1]).all()):
        raise ValueError(f"implicit_grid: {name} must be strictly ascending")    # (an axis on the device is checked there)
    return t.detach().to(device=device, dtype=torch.float32).contiguous()


def _sweep(X, Y, Z, points, normals, radius, K, points_per_pass):
    """-> (volume, flags uint8 [>= n_bricks], n_active, (nbx, nby, nbz), state); the body of implicit_grid.  state = the checked inputs
    (X, Y, Z, pts, nrm, packed records or None when nothing is active, radius, K) for the callers that evaluate again at the vertices"""
    pts, nrm, K, N = _cloud("implicit_grid", points, normals, K)
    radius = _radius("implicit_grid", radius)
    points_per_pass = int(points_per_pass)
    if points_per_pass < 1:
        raise ValueError("implicit_grid: points_per_pass must be positive")
    _lib.load()
    dev = pts.device
    X, Y, Z = _axis(X, "X", dev), _axis(Y, "Y", dev), _axis(Z, "Z", dev)
    nx, ny, nz = X.numel(), Y.numel(), Z.numel()
    if nx * ny * nz >= _mc.MAX_POINTS:
        raise ValueError(f"implicit_grid: a grid of {nx} x {ny} x {nz} points is refused: nx * ny * nz must stay below 2^31")
    nb = tuple((n + BRICK - 1) // BRICK for n in (nx, ny, nz))
    n_bricks = nb[0] * nb[1] * nb[2]
    flags = torch.empty((n_bricks + 15) // 16 * 16, dtype=torch.uint8, device=dev)
    meta = torch.empty(4, dtype=torch.int32, device=dev)
    bricks = torch.empty(n_bricks, dtype=torch.int32, device=dev)
    call("sgr_point_surface_mark", dev, N, p(pts), radius, nx, ny, nz, p(X), p(Y), p(Z), p(flags), p(meta))
    call("sgr_sparse_sweep_compact", dev, nx, ny, nz, p(X), p(Y), p(Z), 0, 0.0, 0.0, p(flags), p(bricks), p(meta))
    volume = torch.full((nx, ny, nz), float("nan"), dtype=torch.float32, device=dev)
    n_active, bad_axis = meta.tolist()[:2]                                  # the one device -> host read: it sizes the chunk loop
    if bad_axis:
        raise ValueError("implicit_grid: X, Y and Z must be strictly ascending")
    packed = None
    if n_active:
        packed = _pack(pts, nrm)
        chunk = max(1, points_per_pass // (BRICK ** 3))
        n_max = min(chunk, n_active) * BRICK ** 3
        pts_buf = torch.empty(n_max, 3, dtype=torch.float32, device=dev)
        val_buf = torch.empty(n_max, dtype=torch.float32, device=dev)
        for b0 in range(0, n_active, chunk):
            b1 = min(b0 + chunk, n_active)
            n = (b1 - b0) * BRICK ** 3
            q, val = pts_buf[:n], val_buf[:n]
            call("sgr_sparse_sweep_points", dev, nx, ny, nz, p(X), p(Y), p(Z), p(bricks), b0, b1, p(q))
            _eval(q, pts, packed, radius, K, val, None)
            call("sgr_sparse_sweep_scatter", dev, nx, ny, nz, p(bricks), b0, b1, p(val), p(volume))
    return volume, flags, int(n_active), nb, (X, Y, Z, pts, nrm, packed, radius, K)


def implicit_grid(X, Y, Z, points, normals, radius, K: int = 16, points_per_pass: int = 2_000_000, return_active: bool = False):
    """volume[nx,ny,nz] float32 (z fastest): the implicit at every point of meshgrid(X, Y, Z) that lies within `radius` of a cloud
    point, NaN everywhere else.  The grid is cut into bricks of 8 x 8 x 8 points; a brick is ACTIVE when its in-grid point span, grown
    by radius (1 + 2^-20) on each axis, holds a cloud point (a box rule, conservative under float32 rounding: csrc/point_surface.hip);
    only active bricks go through the k-NN and the evaluation kernel.  X, Y, Z strictly ascending (ValueError otherwise); points and
    normals finite; 1 <= K <= 32, K <= N.  The result does not depend on `points_per_pass` (chunks of max(1, points_per_pass // 512)
    bricks; every point is computed on its own).  `return_active=True`: returns (volume, mask), mask bool [ceil(nx/8), ceil(ny/8),
    ceil(nz/8)] of the active bricks.
    One device -> host read per call: the number of active bricks; with none active nothing further is launched."""
    volume, flags, _, nb, _ = _sweep(X, Y, Z, points, normals, radius, K, points_per_pass)
    if return_active:
        return volume, flags[:nb[0] * nb[1] * nb[2]].view(*nb).bool()
    return volume


def spurious_vertices(verts_index, volume):
    """bool[V]: the marching-cubes vertices (index coordinates) that lie between a finite and a non-finite grid point -- volume at
    floor(c) or ceil(c) is not finite.  No host synchronisation."""
    need_gpu("spurious_vertices", verts_index=verts_index, volume=volume)
    nx, ny, nz = (int(s) for s in volume.shape)
    v = verts_index.detach().to(torch.float32).contiguous()
    out = torch.empty(v.shape[0], dtype=torch.uint8, device=v.device)
    call("sgr_point_surface_spurious", v.device, int(v.shape[0]), p(v), nx, ny, nz, p(volume.contiguous()), p(out))
    return out.bool()


def _index_mesh(X, Y, Z, points, normals, radius, K, points_per_pass):
    """the mesh in index coordinates after the spurious-face rule: (verts_index, faces, state)"""
    volume, _, n_active, _, state = _sweep(X, Y, Z, points, normals, radius, K, points_per_pass)
    dev = volume.device
    empty = (torch.zeros(0, 3, dtype=torch.float32, device=dev), torch.zeros(0, 3, dtype=torch.int64, device=dev), state)
    if not n_active:
        return empty                                                        # nothing further is launched
    verts_index, faces = _mc.marching_cubes(volume, 0.0)                    # read 2: (V, F)
    if not faces.shape[0]:
        return empty
    verts_index, faces = _decimate.remove_vertices_by_mask(verts_index, faces, spurious_vertices(verts_index, volume), unreferenced=True)
    return verts_index, faces, state                                        # read 3: the surviving (V, F)


def mesh_from_oriented_points(points, normals, X, Y, Z, radius=None, K: int = 16, colors=None, weight_quantile: float = 0.0,
                              decimation_target=None, clean: bool = False, points_per_pass: int = 2_000_000):
    """The mesh of the implicit's zero set: `implicit_grid`, `marching_cubes(volume, 0.0)`, the spurious-face rule (every face with a
    vertex between a finite and a non-finite grid point is dropped, then every vertex no face names; order kept) and `grid_to_world`.
    points[N,3], normals[N,3] (towards lower density, as sampler.sample_level_sets returns them); radius=None: 3 x the largest spacing
    of the three axes.  Returns dict(verts[V,3] float32, faces[F,3] int64 wound outwards, normals[V,3], weights[V] = the implicit's
    weight at the vertex, and colors[V, ...] = colors[nearest cloud point] when `colors[N, ...]` is given).
    weight_quantile=q > 0: the vertices whose weight is below the q-quantile of all weights are removed with their faces
    (`quantile` below, float64; sugar_amd.decimate.remove_vertices_by_mask; the reference's `vertices_density_quantile` trim,
    coarse_mesh.py:392-395).  The default
    is 0: the implicit fills no hole, so there is no filled-in surface to take away.  Then decimation_target=N / clean=True run
    sugar_amd.decimate.decimate / clean (weights and colours are then taken at the final vertices).
    Device -> host reads per call: the active-brick count, marching cubes' (V, F), the surviving (V, F) of the spurious-face rule, and
    one more (V, F) if the quantile trim is on; decimate and clean add their own, and radius=None reads the spacing of device axes.  With no active brick nothing further is launched
    and the mesh is empty.  This is not Poisson reconstruction: holes stay open."""
    from .extract import grid_to_world
    if not 0.0 <= float(weight_quantile) < 1.0:
        raise ValueError("mesh_from_oriented_points: weight_quantile must be in [0, 1)")
    if decimation_target is not None and int(decimation_target) < 0:
        raise ValueError("mesh_from_oriented_points: decimation_target must not be negative")
    need_gpu("mesh_from_oriented_points", points=points, normals=normals)
    dev = points.device
    if radius is None:
        gaps = [float((a[1:].double() - a[:-1].double()).max()) for a in (X, Y, Z) if torch.is_tensor(a) and a.dim() == 1 and a.numel() > 1]
        if not gaps:
            raise ValueError("mesh_from_oriented_points: radius=None needs an axis with at least two points")
        radius = float(torch.tensor(3.0 * max(gaps), dtype=torch.float32))
    if colors is not None and (not torch.is_tensor(colors) or colors.shape[0] != points.shape[0]):
        raise ValueError("mesh_from_oriented_points: colors must have one row per cloud point")
    verts_index, faces, (X, Y, Z, pts, nrm, packed, radius, K) = _index_mesh(X, Y, Z, points, normals, radius, K, points_per_pass)
    if not verts_index.shape[0]:
        mesh = dict(verts=verts_index, faces=faces, normals=verts_index.clone(), weights=verts_index.new_zeros(0))
        if colors is not None:
            mesh["colors"] = colors.detach().to(dev)[:0]
        return mesh
    verts = grid_to_world(verts_index, X, Y, Z)

    def weights_at(v):
        w = torch.empty(v.shape[0], dtype=torch.float32, device=dev)
        _eval(v, pts, packed, radius, K, torch.empty_like(w), w)
        return w

    weights = weights_at(verts.contiguous())
    if float(weight_quantile) > 0 and verts.shape[0]:
        below = weights.double() < quantile(weights, float(weight_quantile))
        verts, faces, weights = _decimate.remove_vertices_by_mask(verts, faces, below, weights)                 # read 4
    post = False
    if decimation_target is not None and faces.shape[0]:
        verts, faces, _ = _decimate.decimate(verts, faces, int(decimation_target))
        post = True
    if clean and faces.shape[0]:
        verts, faces, _ = _decimate.clean(verts, faces)
        post = True
    if post:
        weights = weights_at(verts.contiguous())
    mesh = dict(verts=verts, faces=faces, normals=_mc.vertex_normals(verts, faces) if verts.shape[0] else verts.new_zeros(0, 3),
                weights=weights)
    if colors is not None:
        c = colors.detach().to(dev)
        mesh["colors"] = c[knn_points(verts[None].contiguous(), pts[None], K=1).idx[0, :, 0]] if verts.shape[0] else c[:0]
    return mesh


def quantile(values, q):
    """the q-quantile of a 1-D tensor in float64, linear interpolation between the order statistics at q (n - 1) (numpy's default
    rule), as a 0-d tensor; by a sort, so that the length is not bounded as `torch.quantile`'s is.  No host synchronisation."""
    s = torch.sort(values.double()).values
    pos = float(q) * (s.numel() - 1)
    i = min(int(math.floor(pos)), s.numel() - 1)
    j = min(i + 1, s.numel() - 1)
    return s[i] + (pos - i) * (s[j] - s[i])


def statistical_outlier_mask(points, nb_neighbors: int = 20, std_ratio: float = 20.0):
    """bool[N], True for the points to KEEP: the step of coarse_mesh.py:382 (`remove_statistical_outlier(20, 20.)`) with this rule, which
    is ours -- open3d is absent and no bit-parity with it is claimed: d_i = the mean Euclidean distance from point i to its
    `nb_neighbors` nearest cloud points, itself included (HIP k-NN of the cloud on itself; min(nb_neighbors, N, 32) neighbours); a point
    is kept iff d_i <= mean(d) + std_ratio x std(d), std the sample standard deviation (N - 1; 0 for N < 2).  float64 statistics.
    No host synchronisation."""
    need_gpu("statistical_outlier_mask", points=points)
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("statistical_outlier_mask: points must be [N,3]")
    N = int(points.shape[0])
    if N == 0:
        return torch.zeros(0, dtype=torch.bool, device=points.device)
    k = max(1, min(int(nb_neighbors), N, MAX_K))
    pts = points.detach().to(torch.float32).contiguous()
    d2 = knn_points(pts[None], pts[None], K=k).dists[0]
    return outlier_rule(d2.clamp_min(0).sqrt().double().mean(dim=1), std_ratio)


def outlier_rule(mean_dist, std_ratio):
    """keep iff mean_dist <= mean + std_ratio x sample std (works on CPU tensors too: the tests state the rule through it)"""
    m = mean_dist.double()
    std = m.std(unbiased=True) if m.numel() > 1 else m.new_zeros(())
    return m <= m.mean() + float(std_ratio) * std
