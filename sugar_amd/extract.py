"""Coarse mesh extraction by marching cubes, on the device from the Gaussians to the mesh: the `use_marching_cubes` branch of
sugar_extractors/coarse_mesh.py (:623-757); its open3d calls (decimation, cleaning) are sugar_amd.decimate's, on request.

  density_grid(X, Y, Z, centers, inv_scaled_rot, strengths, ...)  -> volume[nx,ny,nz]: `SuGaR.compute_density` (sugar_model.py:1345-1368)
      on the grid meshgrid(X, Y, Z), swept in slabs: sgr_grid_points writes a slab's points, the HIP k-NN finds each point's K nearest
      Gaussians (what `get_gaussians_closest_to_samples` does), the HIP density field (`k_density_fwd`) sums their opacities, straight
      into the volume.  The reference's [512^3, 3] point tensor (1.6 GB) and its repeated `torch.cat` never exist.
  density_grid_sparse(X, Y, Z, centers, inv_scaled_rot, strengths, level, ...)  -> the same volume wherever marching cubes at `level` reads
      it, and 0 elsewhere: only the 8 x 8 x 8-point bricks a Gaussian can reach (csrc/sparse_sweep.hip) go through the k-NN and the
      density kernel.  The mesh is bit-identical to the dense sweep's; `sweep="sparse"` below and `--sweep sparse` select it.
  extract_mesh_marching_cubes(points, scales, quaternions, opacities, sh_dc, extent, ...) -> dict(verts, faces, normals, colors):
      the foreground grid over +-extent, the background grid over +-4 extent with the foreground box blanked (:698), marching cubes
      (sugar_amd.marching_cubes), colours 0.5 + C0 * dc of the nearest Gaussian (SH2RGB, :664), vertex normals, both meshes concatenated.

  extract_mesh_level_sets(points, scales, quaternions, opacities, sh_dc, cameras, extent, ...) -> the same dict plus weights: the
      reference's DEFAULT route (coarse_mesh.py:243-490) -- level-set points with normals sampled from every camera
      (sugar_amd.sampler), split into foreground and background, outliers removed -- with sugar_amd.point_surface's local implicit
      surface where the reference calls open3d's Poisson reconstruction.  It is not Poisson: holes stay open.  Opt-in (`--route levelset`).

Deliberate differences from the reference:
  * vertices sit at the true grid coordinates X[i] + t (X[i+1] - X[i]).  The reference maps index coordinates with
    `-extent + vertices / resolution * 2 extent` (:661) although linspace(-1, 1, resolution) has a spacing of 2 / (resolution - 1): its
    vertices are off by up to one cell at the far end of each axis;
  * decimation and cleaning are opt-in: by default the mesh returned here is the full marching-cubes mesh.  With `decimation_target=N`
    the foreground and the background mesh are each decimated to N faces by sugar_amd.decimate.decimate, and with `clean=True` each is
    then cleaned by sugar_amd.decimate.clean -- `simplify_quadric_decimation` and the `remove_*` calls of :716-742, as native HIP code
    with its own stated rules (not open3d's implementation).  Normals and colours are computed after both.

    python -m sugar_amd.extract point_cloud.ply --out mesh.ply [--resolution 512 --level 0.3 --extent E --no-background]
                                                               [--decimate N [--no-clean]] [--sweep {dense,sparse}]
    python -m sugar_amd.extract point_cloud.ply --route levelset --cameras cameras.json --out mesh.ply [--surface-level 0.3 --n-points N
                                                               --radius-cells 3 --weight-quantile Q --resolution R --decimate N
                                                               --no-clean --no-background]

There is no CPU path: CPU tensors raise."""
from __future__ import annotations

import argparse
import math

import torch

from . import _lib
from ._call import call, ptr as p
from . import decimate as _decimate
from . import field as _field
from . import marching_cubes as _mc
from .knn import knn_points

SH_C0 = 0.28209479177387814
BACKGROUND_SCALE = 4.0  # the background grid spans +-4 extent (coarse_mesh.py:675-677)


def _axis(t, name, device):
    if not torch.is_tensor(t) or t.dim() != 1 or t.numel() < 1:
        raise ValueError(f"density_grid: {name} must be a 1-D tensor")
    return t.detach().to(device=device, dtype=torch.float32).contiguous()


def density_grid(X, Y, Z, centers, inv_scaled_rot, strengths, K: int = 16, points_per_pass: int = 2_000_000, zero_inside=None):
    """volume[nx,ny,nz] float32 (z fastest): the density of sugar_model.py:1345-1368 at every point of meshgrid(X, Y, Z).
    centers[P,3]; inv_scaled_rot[P,3,3] = get_covariance(return_full_matrix=True, return_sqrt=True, inverse_scales=True); strengths[P]
    or [P,1]; K nearest Gaussians per point (`reset_neighbors(16)`, coarse_mesh.py:627).  `points_per_pass` bounds the slab (the
    result does not depend on it: every point is computed on its own).  `zero_inside=(lo, hi)`: the density is set to 0 at every grid
    point strictly inside the axis-aligned box lo < x, y, z < hi (scalars), the background pass's blanking of the foreground (:698).
    No host synchronisation."""
    if not torch.is_tensor(centers) or not centers.is_cuda:
        raise RuntimeError("density_grid: centers must be a tensor on a ROCm device; there is no CPU fallback")
    lib = _lib.load()
    dev = centers.device
    X, Y, Z = _axis(X, "X", dev), _axis(Y, "Y", dev), _axis(Z, "Z", dev)
    nx, ny, nz = X.numel(), Y.numel(), Z.numel()
    N = nx * ny * nz
    if N >= _mc.MAX_POINTS:
        raise ValueError(f"density_grid: a grid of {nx} x {ny} x {nz} points is refused: nx * ny * nz must stay below 2^31")
    points_per_pass = int(points_per_pass)
    if points_per_pass < 1:
        raise ValueError("density_grid: points_per_pass must be positive")
    P = int(centers.shape[0])
    ce = centers.detach().reshape(P, 3).contiguous().float()
    Bm = inv_scaled_rot.detach().reshape(P, 9).contiguous().float()
    st = strengths.detach().reshape(P).contiguous().float()
    packed = _field._pack(lib, ce, Bm, st)
    volume = torch.empty(nx, ny, nz, dtype=torch.float32, device=dev)
    flat = volume.view(-1)
    n_max = min(points_per_pass, N)
    pts_buf = torch.empty(n_max, 3, dtype=torch.float32, device=dev)
    opac = torch.empty(n_max, int(K), dtype=torch.float32, device=dev)
    for start in range(0, N, points_per_pass):
        n = min(points_per_pass, N - start)
        pts = pts_buf[:n]
        call("sgr_grid_points", dev, nx, ny, nz, p(X), p(Y), p(Z), start, n, p(pts))
        idx = knn_points(pts[None], ce[None], K=int(K)).idx[0]
        dens = flat[start:start + n]
        call("sgr_density_field_forward", dev, n, int(K), p(pts), p(idx), p(ce), p(Bm), p(st), 1.0, p(opac), p(dens), p(packed))
    if zero_inside is not None:
        lo, hi = float(zero_inside[0]), float(zero_inside[1])
        mx, my, mz = ((a > lo) & (a < hi) for a in (X, Y, Z))
        volume.masked_fill_(mx[:, None, None] & my[None, :, None] & mz[None, None, :], 0.0)
    return volume


BRICK = 8  # points per brick edge of the sparse sweep (csrc/sparse_sweep.hip)


def _sparse_sweep(X, Y, Z, centers, inv_scaled_rot, strengths, level, K, points_per_pass, zero_inside):
    """-> (volume, flags uint8 [>= n_bricks], n_active, (nbx, nby, nbz)); the body of density_grid_sparse"""
    level = float(level)
    if not (math.isfinite(level) and level > 0):
        raise ValueError("density_grid_sparse: level must be finite and positive (the skipped points hold 0, which must lie below it)")
    for name, a in (("X", X), ("Y", Y), ("Z", Z)):
        if torch.is_tensor(a) and a.dim() == 1 and not a.is_cuda and a.numel() > 1 and not bool((a[1:] > a[:-1]).all()):
            raise ValueError(f"density_grid_sparse: {name} must be strictly ascending")   # (an axis on the device is checked there)
    K, points_per_pass = int(K), int(points_per_pass)
    if K < 1:
        raise ValueError("density_grid_sparse: K must be positive")
    if points_per_pass < 1:
        raise ValueError("density_grid_sparse: points_per_pass must be positive")
    if not torch.is_tensor(centers) or not centers.is_cuda:
        raise RuntimeError("density_grid_sparse: centers must be a tensor on a ROCm device; there is no CPU fallback")
    lib = _lib.load()
    dev = centers.device
    X, Y, Z = _axis(X, "X", dev), _axis(Y, "Y", dev), _axis(Z, "Z", dev)
    nx, ny, nz = X.numel(), Y.numel(), Z.numel()
    if nx * ny * nz >= _mc.MAX_POINTS:
        raise ValueError(f"density_grid_sparse: a grid of {nx} x {ny} x {nz} points is refused: nx * ny * nz must stay below 2^31")
    P = int(centers.shape[0])
    if P < K:
        raise ValueError(f"density_grid_sparse: {P} Gaussians are fewer than K = {K}")
    ce = centers.detach().reshape(P, 3).contiguous().float()
    Bm = inv_scaled_rot.detach().reshape(P, 9).contiguous().float()
    st = strengths.detach().reshape(P).contiguous().float()
    packed = _field._pack(lib, ce, Bm, st)
    nb = tuple((n + BRICK - 1) // BRICK for n in (nx, ny, nz))
    n_bricks = nb[0] * nb[1] * nb[2]
    gap = torch.stack([(a[1:].double() - a[:-1].double()).max() if a.numel() > 1 else torch.zeros((), dtype=torch.float64, device=dev)
                       for a in (X, Y, Z)])
    flags = torch.empty((n_bricks + 15) // 16 * 16, dtype=torch.uint8, device=dev)
    big = torch.empty(P, dtype=torch.int32, device=dev)
    meta = torch.empty(4, dtype=torch.int32, device=dev)
    bricks = torch.empty(n_bricks, dtype=torch.int32, device=dev)
    call("sgr_sparse_sweep_mark", dev, P, p(packed), K, level, nx, ny, nz, p(X), p(Y), p(Z), p(gap), p(flags), p(big), p(meta))
    box = (float(zero_inside[0]), float(zero_inside[1])) if zero_inside is not None else (0.0, 0.0)
    call("sgr_sparse_sweep_compact", dev, nx, ny, nz, p(X), p(Y), p(Z), int(zero_inside is not None), box[0], box[1], p(flags), p(bricks),
         p(meta))
    volume = torch.zeros(nx, ny, nz, dtype=torch.float32, device=dev)
    n_active, bad_axis = meta.tolist()[:2]                                  # the one device -> host read: it sizes the chunk loop
    if bad_axis:
        raise ValueError("density_grid_sparse: X, Y and Z must be strictly ascending")
    if n_active:
        chunk = max(1, points_per_pass // (BRICK ** 3))
        n_max = min(chunk, n_active) * BRICK ** 3
        pts_buf = torch.empty(n_max, 3, dtype=torch.float32, device=dev)
        opac = torch.empty(n_max, K, dtype=torch.float32, device=dev)
        dens_buf = torch.empty(n_max, dtype=torch.float32, device=dev)
        for b0 in range(0, n_active, chunk):
            b1 = min(b0 + chunk, n_active)
            n = (b1 - b0) * BRICK ** 3
            pts, dens = pts_buf[:n], dens_buf[:n]
            call("sgr_sparse_sweep_points", dev, nx, ny, nz, p(X), p(Y), p(Z), p(bricks), b0, b1, p(pts))
            idx = knn_points(pts[None], ce[None], K=K).idx[0]
            call("sgr_density_field_forward", dev, n, K, p(pts), p(idx), p(ce), p(Bm), p(st), 1.0, p(opac), p(dens), p(packed))
            call("sgr_sparse_sweep_scatter", dev, nx, ny, nz, p(bricks), b0, b1, p(dens), p(volume))
        if zero_inside is not None:
            mx, my, mz = ((a > box[0]) & (a < box[1]) for a in (X, Y, Z))
            volume.masked_fill_(mx[:, None, None] & my[None, :, None] & mz[None, None, :], 0.0)
    return volume, flags, int(n_active), nb


def density_grid_sparse(X, Y, Z, centers, inv_scaled_rot, strengths, level, K: int = 16, points_per_pass: int = 2_000_000, zero_inside=None,
                        return_active: bool = False):
    """volume[nx,ny,nz] float32 from which `marching_cubes(volume, level)` extracts, bit for bit, the mesh it extracts from
    `density_grid(...)` with the same arguments -- at the cost of the k-NN for the grid points near the cloud only.  The grid is cut
    into bricks of 8 x 8 x 8 points; a brick is ACTIVE when the box of a Gaussian that can lift a point to `level` touches it (the rule:
    csrc/sparse_sweep.hip).  Every point of an active brick holds exactly the dense sweep's value; every other point
    holds 0.0 where the dense sweep holds some value below `level` that no crossed edge reads.  Hence `level` must be finite and > 0,
    and X, Y, Z strictly ascending (ValueError otherwise).  `zero_inside=(lo, hi)` additionally drops the bricks wholly inside the box
    (the dense sweep writes 0 there); partly covered bricks are computed and blanked as in `density_grid`.  The result does not depend
    on `points_per_pass` (chunks of max(1, points_per_pass // 512) bricks).  `return_active=True`: returns (volume, mask), mask bool
    [ceil(nx/8), ceil(ny/8), ceil(nz/8)] of the active bricks.
    Preconditions (outside them `density_grid` remains the tool): every inv_scaled_rot has orthogonal columns (it is R diag(1 / sigma));
    all inputs are finite; P >= K.
    One device -> host read per call: the number of active bricks, which sizes the chunk loop; with none active nothing further is
    launched and the volume is all zero."""
    volume, flags, _, nb = _sparse_sweep(X, Y, Z, centers, inv_scaled_rot, strengths, level, K, points_per_pass, zero_inside)
    if return_active:
        return volume, flags[:nb[0] * nb[1] * nb[2]].view(*nb).bool()
    return volume


def grid_to_world(verts_index, X, Y, Z):
    """index coordinates -> X[i] + t (X[i+1] - X[i]) per axis (i = floor, clamped so that the last grid point is i + 1 with t = 1)"""
    out = torch.empty_like(verts_index)
    for a, ax in enumerate((X, Y, Z)):
        c = verts_index[:, a]
        if ax.numel() < 2:
            out[:, a] = ax[0]
            continue
        i = c.floor().clamp(0, ax.numel() - 2).to(torch.int64)
        lo, hi = ax[i], ax[i + 1]
        out[:, a] = lo + (c - i.to(c.dtype)) * (hi - lo)
    return out


def nearest_gaussian_colors(verts, points, sh_dc):
    """SH2RGB of the DC coefficient of the nearest Gaussian (coarse_mesh.py:663-664): 0.5 + C0 * sh_dc[idx]; returns (colors, idx)"""
    if verts.shape[0] == 0:
        return verts.new_zeros(0, 3), torch.zeros(0, dtype=torch.int64, device=verts.device)
    idx = knn_points(verts[None].contiguous(), points[None], K=1).idx[0, :, 0]
    return 0.5 + SH_C0 * sh_dc.reshape(-1, 3)[idx], idx


def _one_mesh(X, centers, B, strengths, sh_dc, level, K, points_per_pass, zero_inside, decimation_target=None, clean=False, sweep="dense"):
    total = ((X.numel() + BRICK - 1) // BRICK) ** 3
    if sweep == "sparse":
        volume, _, active, _ = _sparse_sweep(X, X, X, centers, B, strengths, level, K, points_per_pass, zero_inside)
    else:
        volume, active = density_grid(X, X, X, centers, B, strengths, K=K, points_per_pass=points_per_pass, zero_inside=zero_inside), total
    verts_index, faces = _mc.marching_cubes(volume, level)
    del volume
    verts = grid_to_world(verts_index, X, X, X)
    if decimation_target is not None and faces.shape[0]:
        verts, faces, _ = _decimate.decimate(verts, faces, int(decimation_target))
    if clean and faces.shape[0]:
        verts, faces, _ = _decimate.clean(verts, faces)
    colors, _ = nearest_gaussian_colors(verts, centers, sh_dc)
    normals = _mc.vertex_normals(verts, faces) if verts.shape[0] else verts.new_zeros(0, 3)
    return verts, faces, normals, colors, (active, total)


def extract_mesh_marching_cubes(points, scales, quaternions, opacities, sh_dc, extent, resolution: int = 512, level: float = 0.3,
                                background: bool = True, K: int = 16, points_per_pass: int = 2_000_000, decimation_target=None,
                                clean: bool = False, sweep: str = "dense", return_stats: bool = False):
    """The marching-cubes mesh of a coarse SuGaR model.  points[P,3]; scales[P,3] (activated: `SuGaR.scaling`); quaternions[P,4] (real
    part first); opacities[P] or [P,1] in [0, 1] (`SuGaR.strengths`); sh_dc[P,3] or [P,1,3] (`_sh_coordinates_dc`); extent: the cameras'
    spatial extent (`get_cameras_spatial_extent()`); level: surface_levels[0].
    Returns dict(verts[V,3] float32, faces[F,3] int64, normals[V,3], colors[V,3] in RGB floats (0.5 + C0 dc, not clamped)), the foreground
    mesh first, then (background=True) the background mesh.  decimation_target=N: each of the two meshes is decimated to at most N faces
    (coarse_mesh.py:722-727); clean=True: each is then cleaned (:734-742).  With the defaults neither happens and the output is the full
    marching-cubes mesh.  See the module docstring for the differences from the reference.
    sweep="sparse": both volumes come from `density_grid_sparse` at `level` (which must then be finite and > 0): the same four tensors,
    bit for bit, without the k-NN for the grid points no Gaussian reaches.  return_stats=True adds `active_bricks` and `total_bricks`,
    one entry per pass (foreground, background); a dense pass sweeps every brick."""
    if sweep not in ("dense", "sparse"):
        raise ValueError(f"extract_mesh_marching_cubes: sweep must be 'dense' or 'sparse', not {sweep!r}")
    if not torch.is_tensor(points) or not points.is_cuda:
        raise RuntimeError("extract_mesh_marching_cubes: points must be a tensor on a ROCm device; there is no CPU fallback")
    dev = points.device
    extent = float(extent)
    if not extent > 0:
        raise ValueError("extract_mesh_marching_cubes: extent must be positive")
    resolution = int(resolution)
    if resolution < 2 or resolution ** 3 >= _mc.MAX_POINTS:
        raise ValueError("extract_mesh_marching_cubes: resolution must be in [2, 1290]")
    centers = points.detach().float().contiguous()
    B = _field.scaled_rotation(torch.nn.functional.normalize(quaternions.detach().float(), dim=-1), scales.detach().float(), True)
    strengths = opacities.detach().float().reshape(-1)
    dc = sh_dc.detach().float().reshape(-1, 3)
    lin = torch.linspace(-1, 1, resolution, device=dev)
    if decimation_target is not None and int(decimation_target) < 0:
        raise ValueError("extract_mesh_marching_cubes: decimation_target must not be negative")
    post = (decimation_target, bool(clean), sweep)
    parts = [_one_mesh(lin * extent, centers, B, strengths, dc, level, K, points_per_pass, None, *post)]
    if background:
        parts.append(_one_mesh(lin * BACKGROUND_SCALE * extent, centers, B, strengths, dc, level, K, points_per_pass, (-extent, extent), *post))
    n_fg = parts[0][0].shape[0]
    verts = torch.cat([m[0] for m in parts])
    faces = torch.cat([m[1] + (n_fg if i else 0) for i, m in enumerate(parts)])
    mesh = dict(verts=verts, faces=faces, normals=torch.cat([m[2] for m in parts]), colors=torch.cat([m[3] for m in parts]))
    if return_stats:
        mesh.update(active_bricks=[m[4][0] for m in parts], total_bricks=[m[4][1] for m in parts])
    return mesh


def sample_level_set_cloud(points, scales, quaternions, opacities, cameras, surface_level: float = 0.3, n_total_points: int = 10_000_000,
                           K: int = 16, seed: int = 0):
    """(points[n,3], normals[n,3]) of the level set `surface_level`, sampled from every camera (coarse_mesh.py:243-327): per camera
    `sampler.sample_level_sets(..., sync_free=True, seed=seed + i)` with n_total_points // len(cameras) + 1 pixels (:230); the rows go into
    one preallocated buffer and ONE host wait at the end reads every camera's count."""
    from . import sampler
    dev = points.device
    cameras = list(cameras)
    if not cameras:
        raise ValueError("sample_level_set_cloud: no cameras")
    n = int(n_total_points) // len(cameras) + 1
    means = points.detach().float().contiguous()
    sc = scales.detach().float().contiguous()
    q = torch.nn.functional.normalize(quaternions.detach().float(), dim=-1).contiguous()
    op = opacities.detach().float().reshape(-1, 1).contiguous()
    pts = torch.empty(len(cameras), n, 3, dtype=torch.float32, device=dev)
    nrm = torch.empty(len(cameras), n, 3, dtype=torch.float32, device=dev)
    counts = torch.empty(len(cameras), dtype=torch.int32, device=dev)
    level = float(surface_level)
    for i, cam in enumerate(cameras):
        cam = cam._replace(viewmatrix=cam.viewmatrix.to(dev), projmatrix=cam.projmatrix.to(dev), campos=cam.campos.to(dev))
        r = sampler.sample_level_sets(means, sc, q, op, cam, n_surface_points=n, surface_levels=(level,), K=int(K), sync_free=True,
                                      seed=int(seed) + i)[level]
        pts[i], nrm[i], counts[i] = r["intersection_points"], r["normals"], r["count"]
    counts = counts.tolist()                                             # the one host wait of the sampling loop
    return torch.cat([pts[i, :c] for i, c in enumerate(counts)]), torch.cat([nrm[i, :c] for i, c in enumerate(counts)])


def extract_mesh_level_sets(points, scales, quaternions, opacities, sh_dc, cameras, extent, surface_level: float = 0.3,
                            n_total_points: int = 10_000_000, resolution: int = 512, radius_cells: float = 3.0, K: int = 16,
                            background: bool = True, outlier_std_ratio: float = 20.0, weight_quantile: float = 0.0, decimation_target=None,
                            clean: bool = False, seed: int = 0, return_cloud: bool = False):
    """The level-set mesh of a coarse SuGaR model: the reference's default route with a local implicit surface (sugar_amd.point_surface)
    in the place of open3d's Poisson reconstruction.  Model arguments as `extract_mesh_marching_cubes`; cameras: `synthetic.Camera`-shaped
    tuples (`io.cameras_from_json`).
      sampling   `sample_level_set_cloud` at `surface_level` (one level per call; the caller loops over levels);
      split      foreground: strictly inside +-extent on every axis; background: strictly inside +-4 extent and not foreground
                 (coarse_mesh.py:353-359 with its default factors 1 and 4);
      per part   `point_surface.statistical_outlier_mask(20, outlier_std_ratio)` (:382), then `point_surface.mesh_from_oriented_points` on
                 linspace(-1, 1, resolution) x extent (x 4 extent for the background) with radius = radius_cells x the grid spacing,
                 `weight_quantile`, `decimation_target` and `clean` passed through; a part with fewer than K points gives no mesh.
    Returns dict(verts, faces, normals, colors, weights), the foreground first.  Differences from the reference, all deliberate: the
    surface is NOT Poisson's -- it is defined only within `radius` of a sampled point, so unobserved regions stay open instead of being
    closed by a smooth guess (the reference trims such regions by `vertices_density_quantile`); the vertex colours are 0.5 + C0 dc of the
    nearest Gaussian, as on the marching-cubes route, not the rendered pixel colours of the sampled points.
    return_cloud=True adds `cloud_points` and `cloud_normals` (after the split and the outlier mask, foreground first)."""
    from . import point_surface as _ps
    if not torch.is_tensor(points) or not points.is_cuda:
        raise RuntimeError("extract_mesh_level_sets: points must be a tensor on a ROCm device; there is no CPU fallback")
    dev = points.device
    extent = float(extent)
    if not extent > 0:
        raise ValueError("extract_mesh_level_sets: extent must be positive")
    resolution = int(resolution)
    if resolution < 2 or resolution ** 3 >= _mc.MAX_POINTS:
        raise ValueError("extract_mesh_level_sets: resolution must be in [2, 1290]")
    if not float(radius_cells) > 0:
        raise ValueError("extract_mesh_level_sets: radius_cells must be positive")
    centers = points.detach().float().contiguous()
    dc = sh_dc.detach().float().reshape(-1, 3)
    cloud, cloud_n = sample_level_set_cloud(points, scales, quaternions, opacities, cameras, surface_level, n_total_points, K, seed)
    reach = cloud.abs().max(dim=1).values if cloud.shape[0] else cloud.new_zeros(0)
    fg = reach < extent
    masks = [(fg, 1.0)] + ([((reach < BACKGROUND_SCALE * extent) & ~fg, BACKGROUND_SCALE)] if background else [])
    lin = torch.linspace(-1, 1, resolution, device=dev)
    parts, clouds = [], []
    for mask, scale in masks:
        pts, nrm = cloud[mask], cloud_n[mask]
        if pts.shape[0]:
            keep = _ps.statistical_outlier_mask(pts, 20, outlier_std_ratio)
            pts, nrm = pts[keep], nrm[keep]
        clouds.append((pts, nrm))
        if pts.shape[0] < max(int(K), 1):
            continue
        X = lin * (scale * extent)
        radius = float(torch.tensor(float(radius_cells) * 2.0 * scale * extent / (resolution - 1), dtype=torch.float32))
        m = _ps.mesh_from_oriented_points(pts, nrm, X, X, X, radius=radius, K=K, weight_quantile=weight_quantile,
                                          decimation_target=decimation_target, clean=clean)
        m["colors"] = nearest_gaussian_colors(m["verts"], centers, dc)[0]
        parts.append(m)
    if not parts:
        z = torch.zeros(0, 3, dtype=torch.float32, device=dev)
        mesh = dict(verts=z, faces=torch.zeros(0, 3, dtype=torch.int64, device=dev), normals=z.clone(), colors=z.clone(), weights=z[:, 0].clone())
    else:
        offsets = [0]
        for m in parts[:-1]:
            offsets.append(offsets[-1] + m["verts"].shape[0])
        mesh = {k: torch.cat([m[k] for m in parts]) for k in ("verts", "normals", "colors", "weights")}
        mesh["faces"] = torch.cat([m["faces"] + o for m, o in zip(parts, offsets)])
    if return_cloud:
        mesh.update(cloud_points=torch.cat([c[0] for c in clouds]), cloud_normals=torch.cat([c[1] for c in clouds]))
    return mesh


def _parser():
    ap = argparse.ArgumentParser(description="marching-cubes mesh of a 3DGS / SuGaR point cloud (PLY) on the HIP kernels")
    ap.add_argument("point_cloud")
    ap.add_argument("--out", required=True)
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--level", type=float, default=0.3)
    ap.add_argument("--extent", type=float, default=None,
                    help="half-size of the foreground grid (the cameras' spatial extent); default: the 99th percentile of max(|x|, |y|, |z|)")
    ap.add_argument("--no-background", action="store_true")
    ap.add_argument("--decimate", type=int, default=None, metavar="N",
                    help="decimate the foreground and the background mesh to at most N faces each, then clean them")
    ap.add_argument("--no-clean", action="store_true", help="with --decimate: skip the cleaning passes")
    ap.add_argument("--sweep", choices=("dense", "sparse"), default="dense",
                    help="sparse: run the k-NN only in the 8^3-point bricks a Gaussian can reach; the mesh is the same, bit for bit")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--route", choices=("marching-cubes", "levelset"), default="marching-cubes",
                    help="levelset: sample level-set points with normals from every camera of --cameras and mesh them with a local "
                         "implicit surface (not Poisson reconstruction: holes stay open)")
    ap.add_argument("--cameras", default=None, help="levelset: the cameras.json of the training run")
    ap.add_argument("--surface-level", type=float, default=0.3, help="levelset: the density level the points are sampled on")
    ap.add_argument("--n-points", type=int, default=10_000_000, help="levelset: sampled pixels over all cameras")
    ap.add_argument("--radius-cells", type=float, default=3.0, help="levelset: the support radius of the implicit, in grid spacings")
    ap.add_argument("--weight-quantile", type=float, default=0.0, help="levelset: remove the vertices whose weight is below this quantile")
    return ap


def main(argv=None):
    from . import io
    ap = _parser()
    a = ap.parse_args(argv)
    if a.route == "levelset" and not a.cameras:
        ap.error("--route levelset requires --cameras")
    g = io.load_gaussian_ply(a.point_cloud, device=a.device)
    extent = a.extent
    if extent is None:
        r = g["xyz"].abs().max(dim=1).values
        extent = float(r.kthvalue(max(1, int(0.99 * r.numel()))).values)
    if a.route == "levelset":
        cams, _ = io.cameras_from_json(a.cameras, device=a.device)
        mesh = extract_mesh_level_sets(g["xyz"], torch.exp(g["scaling"]), g["rotation"], torch.sigmoid(g["opacity"]), g["features"][:, 0, :],
                                       cams, extent, surface_level=a.surface_level, n_total_points=a.n_points, resolution=a.resolution,
                                       radius_cells=a.radius_cells, background=not a.no_background, weight_quantile=a.weight_quantile,
                                       decimation_target=a.decimate, clean=a.decimate is not None and not a.no_clean)
        io.save_mesh_ply(a.out, mesh["verts"], mesh["faces"], normals=mesh["normals"], colors=mesh["colors"])
        print(f"{a.out}: {mesh['verts'].shape[0]} vertices, {mesh['faces'].shape[0]} faces (extent {extent:.4g}, level-set route at "
              f"{a.surface_level}, local implicit surface, not Poisson)")
        return 0
    mesh = extract_mesh_marching_cubes(g["xyz"], torch.exp(g["scaling"]), g["rotation"], torch.sigmoid(g["opacity"]), g["features"][:, 0, :],
                                       extent, resolution=a.resolution, level=a.level, background=not a.no_background,
                                       decimation_target=a.decimate, clean=a.decimate is not None and not a.no_clean, sweep=a.sweep,
                                       return_stats=True)
    io.save_mesh_ply(a.out, mesh["verts"], mesh["faces"], normals=mesh["normals"], colors=mesh["colors"])
    swept = ""
    if a.sweep == "sparse":
        act, tot = sum(mesh["active_bricks"]), sum(mesh["total_bricks"])
        swept = f", sparse sweep: {act} of {tot} bricks active ({100.0 * act / tot:.2f} %)"
    print(f"{a.out}: {mesh['verts'].shape[0]} vertices, {mesh['faces'].shape[0]} faces (extent {extent:.4g}, level {a.level}{swept})")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
