"""A numpy restatement of csrc/point_surface.hip and of the mesh rules of sugar_amd.point_surface (test infrastructure, no GPU):

  * `implicit(x, points, normals, idx, radius, dtype)`: the value and weight rules in `dtype` arithmetic (float32: the order of
    operations of the kernel, one rounding per operation; float64: the yardstick), the neighbour lists given by the caller;
  * `spurious_vertices` and `remove_vertices_by_mask`: the spurious-vertex rule and the stable compaction;
  * `bricks_with_defined_point` and `brick_box_rule`: the two sides of the brick sandwich;
  * `outlier_keep`: the statistical outlier rule;
  * the shapes and grids of the tests (`CASES`), with the analytic distance to each surface."""
import numpy as np

BRICK = 8
K = 16


# ---------------------------------------------------------------------------------------------------------------- shapes
def fibonacci_sphere(n, radius):
    """(points, normals) float32: n points on the sphere, the outward normals (towards lower density)"""
    i = np.arange(n, dtype=np.float64) + 0.5
    z = 1.0 - 2.0 * i / n
    phi = i * (np.pi * (3.0 - np.sqrt(5.0)))
    rho = np.sqrt(1.0 - z * z)
    nrm = np.stack([rho * np.cos(phi), rho * np.sin(phi), z], axis=1)
    return (radius * nrm).astype(np.float32), nrm.astype(np.float32)


def torus(R, r, n_u, n_v):
    u, v = np.meshgrid(np.arange(n_u) * (2 * np.pi / n_u), np.arange(n_v) * (2 * np.pi / n_v), indexing="ij")
    u, v = u.reshape(-1), v.reshape(-1)
    nrm = np.stack([np.cos(v) * np.cos(u), np.cos(v) * np.sin(u), np.sin(v)], axis=1)
    ring = np.stack([R * np.cos(u), R * np.sin(u), np.zeros_like(u)], axis=1)
    return (ring + r * nrm).astype(np.float32), nrm.astype(np.float32)


def sphere_distance(p, radius=0.6):
    return np.abs(np.linalg.norm(np.asarray(p, np.float64), axis=1) - radius)


def torus_distance(p, R=0.55, r=0.22):
    p = np.asarray(p, np.float64)
    return np.abs(np.hypot(np.hypot(p[:, 0], p[:, 1]) - R, p[:, 2]) - r)


def _axis(half, n):
    return np.linspace(-half, half, n).astype(np.float32)


def case(name):
    """dict(points, normals, axes=(X, Y, Z), radius float32 = 3 x spacing, distance=the analytic distance or None, closed, chi)"""
    cube = (_axis(1.0, 37), _axis(1.0, 37), _axis(1.0, 37))
    if name == "A":
        pts, nrm = fibonacci_sphere(20_000, 0.6)
        out = dict(points=pts, normals=nrm, axes=cube, distance=sphere_distance, closed=True, chi=2)
    elif name == "A'":
        pts, nrm = fibonacci_sphere(3_000, 0.6)
        out = dict(points=pts, normals=nrm, axes=cube, distance=sphere_distance, closed=True, chi=2)
    elif name == "B":
        pts, nrm = torus(0.55, 0.22, 300, 120)
        out = dict(points=pts, normals=nrm, axes=(_axis(1.0, 37), _axis(1.0, 37), _axis(0.5, 19)), distance=torus_distance, closed=True, chi=0)
    elif name == "C":
        pts, nrm = fibonacci_sphere(20_000, 0.6)
        up = pts[:, 2] > 0
        out = dict(points=pts[up], normals=nrm[up], axes=cube, distance=sphere_distance, closed=False, chi=1)
    else:
        raise KeyError(name)
    spacing = max(float(np.max(np.diff(a.astype(np.float64)))) for a in out["axes"])
    out.update(spacing=spacing, radius=np.float32(3.0 * spacing))
    return out


def grid_points(X, Y, Z):
    """[nx ny nz, 3] float32, z fastest"""
    g = np.stack(np.meshgrid(X, Y, Z, indexing="ij"), axis=-1)
    return np.ascontiguousarray(g.reshape(-1, 3), dtype=np.float32)


def grid_to_world(c, X, Y, Z):
    """index coordinates -> world, the float32 rule of sugar_amd.extract.grid_to_world"""
    out = np.empty_like(c, dtype=np.float32)
    for a, ax in enumerate((X, Y, Z)):
        i = np.clip(np.floor(c[:, a]), 0, ax.size - 2).astype(np.int64)
        lo, hi = ax[i], ax[i + 1]
        out[:, a] = lo + (c[:, a] - i.astype(np.float32)) * (hi - lo)
    return out


# ---------------------------------------------------------------------------------------------------------------- neighbours
def exact_knn(x, points, k, chunk=512):
    """idx[n,k] int64: the k nearest cloud points of every query by float64 distance, nearest first.  scipy's k-d tree where scipy is
    installed (exact, and a hundred times faster), else brute force over all pairs, in chunks (ties to the lower index)."""
    x, pts = np.asarray(x, np.float64), np.asarray(points, np.float64)
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        cKDTree = None
    if cKDTree is not None:
        return cKDTree(pts).query(x, k=k)[1].reshape(x.shape[0], k).astype(np.int64)
    out = np.empty((x.shape[0], k), dtype=np.int64)
    p2 = (pts * pts).sum(axis=1)
    for s in range(0, x.shape[0], chunk):
        q = x[s:s + chunk]
        approx = (q * q).sum(axis=1)[:, None] - 2.0 * (q @ pts.T) + p2[None, :]
        kk = min(pts.shape[0], k + 8)                                  # candidates by the expanded form, then exact distances
        cand = np.argpartition(approx, kk - 1, axis=1)[:, :kk]
        d = ((q[:, None, :] - pts[cand]) ** 2).sum(axis=2)
        order = np.lexsort((cand, d), axis=1)[:, :k]
        out[s:s + chunk] = np.take_along_axis(cand, order, axis=1)
    return out


# ---------------------------------------------------------------------------------------------------------------- the implicit
def implicit(x, points, normals, idx, radius, dtype=np.float32):
    """(value[n], weight[n]) in `dtype`: the rules at the top of csrc/point_surface.hip.  radius: a float32 value."""
    T = dtype
    x, pts, nrm = np.asarray(x, np.float32).astype(T), np.asarray(points, np.float32).astype(T), np.asarray(normals, np.float32).astype(T)
    radius = T(np.float32(radius))
    h = radius * T(0.5)
    inv = T(1.0) / (h * h)
    r2 = radius * radius
    n = x.shape[0]
    num, den, smin = np.zeros(n, T), np.zeros(n, T), np.full(n, np.inf, T)
    for k in range(idx.shape[1]):
        p, m = pts[idx[:, k]], nrm[idx[:, k]]
        dx, dy, dz = x[:, 0] - p[:, 0], x[:, 1] - p[:, 1], x[:, 2] - p[:, 2]
        s = (dx * dx + dy * dy) + dz * dz
        c = (dx * m[:, 0] + dy * m[:, 1]) + dz * m[:, 2]
        w = np.exp(-(s * inv)).astype(T)
        num = num + w * c
        den = den + w
        smin = np.minimum(smin, s)
    defined = smin <= r2
    with np.errstate(invalid="ignore", divide="ignore"):
        value = np.where(defined, -(num / den), T(np.nan)).astype(T)
    return value, np.where(defined, den, T(0)).astype(T)


# ---------------------------------------------------------------------------------------------------------------- mesh rules
def spurious_vertices(verts_index, volume):
    """bool[V]: the volume at floor(c) or at ceil(c) is not finite"""
    c = np.asarray(verts_index, np.float32)
    hi = np.array(volume.shape) - 1
    lo_i = np.clip(np.floor(c).astype(np.int64), 0, hi)
    hi_i = np.clip(np.ceil(c).astype(np.int64), 0, hi)
    fin = np.isfinite(volume)
    return ~(fin[lo_i[:, 0], lo_i[:, 1], lo_i[:, 2]] & fin[hi_i[:, 0], hi_i[:, 1], hi_i[:, 2]])


def remove_vertices_by_mask(verts, faces, mask, *per_vertex, unreferenced=False):
    """masked vertices go, and every face naming one; unreferenced=True: then every vertex no surviving face names.  Order kept."""
    verts, faces, mask = np.asarray(verts), np.asarray(faces, np.int64).reshape(-1, 3), np.asarray(mask, bool)
    fkeep = ~mask[faces].any(axis=1)
    vkeep = ~mask
    if unreferenced:
        ref = np.zeros(verts.shape[0], bool)
        ref[faces[fkeep].reshape(-1)] = True
        vkeep = vkeep & ref
    new_id = np.cumsum(vkeep) - 1
    return (verts[vkeep], new_id[faces[fkeep]], *(np.asarray(a)[vkeep] for a in per_vertex))


def drop_spurious(verts_index, faces, volume):
    return remove_vertices_by_mask(verts_index, faces, spurious_vertices(verts_index, volume), unreferenced=True)


# ---------------------------------------------------------------------------------------------------------------- bricks
def n_bricks(n):
    return (n + BRICK - 1) // BRICK


def bricks_with_defined_point(volume):
    nb = tuple(n_bricks(n) for n in volume.shape)
    pad = np.zeros(tuple(b * BRICK for b in nb), bool)
    pad[:volume.shape[0], :volume.shape[1], :volume.shape[2]] = np.isfinite(volume)
    return pad.reshape(nb[0], BRICK, nb[1], BRICK, nb[2], BRICK).any(axis=(1, 3, 5))


def brick_box_rule(X, Y, Z, points, radius):
    """bool[nbx,nby,nbz]: a cloud point lies in the brick's in-grid point span grown by `radius` on every axis, in float64"""
    pts = np.asarray(points, np.float64)
    per_axis = []
    for a, ax in enumerate((X, Y, Z)):
        ax = np.asarray(ax, np.float64)
        b = np.arange(n_bricks(ax.size))
        lo, hi = ax[b * BRICK] - radius, ax[np.minimum(b * BRICK + BRICK - 1, ax.size - 1)] + radius
        per_axis.append((pts[:, a, None] >= lo[None, :]) & (pts[:, a, None] <= hi[None, :]))          # [N, nb_a]
    out = np.zeros(tuple(m.shape[1] for m in per_axis), bool)
    for s in range(0, pts.shape[0], 4096):
        mx, my, mz = (m[s:s + 4096] for m in per_axis)
        out |= np.einsum("ni,nj,nk->ijk", *(m.astype(np.int64) for m in (mx, my, mz))) > 0
    return out


# ---------------------------------------------------------------------------------------------------------------- outliers
def outlier_keep(mean_dist, std_ratio):
    m = np.asarray(mean_dist, np.float64)
    std = m.std(ddof=1) if m.size > 1 else 0.0
    return m <= m.mean() + std_ratio * std
