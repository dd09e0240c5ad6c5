"""The activation rule of the sparse density-grid sweep (csrc/sparse_sweep.hip, sugar_amd.extract.density_grid_sparse), restated in
float64 numpy: inputs -> the bool brick mask [nbx, nby, nbz].  Not a test module; tests/test_sparse_sweep_cpu.py and
tests/test_gpu_sparse_sweep.py import it.

The rule.  density(x) = sum over the K nearest Gaussians of s_k exp(-0.5 clamp(|B_k^T (x - c_k)|^2, 0, 1e8)).  If
density(x) >= level, one of the K terms is >= level / K, so |B_g^T (x - c_g)|^2 <= 2 ln(K s_g / level) for some Gaussian g.  With a
margin for float32 arithmetic the radius is m_g = sqrt(2 ln(2 K s_g / level)), and g reaches only if 2 K s_g > level.  The ellipsoid
{Mahalanobis <= m_g} lies in the axis-aligned box of half-extent m_g sqrt(S_aa), S_aa = sum_i B_ai^2 sigma_i^4 with
sigma_i = 1 / |column i of B_g| (B = R diag(1 / sigma) has orthogonal columns).  Per reaching Gaussian and axis:
    e_a = max(inflation * m_g * sqrt(S_aa), gap_a)        gap_a: the largest spacing between consecutive points of the axis
    [i0, i1] = the indices of the grid points inside [c_a - e_a, c_a + e_a]; empty on any axis: the Gaussian marks nothing
    otherwise [i0 - 1, i1 + 1] clipped to the grid (the six-neighbour dilation), and every 8 x 8 x 8-point brick it touches is active.
With zero_inside = (lo, hi), every brick all of whose in-grid points are strictly inside the box (compared in float32, as the dense
sweep's blanking compares them) is dropped.  The kernels use inflation = 1.01."""
import numpy as np

BRICK = 8
INFLATION = 1.01


def n_bricks(n):
    return (int(n) + BRICK - 1) // BRICK


def gaussian_index_boxes(X, Y, Z, centers, inv_scaled_rot, strengths, level, K=16, inflation=INFLATION):
    """(lo[P,3], hi[P,3]) int64: the dilated, clipped index box of every Gaussian, hi < lo on axis 0 where it marks nothing"""
    axes = [np.asarray(a, dtype=np.float64).reshape(-1) for a in (X, Y, Z)]
    c = np.asarray(centers, dtype=np.float64).reshape(-1, 3)
    B = np.asarray(inv_scaled_rot, dtype=np.float64).reshape(-1, 3, 3)
    s = np.asarray(strengths, dtype=np.float64).reshape(-1)
    P = c.shape[0]
    level = float(level)
    reach = 2.0 * K * s
    reaches = reach > level
    m = np.sqrt(2.0 * np.log(np.where(reaches, reach, level) / level))
    n2 = (B * B).sum(axis=1)                                   # |column i|^2, [P, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        S = ((B * B) / (n2 * n2)[:, None, :]).sum(axis=2)      # S_aa, [P, 3]
    lo = np.zeros((P, 3), dtype=np.int64)
    hi = np.full((P, 3), -1, dtype=np.int64)
    ok = reaches.copy()
    for a, ax in enumerate(axes):
        gap = float(np.max(np.diff(ax))) if ax.size > 1 else 0.0
        e = np.fmax(inflation * m * np.sqrt(S[:, a]), gap)
        i0 = np.searchsorted(ax, c[:, a] - e, side="left")
        i1 = np.searchsorted(ax, c[:, a] + e, side="right") - 1
        ok &= i1 >= i0
        lo[:, a] = np.maximum(i0 - 1, 0)
        hi[:, a] = np.minimum(i1 + 1, ax.size - 1)
    lo[~ok] = 0
    hi[~ok] = -1
    return lo, hi


def brick_mask(X, Y, Z, centers, inv_scaled_rot, strengths, level, K=16, inflation=INFLATION, zero_inside=None):
    """bool [nbx, nby, nbz]: the active bricks"""
    axes = [np.asarray(a).reshape(-1) for a in (X, Y, Z)]
    nb = [n_bricks(a.size) for a in axes]
    lo, hi = gaussian_index_boxes(X, Y, Z, centers, inv_scaled_rot, strengths, level, K, inflation)
    keep = hi[:, 0] >= lo[:, 0]
    boxes = np.unique(np.concatenate([lo[keep] // BRICK, hi[keep] // BRICK], axis=1), axis=0)
    mask = np.zeros(nb, dtype=bool)
    for b in boxes:
        mask[b[0]:b[3] + 1, b[1]:b[4] + 1, b[2]:b[5] + 1] = True
    if zero_inside is not None:
        lo32, hi32 = np.float32(zero_inside[0]), np.float32(zero_inside[1])
        inside = []
        for a, n in zip(axes, nb):
            a32 = a.astype(np.float32)
            first = a32[np.arange(n) * BRICK]
            last = a32[np.minimum(np.arange(n) * BRICK + BRICK - 1, a.size - 1)]
            inside.append((first > lo32) & (last < hi32))
        mask &= ~(inside[0][:, None, None] & inside[1][None, :, None] & inside[2][None, None, :])
    return mask


def point_mask(mask, shape):
    """the brick mask expanded to the grid points, bool [nx, ny, nz]"""
    m = np.repeat(np.repeat(np.repeat(mask, BRICK, axis=0), BRICK, axis=1), BRICK, axis=2)
    return m[:shape[0], :shape[1], :shape[2]]


def needed_points(density, level):
    """bool [nx, ny, nz]: the inside points (finite and >= level) and their six grid neighbours"""
    inside = np.isfinite(density) & (density >= level)
    need = inside.copy()
    for a in range(3):
        sl_lo = [slice(None)] * 3; sl_hi = [slice(None)] * 3
        sl_lo[a] = slice(0, -1); sl_hi[a] = slice(1, None)
        need[tuple(sl_lo)] |= inside[tuple(sl_hi)]
        need[tuple(sl_hi)] |= inside[tuple(sl_lo)]
    return need


def density_float64(X, Y, Z, centers, inv_scaled_rot, strengths, K=16):
    """the dense sweep's density in float64, the K nearest Gaussians from scipy's k-d tree; [nx, ny, nz]"""
    from scipy.spatial import cKDTree
    axes = [np.asarray(a, dtype=np.float64).reshape(-1) for a in (X, Y, Z)]
    c = np.asarray(centers, dtype=np.float64).reshape(-1, 3)
    B = np.asarray(inv_scaled_rot, dtype=np.float64).reshape(-1, 3, 3)
    s = np.asarray(strengths, dtype=np.float64).reshape(-1)
    pts = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 3)
    _, idx = cKDTree(c).query(pts, k=K)
    idx = idx.reshape(pts.shape[0], K)
    d = pts[:, None, :] - c[idx]                               # [N, K, 3]
    w = np.einsum("nkij,nki->nkj", B[idx], d)                  # B^T d
    q = np.clip((w * w).sum(-1), 0.0, 1e8)
    return (s[idx] * np.exp(-0.5 * q)).sum(-1).reshape([a.size for a in axes])


def fixture_grids(fx):
    """the three grids of the tests over tests/golden/sugar_mcgrid.npz (float32 axes): the fixture's own 40^3 at +-0.9, a 40^3 at +-3.6
    (the background pass's proportions: most bricks are out of every Gaussian's reach), and a 37 x 29 x 43 box with three different,
    non-uniform, strictly ascending axes"""
    def warped(lo, hi, n, power):
        u = np.linspace(-1.0, 1.0, n)
        w = np.sign(u) * np.abs(u) ** power                                   # strictly ascending, spacing varies along the axis
        return (lo + (w + 1.0) * 0.5 * (hi - lo)).astype(np.float32)
    wide = np.linspace(-3.6, 3.6, 40).astype(np.float32)
    return {
        "fixture40": (fx["X"], fx["Y"], fx["Z"]),
        "wide40": (wide, wide, wide),
        "box37x29x43": (warped(-0.9, 0.9, 37, 1.3), warped(-0.7, 0.8, 29, 1.0) + np.float32(0.003) * np.sin(np.arange(29, dtype=np.float32)),
                        warped(-1.0, 0.85, 43, 0.8)),
    }
