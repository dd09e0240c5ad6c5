"""GPU tests of the sparse density-grid sweep (csrc/sparse_sweep.hip, sugar_amd.extract.density_grid_sparse):

  * the brick mask against the float64 restatement tests/sparse_sweep_restatement.py: a superset of the bare rule (inflation 1.00), a
    subset of the rule at inflation 1.02 (the kernels use 1.01);
  * safety and exactness against the dense sweep `density_grid`: below the level in every inactive brick, bit-equal in every active
    brick, 0 elsewhere, and the same marching-cubes mesh bit for bit -- on the fixture's three grids, with `zero_inside`, for every
    `points_per_pass`, on a hand-made set of corner cases and on a 100 000-Gaussian bound scene at 128^3;
  * one device -> host read per call;
  * end to end: `extract_mesh_marching_cubes(..., sweep="sparse")` and `--sweep sparse` against `dense`."""
import functools
import os
import sys
import warnings

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sparse_sweep_restatement as ssr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K = 16
LEVELS = (0.3, 0.05)
FX = np.load(os.path.join(HERE, "golden", "sugar_mcgrid.npz"))
GRIDS = ssr.fixture_grids(FX)
GAUSSIANS = (FX["points"], FX["inv_scaled_rot"], FX["strengths"])


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


@functools.lru_cache(maxsize=None)
def _dense(grid, zero_inside=None):
    """the dense sweep over the fixture's Gaussians, computed once per (grid, box) and never written to"""
    from sugar_amd.extract import density_grid
    return density_grid(*_dev(*GRIDS[grid], *GAUSSIANS), K=K, zero_inside=zero_inside)


def _sparse(grid, level, **kw):
    from sugar_amd.extract import density_grid_sparse
    return density_grid_sparse(*_dev(*GRIDS[grid], *GAUSSIANS), level, K=K, return_active=True, **kw)


def _point_mask(mask, shape):
    m = mask.repeat_interleave(ssr.BRICK, 0).repeat_interleave(ssr.BRICK, 1).repeat_interleave(ssr.BRICK, 2)
    return m[:shape[0], :shape[1], :shape[2]]


def _assert_safe_and_exact(dense, sparse, mask, level):
    """the checks of the issue's test 2"""
    from sugar_amd.marching_cubes import marching_cubes
    assert sparse.shape == dense.shape and sparse.dtype == torch.float32
    assert mask.dtype == torch.bool and tuple(mask.shape) == tuple(ssr.n_bricks(n) for n in dense.shape)
    active = _point_mask(mask, dense.shape)
    assert bool((dense[~active] < level).all()), float(dense[~active].max())
    assert torch.equal(sparse[active], dense[active])
    assert bool((sparse[~active] == 0).all())
    sv, sf = marching_cubes(sparse, level)
    dv, df = marching_cubes(dense, level)
    assert torch.equal(sv, dv) and torch.equal(sf, df)
    return int(dv.shape[0])


def _assert_sandwich(mask, axes, gaussians, level, zero_inside=None):
    got = mask.cpu().numpy()
    lower = ssr.brick_mask(*axes, *gaussians, level, K=K, inflation=1.00, zero_inside=zero_inside)
    upper = ssr.brick_mask(*axes, *gaussians, level, K=K, inflation=1.02, zero_inside=zero_inside)
    assert got.shape == lower.shape
    assert not (lower & ~got).any(), "a brick of the bare rule is not active"
    assert not (got & ~upper).any(), "a brick beyond the rule at inflation 1.02 is active"
    return upper


# ------------------------------------------------------------------------------------------------ 1. the mask
@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("grid", list(GRIDS))
def test_brick_mask_lies_between_the_restatements(grid, level):
    _, mask = _sparse(grid, level)
    upper = _assert_sandwich(mask, GRIDS[grid], GAUSSIANS, level)
    print(f"{grid} level {level}: {int(mask.sum())} of {mask.numel()} bricks active (restatement at 1.02: {int(upper.sum())})")
    if grid == "wide40":
        assert mask.numel() == 125 and int(upper.sum()) <= 16 and int(mask.sum()) <= 16


# ------------------------------------------------------------------------------------------------ 2. safety and exactness
@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("grid", list(GRIDS))
def test_safe_and_exact_against_the_dense_sweep(grid, level):
    sparse, mask = _sparse(grid, level)
    assert _assert_safe_and_exact(_dense(grid), sparse, mask, level) > 0


# ------------------------------------------------------------------------------------------------ 3. zero_inside
@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("box", [(-0.5, 0.5), (-0.9, 0.9)])
def test_zero_inside(box, level):
    """On the 40^3 grid at +-3.6 a brick spans 7 x 0.185 = 1.29, so none fits into (-0.5, 0.5): that box changes the volume (partly covered
    bricks are blanked) but can drop no brick.  (-0.9, 0.9), the foreground box of a background pass over +-4 x 0.9, holds the central
    brick, which the blanking rule must drop."""
    sparse, mask = _sparse("wide40", level, zero_inside=box)
    _assert_sandwich(mask, GRIDS["wide40"], GAUSSIANS, level, zero_inside=box)
    dense = _dense("wide40", box)
    _assert_safe_and_exact(dense, sparse, mask, level)
    assert not torch.equal(dense, _dense("wide40"))
    _, mask_no_box = _sparse("wide40", level)
    assert not bool((mask & ~mask_no_box).any())
    if box == (-0.9, 0.9):
        assert not torch.equal(mask, mask_no_box) and bool(mask_no_box[2, 2, 2]) and not bool(mask[2, 2, 2])
    else:
        assert torch.equal(mask, mask_no_box)


# ------------------------------------------------------------------------------------------------ 4. points_per_pass, repeatability
def test_result_does_not_depend_on_points_per_pass():
    """37 x 29 x 43: partial bricks on every axis; chunks of 1 brick (1, 511, 513 points per pass) and of 13 bricks (7001)"""
    ref, ref_mask = _sparse("box37x29x43", 0.3)
    again, again_mask = _sparse("box37x29x43", 0.3)
    assert torch.equal(ref, again) and torch.equal(ref_mask, again_mask)
    for ppp in (1, 511, 513, 7001):
        vol, mask = _sparse("box37x29x43", 0.3, points_per_pass=ppp)
        assert torch.equal(vol, ref) and torch.equal(mask, ref_mask), ppp


# ------------------------------------------------------------------------------------------------ 5. corners of the rule
CORNER_LEVEL = 0.3
SIGMA_CLAMP = 1e-8


def _corner_axes():
    return (np.linspace(-1.0, 1.0, 21).astype(np.float32), np.linspace(-0.9, 0.9, 19).astype(np.float32),
            np.linspace(-1.1, 1.1, 23).astype(np.float32))                     # spacing 0.1 on every axis; 3 x 3 x 3 bricks, all edge bricks partial


def _corner_gaussians(with_covering):
    """(centers[P,3], B[P,3,3], strengths[P]) float32 and the row of each named case"""
    X, Y, Z = _corner_axes()
    rows, names = [], {}
    eye = np.eye(3)
    c45 = np.sqrt(0.5)
    rot45 = np.array([[1.0, 0.0, 0.0], [0.0, c45, -c45], [0.0, c45, c45]])     # about x: the thin axis (column 2) becomes (0, -s, c)

    def add(name, centre, R, sigma, s):
        names[name] = len(rows)
        rows.append((np.asarray(centre, np.float64), R @ np.diag(1.0 / np.maximum(np.asarray(sigma, np.float64), SIGMA_CLAMP)), s))

    add("outside_box_enters", (1.3, 0.0, 0.0), eye, (0.12, 0.12, 0.12), 0.9)        # reach 3.05 x 0.12 = 0.37: down to x = 0.93
    add("outside_box_stays_out", (0.0, 3.0, 0.0), eye, (0.05, 0.05, 0.05), 0.9)
    add("too_weak", (-0.5, -0.5, -0.6), eye, (0.1, 0.1, 0.1), CORNER_LEVEL / (2 * K) * 0.96)   # 2 K s <= level
    add("no_grid_point_in_box", (0.2, 0.2, 1.25), eye, (0.01, 0.01, 0.01), 0.9)     # z range [1.15, 1.35]: beyond Z[-1] = 1.1
    plane_z = float(Z[12])                                                           # a grid plane, 0.1 in float32
    for i, (tag, off) in enumerate((("on", 0.0), ("1e-7", 1e-7), ("1e-5", 1e-5))):
        add(f"flat_aligned_{tag}", (-0.6 + 0.5 * i, 0.3, plane_z + off), eye, (0.12, 0.12, SIGMA_CLAMP), 0.95)
    for i, (tag, off) in enumerate((("on", 0.0), ("1e-7", 1e-7), ("1e-5", 1e-5))):
        n = rot45[:, 2]                                                              # centre on a grid point, moved along the normal
        centre = np.array([float(X[4 + 6 * i]), float(Y[5]), float(Z[6])]) + off * n
        add(f"flat_rotated_{tag}", centre, rot45, (0.12, 0.12, SIGMA_CLAMP), 0.95)
    g = np.random.default_rng(11)
    for i in range(8):                                                               # ordinary Gaussians: P >= K without the covering one
        q = g.standard_normal(4); q /= np.linalg.norm(q)
        w, x, y, z = q
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                      [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                      [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        centre = np.append(g.uniform(-0.8, 0.8, 2), g.uniform(-0.8, 0.0))            # below z = 0.4: the top layer of bricks stays out of reach
        add(f"ordinary_{i}", centre, R, g.uniform(0.04, 0.12, 3), g.uniform(0.3, 1.0))
    if with_covering:
        add("covers_the_grid", (0.1, 0.0, -0.1), eye, (2.0, 2.0, 2.0), 0.02)         # 2 K s = 0.64 > level; reach 1.23 x 2.0 on every axis
    centers = np.stack([r[0] for r in rows]).astype(np.float32)
    B = np.stack([r[1] for r in rows]).astype(np.float32)
    s = np.array([r[2] for r in rows], dtype=np.float32)
    return centers, B, s, names


@pytest.mark.parametrize("with_covering", [False, True], ids=["partial", "covering"])
def test_corners_of_the_rule(with_covering):
    from sugar_amd.extract import density_grid, density_grid_sparse
    axes = _corner_axes()
    centers, B, s, names = _corner_gaussians(with_covering)
    assert centers.shape[0] >= K and [a.size for a in axes] == [21, 19, 23]
    args = _dev(*axes, centers, B, s)
    dense = density_grid(*args, K=K)
    sparse, mask = density_grid_sparse(*args, CORNER_LEVEL, K=K, return_active=True)
    n_verts = _assert_safe_and_exact(dense, sparse, mask, CORNER_LEVEL)
    assert n_verts > 0
    _assert_sandwich(mask, axes, (centers, B, s), CORNER_LEVEL)
    lo, hi = ssr.gaussian_index_boxes(*axes, centers, B, s, CORNER_LEVEL, K=K)
    marks = hi[:, 0] >= lo[:, 0]
    assert marks[names["outside_box_enters"]]
    for name in ("outside_box_stays_out", "too_weak", "no_grid_point_in_box"):
        assert not marks[names[name]], name
    if with_covering:
        assert bool(mask.all()) and mask.numel() == 27                              # 27 bricks > 8: the workgroup-per-Gaussian launch
    else:
        assert not bool(mask[:, :, 2].any()) and bool(mask[:, :, :2].any())       # no box reaches the points 16 .. 22 of z
        alone = np.zeros(len(s), dtype=bool); alone[names["outside_box_enters"]] = True
        only = ssr.brick_mask(*axes, centers[alone], B[alone], s[alone], CORNER_LEVEL, K=K, inflation=1.0)
        assert only.any() and bool(mask[torch.from_numpy(only).to(DEV)].all())


# ------------------------------------------------------------------------------------------------ 6. nothing active
def test_nothing_active():
    from sugar_amd.extract import density_grid_sparse, extract_mesh_marching_cubes
    from sugar_amd.marching_cubes import marching_cubes
    level = 0.3
    weak = np.full_like(FX["strengths"], level / (4 * K))
    vol, mask = density_grid_sparse(*_dev(*GRIDS["fixture40"], FX["points"], FX["inv_scaled_rot"], weak), level, K=K, return_active=True)
    assert vol.shape == (40, 40, 40) and not bool(vol.any()) and not bool(mask.any())
    verts, faces = marching_cubes(vol, level)
    assert verts.shape == (0, 3) and faces.shape == (0, 3)
    m = _fixture_model()
    mesh = extract_mesh_marching_cubes(m["points"], m["scales"], m["quats"], torch.full_like(m["opacities"], level / (4 * K)), m["sh_dc"],
                                       extent=0.9, resolution=24, level=level, sweep="sparse", return_stats=True)
    assert mesh["verts"].shape == (0, 3) and mesh["faces"].shape == (0, 3) and mesh["active_bricks"] == [0, 0]


# ------------------------------------------------------------------------------------------------ 7. synchronisation
def _count_syncs(fn):
    """how many synchronising operations torch reports while fn runs"""
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            out = fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    return sum("called a synchronizing" in str(w.message) for w in seen), out


def test_one_device_to_host_read_per_call():
    from sugar_amd.extract import density_grid_sparse
    args = _dev(*GRIDS["wide40"], *GAUSSIANS)
    density_grid_sparse(*args, 0.3, points_per_pass=1500); torch.cuda.synchronize()      # (warm: code objects, the allocator)
    probe = torch.zeros(4, dtype=torch.int32, device=DEV)
    assert _count_syncs(lambda: probe.tolist())[0] == 1                                  # (the counter sees a read, and counts it once)
    n, (vol, mask) = _count_syncs(lambda: density_grid_sparse(*args, 0.3, points_per_pass=1500, zero_inside=(-0.9, 0.9), return_active=True))
    assert n == 1, f"{n} synchronising operations"
    assert int(mask.sum()) > 3                                                           # several chunks of 2 bricks ran in there
    weak = torch.full_like(args[5], 0.3 / (4 * K))
    n, _ = _count_syncs(lambda: density_grid_sparse(*args[:5], weak, 0.3))               # nothing active: still the one read
    assert n == 1


def test_non_ascending_axis_on_the_device_raises():
    from sugar_amd.extract import density_grid_sparse
    args = _dev(*GRIDS["fixture40"], *GAUSSIANS)
    bad = args[1].clone(); bad[20] = bad[19]
    with pytest.raises(ValueError, match="strictly ascending"):
        density_grid_sparse(args[0], bad, args[2], *args[3:], 0.3)


# ------------------------------------------------------------------------------------------------ 8. end to end
@functools.lru_cache(maxsize=None)
def _fixture_model():
    """the fixture's Gaussians as a model: scales and quaternions recovered from inv_scaled_rot = R diag(1 / sigma)"""
    from scipy.spatial.transform import Rotation
    B = FX["inv_scaled_rot"].astype(np.float64)
    norms = np.linalg.norm(B, axis=1)                                   # |column i| = 1 / sigma_i
    R = B / norms[:, None, :]
    q = Rotation.from_matrix(R).as_quat()                               # (x, y, z, w)
    quats = np.concatenate([q[:, 3:], q[:, :3]], axis=1).astype(np.float32)
    pts, scales, quats, opac, dc = _dev(FX["points"], (1.0 / norms).astype(np.float32), quats, FX["strengths"], FX["sh_dc"])
    return dict(points=pts, scales=scales, quats=quats, opacities=opac, sh_dc=dc)


@pytest.mark.parametrize("background", [False, True])
def test_extraction_end_to_end(background):
    from sugar_amd.extract import extract_mesh_marching_cubes
    m = _fixture_model()
    run = lambda **kw: extract_mesh_marching_cubes(m["points"], m["scales"], m["quats"], m["opacities"], m["sh_dc"], extent=0.9,
                                                   resolution=48, level=0.3, background=background, **kw)
    dense = run(sweep="dense")
    sparse = run(sweep="sparse")
    assert sorted(dense) == sorted(sparse) == ["colors", "faces", "normals", "verts"]
    assert dense["verts"].shape[0] > 100 and dense["faces"].shape[0] > 100
    for k in dense:
        assert torch.equal(dense[k], sparse[k]), k
    stats = run(sweep="sparse", return_stats=True)
    passes = 2 if background else 1
    assert stats["total_bricks"] == [216] * passes and len(stats["active_bricks"]) == passes
    assert all(0 < a <= 216 for a in stats["active_bricks"])
    if background:
        assert stats["active_bricks"][1] < 216 // 4
    assert run(sweep="dense", return_stats=True)["active_bricks"] == [216] * passes


def test_command_line_writes_the_same_ply(tmp_path, capsys):
    from sugar_amd import extract, io
    m = _fixture_model()
    P = m["points"].shape[0]
    feats = torch.zeros(P, 16, 3, device=DEV); feats[:, 0] = m["sh_dc"]
    cloud = str(tmp_path / "point_cloud.ply")
    io.save_gaussian_ply(cloud, m["points"], feats, torch.logit(m["opacities"]).reshape(P, 1), torch.log(m["scales"]), m["quats"])
    outs = {}
    for sweep in ("dense", "sparse"):
        out = str(tmp_path / f"{sweep}.ply")
        assert extract.main([cloud, "--out", out, "--resolution", "48", "--level", "0.3", "--extent", "0.9", "--sweep", sweep]) == 0
        outs[sweep] = (open(out, "rb").read(), capsys.readouterr().out)
    assert len(outs["dense"][0]) > 10000 and outs["dense"][0] == outs["sparse"][0]
    assert "bricks active" in outs["sparse"][1] and "bricks active" not in outs["dense"][1]


# ------------------------------------------------------------------------------------------------ 9. mid-size
def test_bound_scene_at_128(record_property):
    """128^3 over make_bound_scene(100 000): flat Gaussians, 3.3e-6 thick against a spacing of 0.05.  Foreground only."""
    from sugar_amd import field, synthetic as syn
    from sugar_amd.extract import density_grid, density_grid_sparse
    sc = syn.make_bound_scene(100_000, 7, opaque=True).scene
    pts = sc.means3D.to(DEV).contiguous()
    B = field.scaled_rotation(sc.rotations.to(DEV), sc.scales.to(DEV), True)
    st = sc.opacities.to(DEV).reshape(-1)
    extent = float(pts.abs().max()) * 1.05
    X = torch.linspace(-1, 1, 128, device=DEV) * extent
    dense = density_grid(X, X, X, pts, B, st, K=K)
    for level in LEVELS:
        sparse, mask = density_grid_sparse(X, X, X, pts, B, st, level, K=K, return_active=True)
        _assert_safe_and_exact(dense, sparse, mask, level)
        frac = float(mask.float().mean())
        print(f"bound scene, 128^3, level {level}: {int(mask.sum())} of {mask.numel()} bricks active ({100 * frac:.1f} %)")
        record_property(f"active_brick_fraction_level_{level}", frac)
