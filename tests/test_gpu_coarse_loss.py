"""GPU parity of the coarse trainers' inline loss terms (sugar_amd.coarse_loss over csrc/coarse_loss.hip).

  * the three operations against tests/golden/coarse_loss.npz, which the reference's own model wrote: an array within 4 x its `yard_*`
    (the distance of the float32 trainer statements from the same statements in float64), floor 1e-7 norm-wise -- the bar of
    tests/test_gpu_sdf_regulariser.py; a scalar mean within max(4 x yard, 2 float32 ulp); M and the band mask exactly.
  * shapes beyond the fixture against the float64 restatement (tests/coarse_loss_restatement.py) computed here, the yard computed here
    from the restatement's float32 run: N = 1 in front of and behind znear (M = 0), N = 257, K = 8, 4 097 samples of one Gaussian, a
    16 x 16 depth map with lookup points on pixel centres and on the border, a contiguous map and the stride-3 view (equal bits), a
    depth map that does not require grad.
  * constructed kinks with exactly representable values: orthogonal axis-aligned normals (sign = 0), an all-zero opacity row, a
    min_scaling below 1e-6, samples at and beyond clamp_max, est = 0.
  * both estimation modes, the squared switches, the std normalisation and through_normal_only both ways (the fixture's variants);
    unreferenced Gaussians exactly zero; out-of-range neighbour indices contribute nothing; every output bit-identical between two
    runs, except the depth map's gradient; no operation synchronises with the host.
  * the composite on tests/sugar_regulariser_standin.make_module() under a fixed seed against the restatement on the same stand-in and
    seed, with `install_row_gathers` on and off.
Each check prints its distance, its bar and its ratio to the yard."""
import os
import sys

import numpy as np
import pytest
import torch

from sugar_amd import coarse_loss, shims, synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
FX = np.load(os.path.join(HERE, "golden", "coarse_loss.npz"))
FIELD_FX = np.load(os.path.join(HERE, "golden", "sugar_field.npz"))
REG_FX = np.load(os.path.join(HERE, "golden", "sdf_regulariser.npz"))
FLOOR = 1e-7
TWO_ULP = 2.0 * 2.0 ** -23

from tests import coarse_loss_restatement as cl  # noqa: E402
from tests import sdf_regulariser_restatement as rs  # noqa: E402
from tests.golden.make_coarse_loss import EST_VARIANTS, SURFACE_WEIGHT, estimation_inputs  # noqa: E402


def _t(k, fx=FX):
    return torch.as_tensor(fx[k])


def _check(what, got, want, yard):
    """an array within max(4 yard, FLOOR) norm-wise, a scalar within max(4 yard, 2 ulp) relative"""
    got, want = torch.as_tensor(got).detach().cpu(), torch.as_tensor(want).detach().cpu()
    scalar = want.dim() == 0
    d = cl.scalar_distance(got, want) if scalar else rs.distance(got, want)
    bar = max(4.0 * float(yard), TWO_ULP if scalar else FLOOR)
    print(f"{what:52s} distance {d:.3e}   bar {bar:.3e}   yard {float(yard):.3e}   ratio-to-yard {d / max(float(yard), 1e-30):.2f}")
    assert torch.isfinite(got).all(), what
    assert d <= bar, (what, d, bar)


def _stride3(depth_hw, grad=True):
    image = depth_hw[..., None].repeat(1, 1, 3).contiguous().to(DEV).requires_grad_(grad)      # an [H,W,3] render
    return image, image[..., 0]


CAM = dict(world_to_view=_t("cam_world_to_view"), projection=_t("depth_projection", REG_FX), znear=_t("znear"))
EXTENT = float(FX["extent"])
STATE = dict(points=_t("state_points", FIELD_FX), scaling=torch.exp(_t("state_scales", FIELD_FX)),
             quaternions=torch.nn.functional.normalize(_t("state_quaternions", FIELD_FX), dim=-1), knn_idx=_t("state_knn_idx", FIELD_FX),
             normals=_t("normals_out", REG_FX))


# ---------------------------------------------------------------------------------------------------------------- surface band
def test_surface_band_matches_the_fixture():
    args = [STATE[k].to(DEV) for k in ("points", "quaternions", "scaling")] + [CAM["world_to_view"].to(DEV), _t("cam_center").to(DEV),
                                                                               CAM["projection"].to(DEV)]
    _, depth = _stride3(_t("depth_map", REG_FX), grad=False)
    close, std = coarse_loss.surface_band(*args, depth, float(FX["band_threshold"]))
    assert close.dtype == torch.bool and close.shape == std.shape == (2500,) and not std.requires_grad
    assert torch.equal(close.cpu(), _t("band_close"))
    _check("band_std", std, FX["band_std"], FX["yard_band_std"])
    again = coarse_loss.surface_band(*args, depth, float(FX["band_threshold"]))
    flat = coarse_loss.surface_band(*args, _t("depth_map", REG_FX).to(DEV), float(FX["band_threshold"]))   # the contiguous map
    for other in (again, flat):
        assert torch.equal(other[0], close) and torch.equal(other[1], std)


# ----------------------------------------------------------------------------------------------------------- estimation losses
def _est_call(x, sdf, density, beta, idx, depth, opts, std=None, cam=CAM, extent=EXTENT, grads=True):
    """the operation on device copies of the inputs; returns (est, surf, M, {gradients})"""
    opts = dict(opts)
    by_std = opts.pop("by_std", False)
    leaves = [t.to(DEV).clone().requires_grad_(grads) for t in (x, sdf, density, beta)]
    est, surf, M = coarse_loss.estimation_losses(
        leaves[0], depth, cam["world_to_view"].to(DEV), cam["projection"].to(DEV), cam["znear"].to(DEV), sdf=leaves[1], density=leaves[2],
        beta=leaves[3], scale=None if by_std else extent / 10., std=std.to(DEV) if by_std else None, sample_idx=idx.to(DEV),
        clamp_max=10. * extent, **opts)
    g = {}
    if grads:
        (est + SURFACE_WEIGHT * surf if surf is not None else est).backward()
        field = leaves[1] if opts["mode"] == "sdf" else leaves[2]
        g = dict(grad_samples=leaves[0].grad, grad_field=field.grad, grad_beta=leaves[3].grad if opts["mode"] == "density" else None)
    return est, surf, M, g


def _est_restated(x, sdf, density, beta, idx, dmap, opts, dtype, std=None, cam=CAM, extent=EXTENT):
    """the restatement on the CPU in `dtype`, through the stride-3 view"""
    opts = dict(opts)
    by_std = opts.pop("by_std", False)
    image = dmap.to(dtype)[..., None].repeat(1, 1, 3).contiguous().requires_grad_(True)
    leaves = [t.to(dtype).clone().requires_grad_(True) for t in (x, sdf, density, beta)]
    est, surf, M = cl.estimation_losses(leaves[0], image[..., 0], cam["world_to_view"], cam["projection"], cam["znear"].to(dtype), sdf=leaves[1],
                                        density=leaves[2], beta=leaves[3], scale=None if by_std else extent / 10.,
                                        std=std.to(dtype) if by_std else None, sample_idx=idx, clamp_max=10. * extent, **opts)
    total = est + SURFACE_WEIGHT * surf if surf is not None else est
    if int(M) > 0:
        total.backward()
    zero = lambda t: t.grad if t.grad is not None else torch.zeros_like(t)
    field = leaves[1] if opts["mode"] == "sdf" else leaves[2]
    return est, surf, M, dict(grad_samples=zero(leaves[0]), grad_field=zero(field),
                              grad_beta=zero(leaves[3]) if opts["mode"] == "density" else None, grad_depth=zero(image)[..., 0])


@pytest.mark.parametrize("tag", list(EST_VARIANTS))
def test_estimation_losses_match_the_fixture(tag):
    x, idx, sdf, density, beta = estimation_inputs(FX)
    std = _t("band_std")
    runs = []
    for view in ("stride3", "stride3", "contiguous", "no_grad"):
        if view == "contiguous":
            image = _t("depth_map", REG_FX).to(DEV).requires_grad_(True)
            depth = image
        else:
            image, depth = _stride3(_t("depth_map", REG_FX), grad=view != "no_grad")
        est, surf, M, g = _est_call(x, sdf, density, beta, idx, depth, EST_VARIANTS[tag], std=std)
        g["grad_depth"] = None if image.grad is None else (image.grad[..., 0] if view != "contiguous" else image.grad)
        if view == "stride3":
            assert not image.grad[..., 1:].any()
        runs.append((est, surf, M, g))
    est, surf, M, g = runs[0]
    assert M.dtype == torch.int64 and M.dim() == 0 and int(M) == int(FX[tag + "_M"]) == 6000
    assert est.dim() == 0 and est.device.type == "cuda"
    _check(tag + "_loss_est", est, FX[tag + "_loss_est"], FX["yard_" + tag + "_loss_est"])
    if surf is not None:
        _check(tag + "_loss_surf", surf, FX[tag + "_loss_surf"], FX["yard_" + tag + "_loss_surf"])
    for k, v in g.items():
        if v is not None:
            _check(f"{tag}_{k}", v, FX[f"{tag}_{k}"], FX[f"yard_{tag}_{k}"])
    assert not g["grad_samples"][6000:].any() and not g["grad_field"][6000:].any()       # the band behind znear: exactly zero
    # bit-identical between two runs, between the stride-3 view and the contiguous map, and without a gradient on the depth map;
    # the depth map's own gradient (float atomics) is exempt
    assert runs[3][3]["grad_depth"] is None
    for other in runs[1:]:
        assert torch.equal(other[0], est) and torch.equal(other[2], M) and (surf is None or torch.equal(other[1], surf))
        for k in ("grad_samples", "grad_field", "grad_beta"):
            assert g[k] is None or torch.equal(other[3][k], g[k]), k
    _check(tag + "_grad_depth (contiguous map)", runs[2][3]["grad_depth"], FX[tag + "_grad_depth"], FX["yard_" + tag + "_grad_depth"])


def _est_case(what, x, sdf, density, beta, idx, dmap, opts, std=None, cam=CAM, extent=EXTENT):
    """the operation against the float64 restatement computed here; yards from the restatement's float32 run"""
    want = _est_restated(x, sdf, density, beta, idx, dmap, opts, torch.float64, std, cam, extent)
    f32 = _est_restated(x, sdf, density, beta, idx, dmap, opts, torch.float32, std, cam, extent)
    image, depth = _stride3(dmap)
    est, surf, M, g = _est_call(x, sdf, density, beta, idx, depth, opts, std, cam, extent)
    g["grad_depth"] = image.grad[..., 0]
    assert int(M) == int(want[2]) == int(f32[2])
    if int(M) == 0:                                                            # torch's mean of an empty tensor; nothing flows back
        assert torch.isnan(est) and (surf is None or torch.isnan(surf)) and torch.isnan(want[0])
        assert all(v is None or not v.any() for v in g.values())
        return est, surf, M, g
    for i, name in ((0, "loss_est"), (1, "loss_surf")):
        if want[i] is not None:
            _check(f"{what} {name}", (est, surf)[i], want[i], cl.scalar_distance(f32[i], want[i]))
    for k, v in g.items():
        if v is not None:
            _check(f"{what} {k}", v, want[3][k], rs.distance(f32[3][k], want[3][k]))
    return est, surf, M, g


@pytest.mark.parametrize("n", [1, 257])
@pytest.mark.parametrize("tag", ["est_sdf", "est_den_sq"])
def test_estimation_losses_small_n(tag, n):
    x, idx, sdf, density, beta = (t[:n] for t in estimation_inputs(FX))
    _est_case(f"{tag} n={n}", x, sdf, density, beta, idx, _t("depth_map", REG_FX), EST_VARIANTS[tag])


def test_estimation_losses_one_sample_behind_znear():
    x, idx, sdf, density, beta = (t[6000:6001] for t in estimation_inputs(FX))
    for tag in ("est_sdf", "est_den"):
        _, _, M, _ = _est_case(f"{tag} behind", x, sdf, density, beta, idx, _t("depth_map", REG_FX), EST_VARIANTS[tag])
        assert int(M) == 0


EYE_CAM = dict(world_to_view=torch.eye(4)[None], projection=torch.eye(4)[None], znear=torch.tensor([0.5]))


def test_estimation_losses_on_pixel_centres_and_on_the_border():
    """a 16 x 16 map under identity matrices (z = the sample's own z, ndc = its x, y): pixel k's centre is x = 1 - (2 k + 1) / 16,
    exact in float32 -- points exactly on pixel centres, on the border (where the clamp is active and the coordinate's gradient is
    zero) and beyond it"""
    S = 16
    centre = lambda k: 1.0 - (2.0 * k + 1.0) / S
    ks = [0.0, 1.0, 7.0, 14.0, 15.0, -0.5, 15.5, -3.0, 20.0, 3.5, 6.25]
    xy = torch.tensor([[centre(a), centre(b)] for a in ks for b in ks], dtype=torch.float32)
    g = torch.Generator().manual_seed(9)
    x = torch.cat((xy, 1.0 + torch.rand(len(xy), 1, generator=g)), 1)
    dmap = torch.rand(S, S, generator=g) + 1.25
    n = len(x)
    sdf, density, beta = torch.rand(n, generator=g), torch.rand(n, generator=g) * 0.9, torch.rand(n, generator=g) * 0.2 + 0.3
    idx = torch.zeros(n, dtype=torch.int64)
    for tag in ("est_sdf", "est_den"):
        _, _, M, got = _est_case(f"{tag} 16x16", x, sdf, density, beta, idx, dmap, EST_VARIANTS[tag], cam=EYE_CAM, extent=1.0)
        assert int(M) == n
    clamped_x = torch.tensor([[a <= 0 or a >= 15 for b in ks] for a in ks]).flatten()
    clamped_y = torch.tensor([[b <= 0 or b >= 15 for b in ks] for a in ks]).flatten()
    gx = got["grad_samples"].cpu()
    assert not gx[clamped_x, 0].any() and not gx[clamped_y, 1].any() and gx[~clamped_x, 0].abs().min() > 0


def test_estimation_kinks_with_exact_values():
    """a constant map of 3 under identity matrices, scale 1, clamp_max 2: est = 3 - z exactly.
         sample 0: z = 2, sdf = 3     -> |sdf - |est|| / s = 2 = clamp_max: the gradient passes (x <= c)
         sample 1: z = 2, sdf = 3.5   -> 2.5 beyond clamp_max: zero gradient, the term counts as 2
         sample 2: z = 3, sdf = 0.5   -> est = 0: sign(0) = 0, nothing reaches the sample through |est|
         sample 3: z = 1, sdf = 2     -> sdf - |est| = 0: d|x|/dx = 0 at 0
         sample 4: z = 0.25           -> behind znear = 0.5"""
    x = torch.tensor([[0.0, 0.0, 2.0], [0.25, 0.0, 2.0], [0.0, 0.25, 3.0], [-0.25, 0.0, 1.0], [0.0, 0.0, 0.25]])
    sdf = torch.tensor([3.0, 3.5, 0.5, 2.0, 9.0])
    n = len(x)
    image, depth = _stride3(torch.full((16, 16), 3.0))
    leaves = [x.to(DEV).requires_grad_(True), sdf.to(DEV).requires_grad_(True)]
    est, surf, M = coarse_loss.estimation_losses(leaves[0], depth, EYE_CAM["world_to_view"].to(DEV), EYE_CAM["projection"].to(DEV), 0.5,
                                                 sdf=leaves[1], scale=1.0, clamp_max=2.0, with_surface=True)
    assert int(M) == 4
    assert float(est) == (2.0 + 2.0 + 0.5 + 0.0) / 4 and float(surf) == (1.0 + 1.0 + 0.0 + 2.0) / 4
    est.backward(retain_graph=True)
    assert leaves[1].grad.tolist() == [0.25, 0.0, 0.25, 0.0, 0.0]
    # through est = map_z - z: d|sdf - |est||/dz = sign(t) * -sign(est) * -1; the map is constant, so x and y get nothing
    assert leaves[0].grad.tolist() == [[0.0, 0.0, 0.25], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]]
    leaves[0].grad = None
    surf.backward()
    assert leaves[0].grad[:, 2].tolist() == [-0.25, -0.25, 0.0, -0.25, 0.0]                 # |est| / 1 = 2 = clamp_max at sample 3: passes
    want = cl.estimation_losses(x.double(), torch.full((16, 16), 3.0, dtype=torch.float64), EYE_CAM["world_to_view"], EYE_CAM["projection"], 0.5,
                                sdf=sdf.double(), scale=1.0, clamp_max=2.0, with_surface=True)
    assert float(want[0]) == float(est) and float(want[1]) == float(surf) and int(want[2]) == 4
    assert image.grad[..., 0].sum().item() == pytest.approx(0.25 * 3 - 0.25, abs=1e-6)       # the taps of both backwards: sum of dL/dest


# ---------------------------------------------------------------------------------------------------------------- better normal
def _normal_call(x, idx, knn, normals, points, min_scaling, opac, only):
    leaves = [t.to(DEV).clone().requires_grad_(True) for t in (x, normals, points)]
    loss = coarse_loss.better_normal_loss(leaves[0], idx.to(DEV), knn.to(DEV), leaves[1], leaves[2], min_scaling.to(DEV), opac.to(DEV), only)
    loss.backward()
    return loss, dict(grad_samples=leaves[0].grad, grad_normals=leaves[1].grad, grad_points=leaves[2].grad)


def _normal_restated(x, idx, knn, normals, points, min_scaling, opac, only, dtype):
    leaves = [t.to(dtype).clone().requires_grad_(True) for t in (x, normals, points)]
    loss = cl.better_normal_loss(leaves[0], idx, knn, leaves[1], leaves[2], min_scaling.to(dtype), opac.to(dtype), only)
    loss.backward()
    return loss, dict(grad_samples=leaves[0].grad, grad_normals=leaves[1].grad, grad_points=leaves[2].grad)


def _normal_inputs(n=6000, K=16):
    return (_t("samples")[:n], _t("sample_idx")[:n].to(torch.int64), STATE["knn_idx"][:, :K].contiguous(), STATE["normals"], STATE["points"],
            STATE["scaling"].min(dim=-1)[0], _t("field_opacities")[:n, :K].contiguous())


def _unreferenced(idx, knn, P):
    free = torch.ones(P, dtype=torch.bool)
    free[knn[idx].flatten()] = False
    free[idx] = False
    return free


@pytest.mark.parametrize("only", [True, False], ids=["normal_only", "normal_full"])
def test_better_normal_loss_matches_the_fixture(only):
    tag = "normal_only" if only else "normal_full"
    inputs = _normal_inputs()
    runs = [_normal_call(*inputs, only) for _ in range(2)]
    loss, g = runs[0]
    assert loss.dim() == 0 and loss.device.type == "cuda"
    _check(tag + "_loss", loss, FX[tag + "_loss"], FX["yard_" + tag + "_loss"])
    _check(tag + "_grad_normals", g["grad_normals"], FX[tag + "_grad_normals"], FX["yard_" + tag + "_grad_normals"])
    if only:
        assert g["grad_samples"] is None and g["grad_points"] is None
    else:
        _check(tag + "_grad_points", g["grad_points"], FX[tag + "_grad_points"], FX["yard_" + tag + "_grad_points"])
        _check(tag + "_grad_samples", g["grad_samples"], FX[tag + "_grad_samples"], FX["yard_" + tag + "_grad_samples"])
    assert torch.equal(runs[1][0], loss)                                        # bit-identical from run to run
    for k, v in g.items():
        assert v is None or torch.equal(runs[1][1][k], v), k


def _normal_case(what, inputs, only):
    want = _normal_restated(*inputs, only, torch.float64)
    f32 = _normal_restated(*inputs, only, torch.float32)
    loss, g = _normal_call(*inputs, only)
    _check(f"{what} loss", loss, want[0], cl.scalar_distance(f32[0], want[0]))
    for k, v in g.items():
        if want[1][k] is None:
            assert v is None
        else:
            _check(f"{what} {k}", v, want[1][k], rs.distance(f32[1][k], want[1][k]))
    free = _unreferenced(inputs[1], inputs[2], inputs[3].shape[0]).to(DEV)       # Gaussians nothing references: exactly zero
    for k in ("grad_normals", "grad_points"):
        assert g[k] is None or (not g[k][free].any() and g[k][~free].any()), k
    return loss, g


@pytest.mark.parametrize("only", [True, False], ids=["normal_only", "normal_full"])
@pytest.mark.parametrize("n,K", [(1, 16), (257, 16), (6000, 8), (257, 8)])
def test_better_normal_loss_shapes(n, K, only):
    inputs = _normal_inputs(n, K)
    if n == 257:
        assert _unreferenced(inputs[1], inputs[2], 2500).sum() > 100
    _normal_case(f"normal n={n} K={K} only={only}", inputs, only)


@pytest.mark.parametrize("K", [16, 8])
def test_better_normal_loss_4097_samples_of_one_gaussian(K):
    """one group of the gather 4097 * (1 + 1/K-th of the neighbours) entries long: the target's own entries and those of its pairs"""
    n, target = 4097, 1234
    g = torch.Generator().manual_seed(3)
    _, _, knn, normals, points, ms, _ = _normal_inputs(1, K)
    x = points[target][None] + 0.05 * torch.randn(n, 3, generator=g)
    idx = torch.full((n,), target, dtype=torch.int64)
    opac = torch.rand(n, K, generator=g) * 0.1 + 0.01
    for only in (True, False):
        _, got = _normal_case(f"normal one Gaussian K={K} only={only}", (x, idx, knn, normals, points, ms, opac), only)
        rows = got["grad_normals"].abs().sum(-1).nonzero().flatten().tolist()
        assert sorted(rows) == sorted(set(knn[target].tolist() + [target]))


def test_better_normal_loss_out_of_range_and_wrapped_neighbours():
    x, idx, knn, normals, points, ms, opac = _normal_inputs(257, 16)
    P = 2500
    picked = torch.zeros(P, 16, dtype=torch.bool)
    picked[idx[::3], 5] = True
    picked[idx[1::4], 11] = True
    bad = knn.clone()
    bad[picked] = torch.where(torch.arange(int(picked.sum())) % 2 == 0, torch.tensor(P + 5), torch.tensor(-P - 3))
    # the same as: those pairs carry no weight (index 0 stands in, its opacity zero)
    stand_in, opac0 = knn.clone(), opac.clone()
    stand_in[picked] = 0
    opac0[picked[idx]] = 0.0
    for only in (True, False):
        want = _normal_restated(x, idx, stand_in, normals, points, ms, opac0, only, torch.float64)
        f32 = _normal_restated(x, idx, stand_in, normals, points, ms, opac0, only, torch.float32)
        loss, g = _normal_call(x, idx, bad, normals, points, ms, opac, only)
        _check(f"out-of-range loss only={only}", loss, want[0], cl.scalar_distance(f32[0], want[0]))
        for k, v in g.items():
            if v is not None:
                _check(f"out-of-range {k} only={only}", v, want[1][k], rs.distance(f32[1][k], want[1][k]))
        # negative indices wrap once: j - P is j
        wrapped = knn.clone()
        wrapped[picked] -= P
        plain, g_plain = _normal_call(x, idx, knn, normals, points, ms, opac, only)
        again, g_again = _normal_call(x, (idx - P), wrapped, normals, points, ms, opac, only)
        assert torch.equal(plain, again) and all(v is None or torch.equal(v, g_again[k]) for k, v in g_plain.items())


@pytest.mark.parametrize("K", [16, 2])
def test_better_normal_kinks_with_exact_values(K):
    """P = K + 1 Gaussians on a lattice: Gaussian 0 (the sample's own) has the normal e_x, the odd neighbours e_y (axis-aligned and
    orthogonal: sign = 0, the pair carries no weight and its normal no gradient), the even ones (-1/2, 0, 1/2) or -e_x (flipped by the
    sign).
    Sample 1 has an all-zero opacity row (sum w = 0 -> clamp 1e-6 -> w^ = 0: loss_n = |n_s|^2 = 1).  Gaussian 2's min_scaling is
    below 1e-6 (clamped to 1e-6; its opacity 2^-40 keeps its weight next to the others')."""
    P = K + 1
    normals = torch.zeros(P, 3)
    normals[0, 0] = 1.0
    normals[1::2, 1] = 1.0
    normals[2::4] = torch.tensor([-0.5, 0.0, 0.5])
    normals[4::4, 0] = -1.0
    points = torch.zeros(P, 3)
    points[:, 0] = torch.arange(P) * 0.25
    knn = (torch.arange(P)[:, None] + 1 + torch.arange(K)[None]) % P             # Gaussian 0's neighbours: 1 .. K
    ms = torch.full((P,), 0.5)
    ms[2] = 2.0 ** -24
    x = torch.tensor([[2.0, 0.5, 0.25], [1.0, 0.25, 0.5]])
    idx = torch.zeros(2, dtype=torch.int64)
    opac = torch.full((2, K), 0.5)
    opac[0, 1] = 2.0 ** -40                                                      # Gaussian 2: its weight / 1e-12 stays comparable with the others
    opac[1] = 0.0
    for only in (True, False):
        want = _normal_restated(x, idx, knn, normals, points, ms, opac, only, torch.float64)
        loss, g = _normal_call(x, idx, knn, normals, points, ms, opac, only)
        _check(f"kinks K={K} only={only} loss", loss, want[0], 0.0)
        for k, v in g.items():
            if v is not None:
                _check(f"kinks K={K} only={only} {k}", v, want[1][k], 0.0)
        assert not g["grad_normals"][1::2].any()                                 # sign = 0: nothing reaches the orthogonal normals
        assert torch.isfinite(g["grad_normals"]).all() and g["grad_normals"][2].any()
    # the all-zero row alone: loss = |e_x|^2 = 1, dL/dn_s = 2 e_x
    loss, g = _normal_call(x[1:], idx[1:], knn, normals, points, ms, opac[1:], True)
    assert float(loss) == 1.0 and g["grad_normals"][0].tolist() == [2.0, 0.0, 0.0] and not g["grad_normals"][1:].any()


def test_the_three_operations_make_no_host_synchronisation():
    """forward and backward of each operation with the camera's tensors (znear as its device tensor) under
    torch.cuda.set_sync_debug_mode("error"): a host read anywhere raises"""
    x, idx, sdf, density, beta = (t.to(DEV) for t in estimation_inputs(FX))
    V, Pm, znear, cc = (t.to(DEV) for t in (CAM["world_to_view"], CAM["projection"], CAM["znear"], _t("cam_center")))
    pts, q, sc, knn, normals = (STATE[k].to(DEV) for k in ("points", "quaternions", "scaling", "knn_idx", "normals"))
    opac, ms = _t("field_opacities").to(DEV), STATE["scaling"].min(dim=-1)[0].to(DEV)
    image, depth = _stride3(_t("depth_map", REG_FX))

    def all_three():
        close, std = coarse_loss.surface_band(pts, q, sc, V, cc, Pm, depth, 2.0)
        leaves = [t.clone().requires_grad_(True) for t in (x, sdf, normals, pts)]
        est, surf, M = coarse_loss.estimation_losses(leaves[0], depth, V, Pm, znear, sdf=leaves[1], std=std, sample_idx=idx, clamp_max=30.0,
                                                     with_surface=True)
        loss = coarse_loss.better_normal_loss(leaves[0][:6000], idx[:6000], knn, leaves[2], leaves[3], ms, opac, False)
        (est + surf + loss).backward()
        return M
    all_three(); torch.cuda.synchronize()                                        # (warm: code objects, the allocator)
    torch.cuda.set_sync_debug_mode("error")
    try:
        M = all_three()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert int(M) == 6000


# -------------------------------------------------------------------------------------------------------------------- composite
def _new_model(**variant):
    shims.install()
    from tests.golden.make_sugar_field import p3d_cameras_like_the_reference
    from tests.sugar_regulariser_standin import make_module
    cams = syn.orbit_cameras(int(FIELD_FX["W"]), int(FIELD_FX["H"]))
    return make_module(**variant).SuGaR(FIELD_FX, DEV, cams, p3d_cameras_like_the_reference(cams).to(DEV))


PARAMS = ("_points", "_scales", "_quaternions", "all_densities")
TERMS = ("sdf_estimation_loss", "samples_on_surface_loss", "sdf_better_normal_loss")
WEIGHTS = dict(sdf_estimation_loss=1.0, samples_on_surface_loss=0.5, sdf_better_normal_loss=0.75)


@pytest.mark.parametrize("variant", [dict(), dict(patch_sugar=True, patch_gathers=True)], ids=["plain", "row_gathers"])
@pytest.mark.parametrize("options", [
    dict(sdf_estimation_mode="sdf"),
    dict(sdf_estimation_mode="density", squared_sdf_estimation_loss=True, squared_samples_on_surface_loss=True, normalize_by_sdf_std=True,
         sdf_better_normal_gradient_through_normal_only=False),
], ids=["sdf_defaults", "density_squared_std_full"])
def test_composite_equals_the_restatement_on_the_stand_in(variant, options):
    """same seed, same stand-in: the method calls (sampler, field, normals) are the same kernels in both runs and give the same bits, so
    the float64 run of the restatement measures the inline statements alone; its float32 run gives the yards"""
    model = _new_model(**variant)
    fov_camera = model.nerfmodel.training_cameras.p3d_cameras[int(REG_FX["depth_cam_idx"])]
    assert torch.equal(fov_camera.get_world_to_view_transform().get_matrix().cpu(), CAM["world_to_view"])
    visible = _t("sample_mask").to(DEV)
    options = dict(options, enforce_samples_to_be_on_surface=True, close_gaussian_threshold=float(FX["band_threshold"]), density_factor=0.2,
                   n_samples_for_sdf_regularization=6000, sdf_sampling_proportional_to_volume=True, cameras_spatial_extent=EXTENT)

    def run(fn, **more):
        model.zero_grad()
        image, depth = _stride3(_t("depth_map", REG_FX))
        torch.manual_seed(123)
        out = fn(model, fov_camera, depth, visible, **options, **more)
        sum(WEIGHTS[k] * out[k] for k in TERMS).backward()
        grads = {n: getattr(model, n).grad.detach().clone() for n in PARAMS}
        grads["depth"] = image.grad[..., 0].detach().clone()
        return out, grads
    got, got_g = run(coarse_loss.regulariser_terms)
    again, again_g = run(coarse_loss.regulariser_terms)
    want, want_g = run(cl.regulariser_terms, dtype=torch.float64)
    f32, f32_g = run(cl.regulariser_terms, dtype=torch.float32)
    assert set(got) == set(TERMS) | {"n_projected", "n_samples"} and got["n_samples"] == 6000
    assert int(got["n_projected"]) == int(want["n_projected"]) == 6000
    assert torch.equal(want["close"], f32["close"]) and torch.equal(want["samples"], f32["samples"])      # the same draw in every run
    for k in TERMS:
        _check(f"composite {k}", got[k], want[k], cl.scalar_distance(f32[k], want[k]))
        assert torch.equal(got[k], again[k])
    for k in got_g:
        _check(f"composite grad {k}", got_g[k], want_g[k], rs.distance(f32_g[k], want_g[k]))
        if k != "depth":
            assert torch.equal(got_g[k], again_g[k]), k
    band = coarse_loss.surface_band(model.points, model.quaternions, model.scaling, CAM["world_to_view"].to(DEV), fov_camera.get_camera_center(),
                                    CAM["projection"].to(DEV), _stride3(_t("depth_map", REG_FX), grad=False)[1], float(FX["band_threshold"]))
    assert torch.equal(band[0], want["close"]) and torch.equal(band[0].cpu(), _t("band_close"))
