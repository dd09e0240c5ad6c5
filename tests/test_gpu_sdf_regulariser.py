"""GPU parity of the SDF regulariser bindings (sugar_patch.install_regulariser over csrc/sdf_regulariser.hip), driven through the
bound methods of a stand-in class (tests/sugar_regulariser_standin.py) that holds the reference model's state.

  * sample transform, smallest axis, depth lookup: values and every gradient against the float64 restatement
    (tests/sdf_regulariser_restatement.py) fed the inputs of tests/golden/sdf_regulariser.npz, which the reference's own methods
    wrote.  The bar of an array is 4 x its `yard_*` -- the distance of the reference method's own float32 result from the same
    float64 restatement, times a margin for the different summation order -- with a floor of 1e-7.  For a case cut out of the
    fixture (the first n samples or points) the values' yard is that of the same rows of the reference's recorded result.
  * the field tail: the `field_*` arrays of tests/golden/sugar_field.npz at that file's bars (2e-5 values, 1e-4 gradients), the
    gradient w.r.t. `_scales` included, which now comes through dmin_scaling.
  * shapes: N in {1, 257, 6000}; K = 16 and K = 8; 4097 samples of one Gaussian; Gaussians that nothing references (their gradient
    rows exactly zero); lookup points exactly on pixel centres and on the border; the stride-3 depth view.
  * every per-Gaussian gradient is bit-identical between two runs (the depth map's gradient, float atomics, is exempt).
  * the bindings give the same results with `install` and `install_row_gathers` installed, in either order, as without.
Each test prints the distances it measured."""
import copy
import os
import sys
import types

import numpy as np
import pytest
import torch

from sugar_amd import shims, synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
FX = np.load(os.path.join(HERE, "golden", "sdf_regulariser.npz"))
FIELD_FX = np.load(os.path.join(HERE, "golden", "sugar_field.npz"))
PARAMS = ("_points", "_scales", "_quaternions")
FLOOR = 1e-7

from tests import sdf_regulariser_restatement as rs  # noqa: E402


def _bar(name):
    return max(4.0 * float(FX["yard_" + name]), FLOOR)


def _check(what, got, want, bar):
    d = rs.distance(got, want)
    print(f"{what:44s} distance {d:.3e}   bar {bar:.3e}")
    assert torch.isfinite(torch.as_tensor(got)).all(), what
    assert d <= bar, (what, d, bar)


def _t(k, fx=FX):
    return torch.as_tensor(fx[k])


def _new_model(**variant):
    shims.install()
    sys.path.insert(0, os.path.join(HERE, "golden"))
    from tests.golden.make_sugar_field import p3d_cameras_like_the_reference
    from tests.sugar_regulariser_standin import make_module
    cams = syn.orbit_cameras(int(FIELD_FX["W"]), int(FIELD_FX["H"]))
    return make_module(**variant).SuGaR(FIELD_FX, DEV, cams, p3d_cameras_like_the_reference(cams).to(DEV))


@pytest.fixture(scope="module")
def model():
    return _new_model()


class Twin:
    """the model's raw parameters in float64 on the CPU, and its properties (sugar_model.py:383-479, not mesh-bound)"""
    def __init__(self):
        self.raw = [_t("state" + n, FIELD_FX).double().requires_grad_(True) for n in PARAMS]
        self.all_densities = _t("stateall_densities", FIELD_FX).double().requires_grad_(True)

    def props(self):
        return self.raw[0], torch.exp(self.raw[1]), torch.nn.functional.normalize(self.raw[2], dim=-1)

    def grads(self, value, weights, extra=()):
        leaves = self.raw + [self.all_densities] + list(extra)
        got = torch.autograd.grad((value * weights.double()).sum(), leaves, allow_unused=True)
        return [g if g is not None else torch.zeros_like(t) for g, t in zip(got, leaves)]


@pytest.fixture(scope="module")
def twin():
    return Twin()


def _param_grads(model):
    return [getattr(model, n).grad.clone() for n in PARAMS]


class _Draws:
    """hands the bound sampler the fixture's draws where the reference's method would draw them: `torch.multinomial` (positions
    among the masked Gaussians) and `torch.randn_like`"""
    def __init__(self, monkeypatch, idx, noise, mask):
        rank = torch.cumsum(mask.to(torch.int64), 0) - 1 if mask is not None else None
        picks = (rank[idx] if mask is not None else idx).to(DEV)
        self.calls = []
        monkeypatch.setattr(torch, "multinomial", lambda probs, num_samples, replacement=False: self._give("multinomial", picks, num_samples))
        monkeypatch.setattr(torch, "randn_like", lambda like, **k: self._give("randn_like", noise.to(DEV), like.shape[0]))

    def _give(self, what, value, n):
        assert value.shape[0] == n
        self.calls.append(what)
        return value


# ------------------------------------------------------------------------------------------------------------ sample transform
@pytest.fixture(scope="module")
def sample_ref(twin):
    out = {}
    for n in (1, 257, 6000):
        pts, sc, q = twin.props()
        idx, noise, w = _t("sample_idx")[:n], _t("sample_noise")[:n], _t("sample_w")[:n]
        x = rs.sample_transform(pts, q, sc, idx, noise.double(), float(FX["sample_factor"]))
        out[n] = (x.detach(), [g.detach() for g in twin.grads(x, w)[:3]])
    return out


@pytest.mark.parametrize("n", [1, 257, 6000])
def test_sample_points_in_gaussians_matches_the_restatement(model, sample_ref, monkeypatch, n):
    mask = _t("sample_mask")
    idx, noise, w = _t("sample_idx")[:n], _t("sample_noise")[:n], _t("sample_w")[:n]
    draws = _Draws(monkeypatch, idx, noise, mask)
    runs = []
    for _ in range(2):
        model.zero_grad()
        x, got_idx = model.sample_points_in_gaussians(n, sampling_scale_factor=float(FX["sample_factor"]), mask=mask.to(DEV),
                                                      probabilities_proportional_to_volume=True)
        (x * w.to(DEV)).sum().backward()
        runs.append((x.detach().clone(), _param_grads(model)))
    assert draws.calls == ["multinomial", "randn_like"] * 2        # the reference's draws, in the reference's order
    assert torch.equal(got_idx.cpu(), idx) and x.shape == (n, 3)
    want_x, want_g = sample_ref[n]
    yard_rows = rs.distance(FX["sample_out"][:n], want_x)         # the reference's own float32 rows against the same restatement
    _check(f"sample_out[:{n}]", x, want_x, max(4.0 * yard_rows, FLOOR))
    for name, got, want in zip(PARAMS, runs[0][1], want_g):
        _check(f"sample_grad{name} (n = {n})", got, want, _bar("sample_grad" + name))
    assert torch.equal(runs[0][0], runs[1][0]) and all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))   # bit-identical
    # Gaussians that no sample references: their rows of the kernel's per-Gaussian gradients are exactly zero
    from sugar_amd.sdf_regulariser import sample_transform
    leaves = [t.detach().clone().requires_grad_(True) for t in (model.points, model.quaternions, model.scaling)]
    out = sample_transform(*leaves, idx.to(DEV), noise.to(DEV), 1.5)
    out.backward(w.to(DEV))
    unreferenced = torch.ones(leaves[0].shape[0], dtype=torch.bool)
    unreferenced[idx] = False
    assert unreferenced.any()
    for t in leaves:
        assert torch.isfinite(t.grad).all() and not t.grad[unreferenced.to(DEV)].any()


def test_a_seeded_call_draws_what_the_tensor_code_draws(model):
    """the draws are left as they were: volume-proportional probabilities over the masked Gaussians, `torch.multinomial`, the index
    composition through the mask, then `torch.randn_like` of the gathered points -- the same generator state gives the same indices
    and the same noise as those statements give on this device"""
    n, factor = 6000, 1.5
    mask = _t("sample_mask").to(DEV)
    torch.manual_seed(123)
    x, idx = model.sample_points_in_gaussians(n, sampling_scale_factor=factor, mask=mask, probabilities_proportional_to_volume=True)
    torch.manual_seed(123)
    with torch.no_grad():
        s = model.scaling[mask]
        volume = (s[..., 0] * s[..., 1] * s[..., 2]).abs()
        picks = torch.multinomial(volume / volume.sum(dim=-1, keepdim=True), num_samples=n, replacement=True)
        want_idx = torch.arange(model.n_points, device=DEV)[mask][picks]
        noise = torch.randn_like(model.points[want_idx])
        want = rs.sample_transform(model.points.double(), model.quaternions.double(), model.scaling.double(), want_idx, noise.double(), factor)
    assert torch.equal(idx, want_idx)
    _check("sample_out (seeded draws)", x, want, _bar("sample_out"))


def test_4097_samples_of_one_gaussian(model, twin, monkeypatch):
    """one group of the backward 4097 entries long: every lane of its sixteen walks 256 or 257 of them.  The noise and the weights are
    positive, so that the sums are well conditioned and the distance measures the kernel's arithmetic, not the cancellation of a sum."""
    n, target = 4097, 1234
    g = torch.Generator().manual_seed(3)
    idx = torch.full((n,), target, dtype=torch.int64)
    noise, w = torch.randn(n, 3, generator=g).abs(), torch.rand(n, 3, generator=g) + 0.5
    _Draws(monkeypatch, idx, noise, None)
    model.zero_grad()
    x, got_idx = model.sample_points_in_gaussians(n, sampling_scale_factor=0.75, mask=None)
    (x * w.to(DEV)).sum().backward()
    assert torch.equal(got_idx.cpu(), idx)
    pts, sc, q = twin.props()
    want = rs.sample_transform(pts, q, sc, idx, noise.double(), 0.75)
    _check("sample_out (one Gaussian)", x, want.detach(), _bar("sample_out"))
    for name, got, g64 in zip(PARAMS, _param_grads(model), twin.grads(want, w)[:3]):
        _check(f"sample_grad{name} (one Gaussian)", got, g64, _bar("sample_grad" + name))
        rows = got.abs().sum(-1).nonzero().flatten().tolist()
        assert rows == [target], name


# --------------------------------------------------------------------------------------------------------------- smallest axis
def test_smallest_axis_and_normals_match_the_restatement(model, twin):
    runs = []
    for _ in range(2):
        model.zero_grad()
        axis, axis_idx = model.get_smallest_axis(return_idx=True)
        (axis * _t("axis_w").to(DEV)).sum().backward()
        runs.append((axis.detach().clone(), model._quaternions.grad.clone()))
        assert model._scales.grad is None or not model._scales.grad.any()      # the backward goes to the quaternions only
    assert axis_idx.dtype == torch.int64 and torch.equal(axis_idx.cpu(), _t("axis_idx"))
    _, sc, q = twin.props()
    want, _ = rs.smallest_axis(q, sc)
    _check("axis_out", axis, want.detach(), _bar("axis_out"))
    _check("axis_grad_quaternions", runs[0][1], twin.grads(want, _t("axis_w"))[2], _bar("axis_grad_quaternions"))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert torch.equal(model.get_smallest_axis(), runs[0][0])
    normals = model.get_normals()
    _check("normals_out", normals, want.detach(), _bar("normals_out"))
    # ties: the lowest index wins
    from sugar_amd.sdf_regulariser import smallest_axis
    s = torch.tensor([[2., 1., 1.], [1., 1., 1.], [3., 2., 1.], [1., 2., 1.]], device=DEV)
    q4 = torch.nn.functional.normalize(torch.randn(4, 4, generator=torch.Generator().manual_seed(1)), dim=-1).to(DEV)
    assert smallest_axis(q4, s)[1].tolist() == [1, 0, 2, 0]


# ---------------------------------------------------------------------------------------------------------------- depth lookup
def _stride3(depth_hw):
    image = depth_hw[..., None].repeat(1, 1, 3).contiguous().to(DEV).requires_grad_(True)      # an [H,W,3] render
    return image, image[..., 0]


@pytest.fixture(scope="module")
def depth_ref():
    Pm, d = _t("depth_projection").double(), _t("depth_map").double()
    out = {}
    for m in (1, 257, 7000):
        depth, pts = d.clone().requires_grad_(True), _t("depth_pts")[:m].double().requires_grad_(True)
        z = rs.depth_lookup(Pm, depth, pts)
        gp, gd = torch.autograd.grad((z * _t("depth_w")[:m].double()).sum(), (pts, depth))
        out[m] = (z.detach(), gp, gd)
    return out


@pytest.mark.parametrize("m", [1, 257, 7000])
def test_points_depth_in_depth_map_matches_the_restatement(model, depth_ref, m):
    assert len(FX["depth_pts"]) == 7000
    fov_camera = model.nerfmodel.training_cameras.p3d_cameras[int(FX["depth_cam_idx"])]
    assert torch.equal(fov_camera.get_projection_transform().get_matrix().cpu(), _t("depth_projection"))
    image, depth = _stride3(_t("depth_map"))
    assert depth.stride() == (3 * depth.shape[1], 3)                  # the stride-3 view, read in place
    pts = _t("depth_pts")[:m].to(DEV).requires_grad_(True)
    z = model.get_points_depth_in_depth_map(fov_camera, depth, pts)
    (z * _t("depth_w")[:m].to(DEV)).sum().backward()
    want_z, want_gp, want_gd = depth_ref[m]
    _check(f"depth_out[:{m}]", z, want_z, max(4.0 * rs.distance(FX["depth_out"][:m], want_z), FLOOR))
    _check(f"depth_grad_pts (m = {m})", pts.grad, want_gp, _bar("depth_grad_pts"))
    _check(f"depth_grad_map (m = {m})", image.grad[..., 0], want_gd, _bar("depth_grad_map"))
    assert not image.grad[..., 1:].any()
    first = pts.grad.clone()
    pts.grad = None
    (model.get_points_depth_in_depth_map(fov_camera, depth, pts) * _t("depth_w")[:m].to(DEV)).sum().backward()
    assert torch.equal(first, pts.grad)                               # the points' gradient is bit-identical (the map's need not be)
    with torch.no_grad():                                             # the trainer's first call: no graph
        assert torch.equal(model.get_points_depth_in_depth_map(fov_camera, depth.detach(), pts.detach()), z.detach())


def test_lookup_points_on_pixel_centres_and_on_the_border(model):
    """a 16 x 16 map under an identity projection: pixel k's centre is x = 1 - (2 k + 1) / 16, exact in float32, and so is every step of
    the kernel's coordinate arithmetic -- the points sit EXACTLY on pixel centres, on the border (pixel 0 and pixel 15, where
    grid_sample's clamp is active and the coordinate's gradient is zero) and beyond it."""
    S = 16
    small = copy.copy(model)
    small.image_height = small.image_width = S
    eye = torch.eye(4, device=DEV)[None]
    camera = types.SimpleNamespace(get_projection_transform=lambda: types.SimpleNamespace(get_matrix=lambda: eye))
    centre = lambda k: 1.0 - (2.0 * k + 1.0) / S
    ks = [0.0, 1.0, 7.0, 14.0, 15.0, -0.5, 15.5, -3.0, 20.0, 3.5, 6.25]     # centres, both borders, beyond them, in between
    xy = torch.tensor([[centre(a), centre(b)] for a in ks for b in ks], dtype=torch.float32)
    pts = torch.cat((xy, torch.ones(len(xy), 1)), 1)
    g = torch.Generator().manual_seed(9)
    dmap, w = torch.rand(S, S, generator=g) + 1.0, torch.randn(len(pts), generator=g)
    image, depth = _stride3(dmap)
    p = pts.to(DEV).requires_grad_(True)
    z = small.get_points_depth_in_depth_map(camera, depth, p)
    (z * w.to(DEV)).sum().backward()
    d64, p64 = dmap.double().requires_grad_(True), pts.double().requires_grad_(True)
    z64 = rs.depth_lookup(eye[0].cpu().double(), d64, p64)
    gp, gd = torch.autograd.grad((z64 * w.double()).sum(), (p64, d64))
    _check("depth_out (centres, border)", z, z64.detach(), _bar("depth_out"))
    _check("depth_grad_pts (centres, border)", p.grad, gp, _bar("depth_grad_pts"))
    _check("depth_grad_map (centres, border)", image.grad[..., 0], gd, _bar("depth_grad_map"))
    on_centre = torch.tensor([[a == int(a) and 0 <= a <= 15 and b == int(b) and 0 <= b <= 15 for b in ks] for a in ks]).flatten()
    ia, ib = torch.tensor([[int(a), int(b)] for a in ks for b in ks])[on_centre].T
    assert torch.equal(z.detach().cpu()[on_centre], dmap[ib, ia])     # on a pixel centre the lookup IS the pixel
    clamped_x = torch.tensor([[a <= 0 or a >= 15 for b in ks] for a in ks]).flatten()
    clamped_y = torch.tensor([[b <= 0 or b >= 15 for b in ks] for a in ks]).flatten()
    assert not p.grad.cpu()[clamped_x, 0].any() and not p.grad.cpu()[clamped_y, 1].any()
    assert p.grad.cpu()[~clamped_x, 0].abs().min() > 0


# ------------------------------------------------------------------------------------------------------------------- sdf field
def _field_call(model, n, K=16, factor=0.2, x_grad=True):
    x = _t("field_x", FIELD_FX)[:n].to(DEV).requires_grad_(x_grad)
    gi = _t("field_gaussian_idx", FIELD_FX)[:n].to(DEV)
    kw = dict(return_sdf=True, density_threshold=1., density_factor=factor, return_sdf_grad=False,
              return_closest_gaussian_opacities=True, return_beta=True)
    if K == 16:
        return x, model.get_field_values(x, gi, **kw)
    return x, model.get_field_values(x, closest_gaussians_idx=model.knn_idx[gi][:, :K].contiguous(), **kw)


def _functional(f, n, K, to):
    w = lambda k: to(_t("field_" + k, FIELD_FX)[:n])
    return ((f["density"] * w("w_density")).sum() + (f["sdf"] * w("w_sdf")).sum()
            + (f["closest_gaussian_opacities"] * w("w_opacities")[:, :K]).sum() + (f["beta"] * w("w_beta")).sum())


def _twin_field(twin, n, K, factor):
    """the float64 restatement of get_field_values over the twin's parameters: (fields, x, gradients w.r.t. x and the four parameters)"""
    pts, sc, q = twin.props()
    B = rs.rotation_matrix(q) * (1.0 / sc.clamp(min=1e-8))[:, None]             # get_covariance(return_sqrt, inverse_scales), :730-736
    x = _t("field_x", FIELD_FX)[:n].double().requires_grad_(True)
    nbr = _t("state_knn_idx", FIELD_FX)[_t("field_gaussian_idx", FIELD_FX)[:n]][:, :K]
    o, density, beta, sdf = rs.sdf_field(x, nbr, pts, B, torch.sigmoid(twin.all_densities.view(-1)), sc.min(dim=-1)[0], factor, 1.0, 1e-16)
    f = {"density": density, "sdf": sdf, "beta": beta, "closest_gaussian_opacities": o}
    grads = twin.grads(_functional(f, n, K, lambda t: t.double()), torch.ones((), dtype=torch.float64), extra=[x])
    return f, grads


def test_field_values_and_gradients_match_the_reference_method(model):
    """the test of tests/test_gpu_sugar_field.py, through the one-forward-one-backward binding"""
    with torch.no_grad():
        _, hi = _field_call(model, 6000, factor=1.3, x_grad=False)
    for k in ("density", "sdf", "beta", "closest_gaussian_opacities"):
        ref = FIELD_FX["field_hi_" + k]
        ok = np.isfinite(ref)
        assert ok.mean() > 0.99
        _check("field_hi_" + k, hi[k].cpu()[torch.as_tensor(ok)], ref[ok], 2e-5)
    runs = []
    for _ in range(2):
        model.zero_grad()
        x, f = _field_call(model, 6000)
        _functional(f, 6000, 16, lambda t: t.to(DEV)).backward()
        runs.append([x.grad.clone()] + [getattr(model, n).grad.clone() for n in PARAMS + ("all_densities",)])
    for k in ("density", "sdf", "beta", "closest_gaussian_opacities"):
        _check("field_out_" + k, f[k], FIELD_FX["field_out_" + k], 2e-5)
    _check("field_grad_x", runs[0][0], FIELD_FX["field_grad_x"], 1e-4)
    for name, got in zip(PARAMS + ("all_densities",), runs[0][1:]):
        _check("field_grad" + name, got, FIELD_FX["field_grad" + name], 1e-4)
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1]))            # bit-identical from run to run


@pytest.mark.parametrize("n,K", [(1, 16), (257, 16), (6000, 8), (257, 8)])
def test_field_tail_shapes_against_the_restatement(model, twin, n, K):
    want, want_g = _twin_field(twin, n, K, 0.2)
    model.zero_grad()
    x, f = _field_call(model, n, K)
    _functional(f, n, K, lambda t: t.to(DEV)).backward()
    for k in ("density", "sdf", "beta", "closest_gaussian_opacities"):
        assert f[k].shape == want[k].shape
        _check(f"{k} (n = {n}, K = {K})", f[k], want[k].detach(), 2e-5)
    _check(f"grad_x (n = {n}, K = {K})", x.grad, want_g[4], 1e-4)
    for i, name in enumerate(PARAMS + ("all_densities",)):
        _check(f"grad{name} (n = {n}, K = {K})", getattr(model, name).grad, want_g[i], 1e-4)


@pytest.mark.parametrize("K", [16, 8])
def test_field_gradient_rows_of_unreferenced_gaussians_are_zero(model, K):
    from sugar_amd.sdf_regulariser import sdf_field
    n = 257
    x = _t("field_x", FIELD_FX)[:n].to(DEV)
    nbr = model.knn_idx[_t("field_gaussian_idx", FIELD_FX)[:n].to(DEV)][:, :K].contiguous()
    with torch.no_grad():
        B = model.get_covariance(return_full_matrix=True, return_sqrt=True, inverse_scales=True)
    leaves = [t.detach().clone().requires_grad_(True) for t in (model.points, B, model.strengths, model.scaling.min(dim=-1)[0])]
    runs = []
    for _ in range(2):
        for t in leaves:
            t.grad = None
        o, density, beta, sdf = sdf_field(x, nbr, *leaves, 0.2, 1.0, 1e-16)
        (o.sum() + density.sum() + 0.3 * beta.sum() - 0.7 * sdf.sum()).backward()
        runs.append([t.grad.clone() for t in leaves])
    unreferenced = torch.ones(leaves[0].shape[0], dtype=torch.bool, device=DEV)
    unreferenced[nbr.flatten()] = False
    assert unreferenced.sum() > 100
    for a, b in zip(*runs):
        assert torch.isfinite(a).all() and not a[unreferenced].any() and a[~unreferenced].any()
        assert torch.equal(a, b)


# --------------------------------------------------------------------------------------------------------- with the other bindings
@pytest.mark.parametrize("variant", [dict(patch_sugar=True, patch_gathers=True), dict(patch_sugar=True, patch_gathers=True, regulariser_first=True)],
                         ids=["regulariser_last", "regulariser_first"])
def test_same_results_with_patch_sugar_and_patch_gathers_installed(model, monkeypatch, variant):
    other = _new_model(**variant)
    assert sorted(type(other)._sugar_amd_original) and sorted(type(other)._sugar_amd_row_gather_original)
    from sugar_amd.row_gather import RowGatherTensor
    assert isinstance(other.points, RowGatherTensor) and not isinstance(model.points, RowGatherTensor)
    n = 6000
    _Draws(monkeypatch, _t("sample_idx"), _t("sample_noise"), _t("sample_mask"))
    fov_camera = model.nerfmodel.training_cameras.p3d_cameras[int(FX["depth_cam_idx"])]
    results = []
    for m in (model, other):
        exact = []

        def backward_of(loss):     # one operation at a time: a parameter then gets at most two addends, whose order cannot matter
            m.zero_grad()
            loss.backward()
            exact.extend(getattr(m, name).grad for name in PARAMS + ("all_densities",) if getattr(m, name).grad is not None)
        image, depth = _stride3(_t("depth_map"))
        pts = _t("depth_pts").to(DEV).requires_grad_(True)
        x, idx = m.sample_points_in_gaussians(n, sampling_scale_factor=1.5, mask=_t("sample_mask").to(DEV))
        backward_of((x * _t("sample_w").to(DEV)).sum())
        axis = m.get_normals()
        backward_of((axis * _t("axis_w").to(DEV)).sum())
        z = m.get_points_depth_in_depth_map(fov_camera, depth, pts)
        backward_of((z * _t("depth_w").to(DEV)).sum())
        xf, f = _field_call(m, n)
        backward_of(_functional(f, n, 16, lambda t: t.to(DEV)))
        exact += [x, idx, axis, z, f["density"], f["sdf"], f["beta"], f["closest_gaussian_opacities"], xf.grad, pts.grad]
        assert len(exact) == 3 + 1 + 0 + 4 + 10
        results.append(([t.detach().as_subclass(torch.Tensor).clone() for t in exact], image.grad.clone()))
    for i, (a, b) in enumerate(zip(results[0][0], results[1][0])):
        assert torch.equal(a, b), i
    _check("depth map gradient, the two stacks", results[1][1], results[0][1], 1e-6)      # float atomics: equal up to the order of the adds
