"""CPU test of the float64 reference of the backward preprocess (oracle/torch_cpu_rasterizer.py::preprocess_backward_ref) against
the float32 C oracle (orc_preprocess_backward) on the scene of tests/bwd_rows_utils.py, with injected sums.

It asserts that the scene holds every group of rows the GPU test (tests/test_gpu_preprocess_bwd_rows.py) relies on, prints the
float32 oracle's per-row error distribution -- the yardstick of the GPU test, which recomputes it the same way --, and checks two
facts that need no GPU: far from det = 0 the 1e-7 term of the conic backward is invisible, and a reference WITHOUT the
clamp-as-constant rule differs from the oracle by more than 1e-2 on the clamped rows (the scene can see that branch).

Bounds on the oracle's own error (float32 against float64; derived, not fitted): a row is the result of a few hundred float32
operations, 2^-24 each, so the median row lies within 1e-5 of its largest entry; cancellation (needles, sub-pixel Gaussians, whose
cov2D is 0.3 I plus a difference of large terms) costs the worst row up to two more orders: 1e-3.  A wrong branch moves a row by
order 1."""
import functools

import numpy as np
import pytest
import torch

from oracle import torch_cpu_rasterizer as tcr
from tests import bwd_rows_utils as br

MODES = {"nonraw": dict(raw=False), "raw": dict(raw=True), "cov3D": dict(raw=False, cov=True),
         "colors": dict(raw=False, mode="colors"), "scale_modifier": dict(raw=False, scale_modifier=0.7)}
WORST, MEDIAN = 1e-3, 1e-5


@functools.lru_cache(maxsize=None)
def _case(mode, cam_i=0):
    opts = dict(MODES[mode])
    raw = opts.pop("raw")
    sc = br.scene()
    kw = br.inputs(sc, br.camera(cam_i), raw=raw, **opts)
    st, rec = br.oracle_forward(sc, kw, raw)
    ref = tcr.preprocess_backward_ref(rec, sc.sums, raw=raw, **kw)
    got = br.oracle_rows(sc, kw, raw, st, rec, sc.sums)
    return sc, kw, raw, st, rec, ref, got


def _view(sc, cam):
    """float64 (t.x / t.z) / (1.3 tanfovx), (t.y / t.z) / (1.3 tanfovy), t.z"""
    V = cam.viewmatrix.double().numpy()
    t = sc.means3D.astype(np.float64) @ V[:3, :3] + V[3, :3]
    return t[:, 0] / t[:, 2] / (1.3 * cam.tanfovx), t[:, 1] / t[:, 2] / (1.3 * cam.tanfovy), t[:, 2]


def test_the_scene_holds_every_group_among_the_rendered_rows():
    sc = br.scene()
    cam = br.camera(0)
    assert sc.means3D.shape[0] == br.P_FULL == 1010
    rx, ry, tz = _view(sc, cam)
    for mode in ("nonraw", "raw"):
        rec = _case(mode)[4]
        vis = rec["radii"] > 0
        n = lambda m: int((vis & m).sum())
        ox, oy = np.abs(rx) > 1, np.abs(ry) > 1
        counts = dict(x_only=n(ox & ~oy), y_only=n(oy & ~ox), both=n(ox & oy))
        print(mode, "rendered", int(vis.sum()), counts)
        assert counts["x_only"] >= 16 and counts["y_only"] >= 16 and counts["both"] >= 8
        for r in (rx, ry):  # both signs of each among the rows clamped in both
            assert n(ox & oy & (r > 1)) >= 2 and n(ox & oy & (r < -1)) >= 2
        # no rendered row so close to the limit that float32 and float64 could take different sides of the branch
        assert np.abs(np.abs(np.stack([rx, ry])[:, vis]) - 1).min() > 1e-3
        bits = (rec["clamped"] * np.array([1, 2, 4])).sum(1)
        per_combo = [n(bits == k) for k in range(8)]
        print(mode, "clamp-bit combinations", per_combo)
        assert min(per_combo) >= 8
        ratio = sc.scales.max(1) / sc.scales.min(1)
        assert n(ratio >= 999) >= 16
        assert n(tz < 0.4) >= 8 and tz[vis].min() > 0.2
        assert len(sc.groups["opac12"]) == 16 and np.allclose(np.abs(sc.raw_opac[sc.groups["opac12"]]), 12)
        one, neg = br.special_rows(sc)
        assert all(n(np.isin(np.arange(br.P_FULL), rows)) >= 4 for rows in one), [len(r) for r in one]
        assert n(np.isin(np.arange(br.P_FULL), neg)) >= 8
        assert 0.25 <= 1 - br.touched(sc.sums).mean() <= 0.40
        assert br.touched(sc.sums)[np.concatenate([sc.groups[k] for k, _ in br.GROUPS])].all()
    # sub-pixel: cov2D within 1e-3 of 0.3 I; the colour group: every channel at least 1e-3 away from its clamp
    kw = _case("nonraw")[1]
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64))
    pp = tcr.preprocess(t(kw["means3D"]), shs=t(kw["shs"]), scales=t(kw["scales"]), rotations=t(kw["rotations"]),
                        viewmatrix=t(kw["viewmatrix"]), projmatrix=t(kw["projmatrix"]), campos=t(kw["campos"]), W=br.W, H=br.H,
                        tanfovx=kw["tanfovx"], tanfovy=kw["tanfovy"])
    vis = _case("nonraw")[4]["radii"] > 0
    sub = (pp["cov2"].numpy() - np.array([0.3, 0.0, 0.3])[None]).__abs__().max(1) < 1e-3
    assert int((vis & sub).sum()) >= 16
    assert np.abs(pp["color_unclamped"].numpy()[sc.groups["colour"]]).min() >= 1e-3
    # raw mode: quaternion norms over six decades, exact zeros among the rendered; non-raw: norms in 0.9 .. 1.1, not 1
    nq = np.linalg.norm(sc.raw_rot.astype(np.float64), axis=1)
    vis = _case("raw")[4]["radii"] > 0
    assert int((vis & (nq == 0)).sum()) >= 4
    assert nq[nq > 0].min() < 2e-3 and nq.max() > 5e2
    ng = np.linalg.norm(sc.rot_given.astype(np.float64), axis=1)
    assert ng.min() >= 0.899 and ng.max() <= 1.101 and np.abs(ng - 1).max() > 0.09
    assert not np.array_equal(br.scene(False).means3D, sc.means3D)  # (the block-ordered variant is another order of the same rows)
    assert np.array_equal(np.sort(br.scene(False).means3D, axis=0), np.sort(sc.means3D, axis=0))


@pytest.mark.parametrize("mode", list(MODES))
def test_float32_oracle_against_the_float64_reference(mode):
    """every rendered, touched row; prints the yardstick of the GPU test"""
    sc, kw, raw, st, rec, ref, got = _case(mode)
    rows = np.flatnonzero((rec["radii"] > 0) & br.touched(sc.sums))
    dead = np.flatnonzero(~((rec["radii"] > 0) & br.touched(sc.sums)))
    assert len(rows) > 500
    for k in br.GRADS + ("opacity",):
        if k not in got:
            continue
        assert k in ref
        assert np.isfinite(ref[k]).all() and np.isfinite(got[k]).all(), k
        err, at = br.row_err(got[k], ref[k], rows)
        print(br.describe(f"{mode} oracle dL_d{k}", err))
        assert err.max() <= WORST, (k, at[np.argsort(err)[-5:]], np.sort(err)[-5:])
        assert np.median(err) <= MEDIAN, k
        assert not ref[k].reshape(br.P_FULL, -1)[dead].any() and not got[k].reshape(br.P_FULL, -1)[dead].any(), k


def test_second_camera():
    sc, kw, raw, st, rec, ref, got = _case("nonraw", 3)
    rows = np.flatnonzero((rec["radii"] > 0) & br.touched(sc.sums))
    for k in ("mean3D", "scale", "rot", "sh"):
        err, at = br.row_err(got[k], ref[k], rows)
        print(br.describe(f"camera 3 oracle dL_d{k}", err))
        assert err.max() <= WORST and np.median(err) <= MEDIAN, k


def test_the_1e7_term_is_invisible_far_from_det_zero_and_visible_on_sub_pixel_rows():
    sc, kw, raw, st, rec, ref, _ = _case("nonraw")
    no_eps = tcr.preprocess_backward_ref(rec, sc.sums, raw=raw, eps_term=False, **kw)
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64))
    det = tcr.preprocess(t(kw["means3D"]), shs=t(kw["shs"]), scales=t(kw["scales"]), rotations=t(kw["rotations"]),
                         viewmatrix=t(kw["viewmatrix"]), projmatrix=t(kw["projmatrix"]), campos=t(kw["campos"]), W=br.W, H=br.H,
                         tanfovx=kw["tanfovx"], tanfovy=kw["tanfovy"])["det"].numpy()
    live = (rec["radii"] > 0) & (np.abs(sc.sums[:, 6:9]) > 0).any(1)
    far = np.flatnonzero(live & (det > 10.0))     # the factor is 1 - 1e-7 / det^2: below 1e-9 here
    sub = np.flatnonzero(live & np.isin(np.arange(br.P_FULL), sc.groups["subpixel"]))  # det ~ 0.09: 1.2e-5
    assert len(far) > 100 and len(sub) >= 8
    for k in ("scale", "rot"):
        e_far, _ = br.row_err(no_eps[k], ref[k], far)
        e_sub, _ = br.row_err(no_eps[k], ref[k], sub)
        print(k, "far", e_far.max(), "sub-pixel", e_sub.min(), e_sub.max())
        assert e_far.max() < 2e-9
        assert e_sub.min() > 5e-6 and e_sub.max() < 2e-5


def test_without_the_clamp_as_constant_rule_the_clamped_rows_differ():
    """The scene sees the x_grad_mul / y_grad_mul branch.  A reference that lets the gradient pass to the clamped t.x / t.y is
    more than 1e-2 away from the oracle on every clamped row that carries one conic sum alone (32 rows; measured 0.012 .. 0.99,
    median 0.35).  On the clamped rows with all nine sums the mean2D path, 0.5 W times larger, dominates dL_dmean3D (measured
    4e-6 .. 6e-3, median 5e-4): there the median distance is still more than 100 times the oracle's worst such row.  All other
    rows and tensors are unchanged."""
    sc, kw, raw, st, rec, ref, got = _case("nonraw")
    loose = tcr.preprocess_backward_ref(rec, sc.sums, raw=raw, clamp_as_constant=False, **kw)
    rx, ry, _ = _view(sc, br.camera(0))
    live = (rec["radii"] > 0) & br.touched(sc.sums)
    out = (np.abs(rx) > 1) | (np.abs(ry) > 1)
    only = np.isin(np.arange(br.P_FULL), br.conic_only_rows(sc))
    assert not (only & ~out).any() and not (only & ~live).any() and int(only.sum()) == 32
    err, _ = br.row_err(got["mean3D"], loose["mean3D"], np.flatnonzero(only))
    print(br.describe("clamp rule removed, clamped rows with one conic sum alone", err), "min", err.min())
    assert len(err) == 32 and err.min() > 1e-2
    rows = np.flatnonzero(live & out & ~only)
    assert len(rows) >= 32
    err, _ = br.row_err(got["mean3D"], loose["mean3D"], rows)
    print(br.describe("clamp rule removed, clamped rows with all nine sums", err))
    worst, _ = br.row_err(got["mean3D"], ref["mean3D"], rows)
    assert np.median(err) > 100 * worst.max()
    inside = np.flatnonzero(live & ~out)
    assert np.array_equal(loose["mean3D"][inside], ref["mean3D"][inside])
    for k in ("scale", "rot", "sh"):  # (the rule only concerns the mean)
        assert np.array_equal(loose[k], ref[k]), k
