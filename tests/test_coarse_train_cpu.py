"""CPU tests of the native coarse-SDF trainer's host side (no kernel runs here):

  * the numpy Philox4x32-10 of tests/coarse_draw_restatement.py against the published known answers (Random123's kat_vectors), the
    index formula against `np.flatnonzero(mask)[j]`, and the restated normals' mean and variance;
  * `coarse_train.phase` at the schedule's boundaries and the positions' learning rate against get_expon_lr_func's formula;
  * the command's parser, the checkpoint's key names and shapes, `save_model` / `model_from` and `save_ply` on CPU tensors, `prune`
    with an optimiser's moments, the spatial extent, and the header's declarations of the new symbols."""
import math
import os
import re

import numpy as np
import pytest
import torch

from sugar_amd import coarse_model, coarse_train, io as sio
from tests import coarse_draw_restatement as cd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- the stream
@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, want):
    got = cd.philox4x32_10(counter, key).reshape(4)
    assert " ".join(f"{int(w):08x}" for w in got) == want


def test_sample_words_are_the_stated_counters():
    seed, call = 0x1234_5678_9ABC_DEF0, (3 << 32) + 5
    a, b = cd.sample_words(4, seed, call)
    key = (seed & 0xFFFFFFFF, seed >> 32)
    for n in range(4):
        assert np.array_equal(a[n], cd.philox4x32_10((2 * n, 0, 5, 3), key).reshape(4))
        assert np.array_equal(b[n], cd.philox4x32_10((2 * n + 1, 0, 5, 3), key).reshape(4))


def test_index_formula_picks_masked_rows_in_ascending_order():
    g = np.random.default_rng(0)
    mask = g.random(1000) < 0.3
    idx, noise, n_masked = cd.draw_samples(mask, 5000, 7, 2)
    ids = np.flatnonzero(mask)
    a, _ = cd.sample_words(5000, 7, 2)
    j = (a[:, 0].astype(np.uint64) * np.uint64(len(ids))) >> np.uint64(32)
    assert n_masked == len(ids) and j.max() < len(ids) and np.array_equal(idx, ids[j]) and mask[idx].all()
    assert set(np.unique(idx)) == set(ids)                                      # 5000 draws over ~300 rows reach every one
    r0 = np.array([0, 1, 2 ** 31, 2 ** 32 - 1], dtype=np.uint32)
    assert cd.pick(r0, 1).tolist() == [0, 0, 0, 0] and cd.pick(r0, 2).tolist() == [0, 0, 1, 1]
    assert cd.pick(r0, 2 ** 31 - 1).tolist() == [0, 0, 2 ** 30 - 1, 2 ** 31 - 2]
    empty = cd.draw_samples(np.zeros(10, bool), 7, 0, 0)
    assert empty[2] == 0 and not empty[0].any() and not empty[1].any()


def test_restated_normals_have_zero_mean_and_unit_variance():
    n = 100_000
    z = cd.normals(n, seed=11, call=4)
    assert z.shape == (n, 3) and np.isfinite(z).all()
    for c in range(3):
        assert abs(z[:, c].mean()) < 4 / math.sqrt(n) and abs(z[:, c].var() - 1.0) < 4 / math.sqrt(n), c
    assert abs(np.corrcoef(z.T)[0, 1]) < 4 / math.sqrt(n) and abs(np.corrcoef(z.T)[0, 2]) < 4 / math.sqrt(n)
    u = cd.unit_open(np.array([0, 2 ** 32 - 1], dtype=np.uint32), np.float64)
    assert u[0] == 2.0 ** -25 and u[1] == 1.0 - 2.0 ** -25                      # never 0 or 1 in exact arithmetic
    assert cd.unit_open(np.array([0], dtype=np.uint32), np.float32)[0] > 0


# -------------------------------------------------------------------------------------------------------------- the schedule
def test_phase_at_the_boundaries():
    ph = {it: coarse_train.phase(it) for it in (7000, 7001, 7500, 8999, 9000, 9001, 9500, 15000)}
    assert not any(ph[7000])                                                    # the checkpoint's own iteration: nothing yet
    assert [ph[it].entropy for it in ph] == [False, True, True, True, False, False, False, False]          # 7000 < it < 9000
    assert [ph[it].reset_neighbors for it in ph] == [False, True, True, False, True, False, True, True]    # 7001, then it % 500 == 0
    assert [ph[it].prune for it in ph] == [False] * 5 + [True, False, False]                               # the start of 9001
    assert [ph[it].reset_after_prune for it in ph] == [ph[it].prune for it in ph]
    for name in ("sdf", "sdf_estimation", "sdf_better_normal"):
        assert [getattr(ph[it], name) for it in ph] == [False] * 5 + [True] * 3, name                      # it > 9000
    assert not coarse_train.phase(9500, regularize_sdf=False).sdf and not coarse_train.phase(9500, regularize_sdf=False).reset_neighbors
    assert not coarse_train.phase(8000, enforce_entropy_regularization=False).entropy
    assert coarse_train.phase(9500, use_sdf_estimation_loss=False) == ph[9500]._replace(sdf_estimation=False)


def test_position_learning_rate_follows_the_formula():
    scale = 3.3
    for it in (1, 7001, 30_000):
        t = it / 30_000
        want = math.exp(math.log(0.00016 * scale) * (1 - t) + math.log(0.0000016 * scale) * t)
        assert coarse_train.position_lr(it, scale) == pytest.approx(want, rel=1e-12)
    assert coarse_train.position_lr(7001, scale, **coarse_train.DEFAULTS) == coarse_train.position_lr(7001, scale)   # as the trainer calls it
    assert coarse_train.position_lr(30_000, scale) == pytest.approx(0.0000016 * scale, rel=1e-12)
    assert coarse_train.position_lr(40_000, scale) == pytest.approx(0.0000016 * scale, rel=1e-12)        # clipped at max_steps
    assert coarse_train.expon_lr(-1, 1.0, 0.1) == 0.0 and coarse_train.expon_lr(5, 0.0, 0.0) == 0.0
    # with a delay (what 3DGS's own schedule may pass): the reverse-cosine factor
    assert coarse_train.expon_lr(50, 1.0, 1.0, lr_delay_steps=100, lr_delay_mult=0.01) == pytest.approx(
        0.01 + 0.99 * math.sin(0.25 * math.pi), rel=1e-12)


# --------------------------------------------------------------------------------------------------------- model and command
def _model(P=7, M=16, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    return coarse_model.CoarseModel(r(P, 3), r(P, 3), r(P, 4), r(P, 1), r(P, 1, 3), r(P, M - 1, 3))


def test_checkpoint_keys_shapes_and_round_trip(tmp_path):
    m = _model()
    state = m.state_dict()
    assert list(state) == ["_points", "all_densities", "_scales", "_quaternions", "_sh_coordinates_dc", "_sh_coordinates_rest"]
    assert [tuple(v.shape) for v in state.values()] == [(7, 3), (7, 1), (7, 3), (7, 4), (7, 1, 3), (7, 15, 3)]
    assert not any(v.requires_grad for v in state.values()) and all(p.requires_grad and p.is_leaf for p in m.parameters())
    path = str(tmp_path / "15000.pt")
    m.save_model(path, iteration=15000, train_losses=[0.5])
    ckpt = torch.load(path)
    assert set(ckpt) == {"state_dict", "iteration", "train_losses"} and ckpt["iteration"] == 15000
    back = coarse_model.CoarseModel.model_from(path)
    for k, v in back.state_dict().items():
        assert torch.equal(v, state[k]), k
    assert all(p.requires_grad and p.is_leaf for p in back.parameters())
    # the properties of a model that is not bound to a mesh
    assert torch.equal(m.scaling, torch.exp(m._scales)) and torch.equal(m.strengths, torch.sigmoid(m.all_densities))
    assert torch.allclose(m.quaternions.norm(dim=-1), torch.ones(7)) and m.sh_coordinates.shape == (7, 16, 3) and m.n_points == 7


def test_save_ply_is_what_the_extractor_reads(tmp_path):
    m = _model()
    path = str(tmp_path / "point_cloud.ply")
    m.save_ply(path)
    g = sio.load_gaussian_ply(path)
    assert torch.equal(g["xyz"], m._points.detach()) and torch.equal(g["scaling"], m._scales.detach())
    assert torch.equal(g["rotation"], m._quaternions.detach()) and torch.equal(g["opacity"], m.all_densities.detach())
    assert torch.equal(g["features"], m.sh_coordinates.detach())
    again = coarse_model.CoarseModel.from_gaussian_ply(path, device="cpu")
    for k, v in again.state_dict().items():
        assert torch.equal(v, m.state_dict()[k]), k


def test_prune_carries_the_adam_moments_of_the_kept_rows():
    m = _model(P=9)
    opt = torch.optim.Adam([{"params": [getattr(m, attr)], "lr": 0.01, "name": name} for name, attr in coarse_train.GROUPS], lr=0.0, eps=1e-15)
    for p in m.parameters():
        p.grad = torch.randn_like(p)
    opt.step()
    before = {name: (getattr(m, attr).detach().clone(), opt.state[getattr(m, attr)]["exp_avg"].clone(),
                     opt.state[getattr(m, attr)]["exp_avg_sq"].clone()) for name, attr in coarse_train.GROUPS}
    keep = torch.tensor([True, False, True, True, False, False, True, True, False])
    m.prune(keep, opt)
    assert m.n_points == 5 and m.knn_idx is None
    for group in opt.param_groups:
        p = group["params"][0]
        attr = dict(coarse_train.GROUPS)[group["name"]]
        assert p is getattr(m, attr) and p.is_leaf and p.requires_grad and p.grad is None
        value, m1, m2 = before[group["name"]]
        assert torch.equal(p.detach(), value[keep]) and torch.equal(opt.state[p]["exp_avg"], m1[keep])
        assert torch.equal(opt.state[p]["exp_avg_sq"], m2[keep]) and float(opt.state[p]["step"]) == 1.0
    assert len(opt.state) == 6
    for p in m.parameters():                                                    # the optimiser keeps working on the new leaves
        p.grad = torch.ones_like(p)
    opt.step()
    with pytest.raises(ValueError):
        m.prune(keep, opt)


def test_spatial_extent_is_the_reference_statement():
    centers = torch.tensor([[1.0, 0.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 3.0, 0.0], [0.0, -1.0, 0.0]])
    mean = centers.mean(dim=0, keepdim=True)
    assert coarse_model.spatial_extent(centers) == 1.1 * torch.norm(centers - mean, dim=-1).max().item()
    with pytest.raises(RuntimeError, match="no cameras"):
        _model().get_cameras_spatial_extent()


def test_unsupported_calls_raise_before_any_kernel():
    m = _model()
    x = torch.zeros(3, 3)
    with pytest.raises(NotImplementedError, match="return_sdf_grad"):
        m.get_field_values(x, torch.zeros(3, dtype=torch.int64), return_sdf_grad=True)
    with pytest.raises(NotImplementedError, match="gaussian_idx"):
        m.get_field_values(x)
    with pytest.raises(NotImplementedError, match="not implemented"):
        m.get_field_values(x, torch.zeros(3, dtype=torch.int64), gaussian_centers=x)
    for kw in (dict(), dict(return_full_matrix=True), dict(return_sqrt=True)):      # (the last: a model that is not on the device)
        with pytest.raises(NotImplementedError, match="get_covariance"):
            m.get_covariance(**kw)
    with pytest.raises(NotImplementedError, match="estimate_from_points"):
        m.get_normals(estimate_from_points=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        coarse_train.CoarseTrainer(m, [], [])
    with pytest.raises(TypeError, match="unknown options"):
        coarse_train.CoarseTrainer(m, [], [], no_such_option=1)


def test_parser_defaults_and_arguments():
    ap = coarse_train._parser()
    a = ap.parse_args(["pc.ply", "--cameras", "c.json", "--images", "im", "--out", "o"])
    assert (a.point_cloud, a.cameras, a.images, a.out) == ("pc.ply", "c.json", "im", "o")
    assert (a.iterations, a.start_iteration, a.estimation_factor, a.normal_factor, a.seed) == (15000, 7000, 0.2, 0.2, 0)
    a = ap.parse_args(["pc.ply", "--cameras", "c.json", "--images", "im", "--out", "o", "--iterations", "9013", "--start-iteration", "8990",
                       "--estimation-factor", "0.1", "--normal-factor", "0.3", "--seed", "5"])
    assert (a.iterations, a.start_iteration, a.estimation_factor, a.normal_factor, a.seed) == (9013, 8990, 0.1, 0.3, 5)
    with pytest.raises(SystemExit):
        ap.parse_args(["pc.ply"])


def test_defaults_are_the_reference_trainers():
    d = coarse_train.DEFAULTS
    assert (d["position_lr_init"], d["position_lr_final"], d["position_lr_max_steps"]) == (0.00016, 0.0000016, 30_000)
    assert (d["feature_lr"], d["opacity_lr"], d["scaling_lr"], d["rotation_lr"]) == (0.0025, 0.05, 0.005, 0.001)
    assert (d["dssim_factor"], d["entropy_regularization_factor"], d["estimation_factor"], d["normal_factor"]) == (0.2, 0.1, 0.2, 0.2)
    assert (d["n_samples_for_sdf_regularization"], d["sdf_sampling_scale_factor"], d["density_factor"]) == (1_000_000, 1.5, 1 / 16)
    assert [g for g, _ in coarse_train.GROUPS] == ["points", "sh_coordinates_dc", "sh_coordinates_rest", "all_densities", "scales", "quaternions"]


def test_header_declares_the_new_symbols():
    from sugar_amd import _lib
    src = open(os.path.join(ROOT, "include", "sugar_raster.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("sgr_draw_samples", "sgr_draw_samples_scratch_bytes", "sgr_opacity_entropy_forward", "sgr_opacity_entropy_backward",
                 "sgr_opacity_entropy_scratch_bytes"):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.SIGNATURES, name
    assert "Philox4x32-10" in src and "0xD2511F53" in src and "0xCD9E8D57" in src and "0x9E3779B9" in src and "0xBB67AE85" in src
    assert re.search(r"#define\s+SGR_ABI_VERSION\s+4\b", src)
