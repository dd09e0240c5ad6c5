"""GPU tests of the backward preprocess's zero-row exit (a rendered Gaussian the blend backward never reached gets zero rows
without its parameters being read), of the verification switch SGR_BWD_DENSE, and of the self-cleaning accumulator table
(SGR_BWD_ACC_CLEAN: the trainer no longer resets 64 B per Gaussian every step).

Scenes: synthetic config1 at 256x256 with P = 60 013 (about a fifth of the visible rows touched; not a multiple of 64, 256 or
any 256 K), 10 000 (most rows touched) and 37 (less than one wave), and one constructed scene of 4 096 + 64 + 5 Gaussians: a
whole workgroup tile of rendered-but-transparent Gaussians (opacity 1e-3 < 1/255: never blended), then 64 that all contribute.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import cpu_oracle as orc
from sugar_amd import synthetic as syn
from tests import parity_utils as pu

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W = H = 256
SIZES = (60013, 10000, 37)
CAMS = (0, 3)
N_TILE = 4096  # Gaussians of the constructed scene's transparent run
N_SUB = 8      # transparent Gaussians of the constructed sub-wave scene


@functools.lru_cache(maxsize=None)
def _scene(P):
    if P == "sub":
        # less than one wave WITH zero rows (config1 at P = 37 has none: all 37 are touched): the first eight transparent
        scene, cams, bg = syn.make_config("config1", P=37)
        opac = scene.opacities.clone()
        opac[:N_SUB] = 1e-3
        return scene._replace(opacities=opac), cams, bg
    if P != "built":
        scene, cams, bg = syn.make_config("config1", P=P)
        return scene, cams, bg
    scene, cams, bg = syn.make_config("config1", P=N_TILE + 64 + 5)
    means, scales, opac = scene.means3D.clone(), scene.scales.clone(), scene.opacities.clone()
    opac[:N_TILE] = 1e-3
    # a 4 x 4 x 4 lattice around the origin (every orbit camera looks at it): small, half transparent, so that even the ones
    # behind three others still receive T >= 1/8
    g = torch.arange(4, dtype=torch.float32) * 0.15 - 0.225
    means[N_TILE:N_TILE + 64] = torch.stack(torch.meshgrid(g, g, g, indexing="ij"), dim=-1).reshape(64, 3)
    scales[N_TILE:N_TILE + 64] = 0.02
    opac[N_TILE:N_TILE + 64] = 0.5
    return scene._replace(means3D=means, scales=scales, opacities=opac), cams, bg


_grad_image = lambda: pu.grad_image(W, H)
_Run = pu.Run   # one forward through the C ABI, and backwards over its scratch (shared with tests/test_gpu_preprocess_bwd_rows.py)


@functools.lru_cache(maxsize=None)
def _oracle(P, cam_i):
    """(forward state, gradients, rendered mask, rows the oracle's blend backward left untouched); computed once per case"""
    scene, cams, bg = _scene(P)
    st = pu.run_oracle(scene, cams[cam_i], bg)
    gr = orc.backward(st, _grad_image())
    n = scene.means3D.shape[0]
    touched = np.zeros(n, bool)
    for k in ("dL_dcolors", "dL_dopacity", "dL_dmeans2D", "dL_dconic"):
        touched |= (gr[k].reshape(n, -1) != 0).any(axis=1)
    vis = st["radii"] > 0
    return st, gr, vis, vis & ~touched


ORACLE_NAMES = dict(mean2D="dL_dmeans2D", opacity="dL_dopacity", mean3D="dL_dmeans3D", scale="dL_dscales", rot="dL_drotations",
                    sh="dL_dsh", color="dL_dcolors")


def _zero_share(P, cam_i):
    _, _, vis, zero = _oracle(P, cam_i)
    return zero.sum() / max(int(vis.sum()), 1)


def _check_against_oracle(P, cam_i, store_sh):
    """No case is skipped: where the oracle has no zero rows (P = 37) the zero-row assertion is empty and everything else holds."""
    scene, cams, bg = _scene(P)
    st, gr, vis, zero = _oracle(P, cam_i)
    print(f"P={P} camera {cam_i}: visible {int(vis.sum())}, untouched in the oracle {int(zero.sum())} ({100 * _zero_share(P, cam_i):.1f} %)")
    run = _Run(scene, cams[cam_i], bg, raw=False)
    assert run.R == st["num_rendered"] and np.array_equal(run.radii.cpu().numpy(), st["radii"])
    out = {k: v.cpu().numpy() for k, v in run.backward(0, store_sh).items()}
    n = scene.means3D.shape[0]
    # every row the oracle's blend backward left untouched is exactly zero in every output
    for k in ("mean2D", "conic", "opacity", "color", "mean3D", "scale", "rot") + (("sh",) if store_sh else ()):
        assert not out[k].reshape(n, -1)[zero].any(), k
    # the tolerances of tests/test_gpu_parity.py for these tensors
    for k, name in ORACLE_NAMES.items():
        if k not in out:
            continue
        ref = gr[name]
        if k == "color" and not store_sh:  # compact mode: the clamp-masked colour gradients
            ref = np.where(st["clamped"].astype(bool), 0.0, ref).astype(np.float32)
        v = out[k]
        e = pu.rel_stats(v.reshape(ref.shape), ref)
        print(k, e)
        assert e["norm_rel"] <= 1e-4 and e["frac_gt_1e4"] <= max(1e-3, 30.0 / v.size), (k, e)
    ref = gr["dL_dconic"].reshape(n, 4)[:, [0, 1, 3]]
    e = pu.rel_stats(out["conic"][:, [0, 1, 3]], ref)
    assert e["norm_rel"] <= 1e-4 and e["frac_gt_1e4"] <= max(1e-3, 30.0 / ref.size), ("conic", e)
    # the statistics count every rendered row once, touched or not
    assert np.array_equal(out["denom"], vis.astype(np.float32))
    assert np.array_equal(out["max_radii"], np.where(vis, np.maximum(2.0, st["radii"]), 2.0).astype(np.float32))
    assert not out["accum"][zero | ~vis].any()
    return out, zero


@pytest.mark.parametrize("store_sh", (False, True))
@pytest.mark.parametrize("cam_i", CAMS)
@pytest.mark.parametrize("P", SIZES + ("sub",))
def test_zero_rows_and_touched_rows_against_the_oracle(P, cam_i, store_sh):
    _check_against_oracle(P, cam_i, store_sh)


def test_the_zero_row_assertions_are_not_empty():
    """Between 5 % and 95 % of the visible rows are zero rows in the oracle for the two large sizes at both cameras and for the
    constructed sub-wave scene, so both kinds of row are compared there.  (From the oracle alone: does not depend on which other
    tests ran, or in which order.  config1 at P = 37 has no zero row at either camera; it is compared all the same.)"""
    for P in (60013, 10000, "sub"):
        for cam_i in CAMS:
            assert 0.05 <= _zero_share(P, cam_i) <= 0.95, (P, cam_i, _zero_share(P, cam_i))


@pytest.mark.parametrize("store_sh", (False, True))
def test_a_whole_tile_of_zero_rows_then_a_wave_of_touched_ones(store_sh):
    out, zero = _check_against_oracle("built", 0, store_sh)
    vis = _oracle("built", 0)[2]
    assert vis[:N_TILE].sum() > 256 * 8  # (rendered: whole workgroup tiles of them)
    assert zero[:N_TILE][vis[:N_TILE]].all()
    for k in ("opacity", "mean3D", "scale", "rot", "color"):
        assert not out[k][:N_TILE].reshape(N_TILE, -1).any(), k
    assert np.array_equal(out["denom"][:N_TILE], vis[:N_TILE].astype(np.float32))
    assert vis[N_TILE:N_TILE + 64].all() and (out["opacity"][N_TILE:N_TILE + 64] != 0).all()


@pytest.mark.parametrize("raw", (False, True))
@pytest.mark.parametrize("store_sh", (False, True))
@pytest.mark.parametrize("cam_i", CAMS)
@pytest.mark.parametrize("P", SIZES + ("built", "sub"))
def test_sparse_path_equals_the_dense_switch(P, cam_i, store_sh, raw):
    """same forward, same accumulator contents (the blend backward runs ONCE, the preprocess half twice): equal outputs"""
    from sugar_amd import _lib
    scene, cams, bg = _scene(P)
    run = _Run(scene, cams[cam_i], bg, raw=raw)
    run.backward(1, False, stats=False)
    acc0 = run.acc().clone()
    sparse = run.backward(2, store_sh)
    assert torch.equal(run.acc(), acc0)  # (without SGR_BWD_ACC_CLEAN the table is read only)
    dense = run.backward(2, store_sh, flags=_lib.SGR_BWD_DENSE)
    vis = run.radii > 0
    n_zero = int((vis & ~(acc0[:, :9] != 0).any(dim=1)).sum())
    print(f"P={P} camera {cam_i}: rendered {int(vis.sum())}, zero rows {n_zero}")
    assert set(sparse) == set(dense)
    for k in sparse:
        assert not torch.isnan(sparse[k]).any(), k
        assert torch.equal(sparse[k], dense[k]), k
    assert torch.equal(sparse["denom"], vis.float())
    # ... and with the cleaning on: same outputs, and the table is zero afterwards
    clean = run.backward(2, store_sh, flags=_lib.SGR_BWD_ACC_CLEAN)
    for k in sparse:
        assert torch.equal(sparse[k], clean[k]), k
    assert not run.acc().view(torch.int32).any()


def _device_cams():
    dev = torch.device(DEV)
    return [c._replace(viewmatrix=c.viewmatrix.to(dev), projmatrix=c.projmatrix.to(dev), campos=c.campos.to(dev))
            for c in syn.orbit_cameras(W, H)]


def _close(a, b, start, least=1e-4):
    """two runs of the same steps: equal up to the float-atomic order of the blend backward (the rule of
    tests/test_gpu_native_trainer.py; `least`: what the largest change must exceed -- parameters move by a learning rate per
    step, Adam's second moments are squares of gradients of 1e-4 and smaller)"""
    upd = float((b - start).abs().max())
    assert upd > least
    assert float(((a - b).abs() > 1e-2 * upd).float().mean()) < 1e-4
    assert float((a - b).norm() / (b - start).norm()) < 1e-3


def _acc_of(nt):
    o = nt._lib.sgr_geom_acc_offset_bytes(nt.params.P)
    return nt._geom[o:o + nt.params.P * 64].view(torch.int32)


def test_trainer_keeps_the_accumulator_clean_and_trains_the_same():
    """three native steps at P = 60 013: the table is all zero after each, and the training equals the autograd trainer's, whose
    backward resets the table on every call"""
    from sugar_amd.diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    from sugar_amd.train_step import GaussianParams, NativeTrainer, ViewShardedTrainer
    dev = torch.device(DEV)
    scene = _scene(60013)[0]
    cams = _device_cams()
    gts = [torch.rand(3, H, W, generator=torch.Generator().manual_seed(i)).to(dev) for i in range(3)]
    pa = GaussianParams(scene, dev)
    start = pa.flat.clone()
    ref = ViewShardedTrainer(pa, GaussianRasterizer, GaussianRasterizationSettings, torch.zeros(3, device=dev))
    for i in range(3):
        ref.step(cams[i], gts[i])
    pb = GaussianParams(scene, dev)
    nt = NativeTrainer(pb, torch.zeros(3), W, H, densify_stats=True)
    assert nt._lib.sgr_trainer_acc_dirty(nt._h) == 1   # a fresh trainer resets the table itself, once
    for i in range(3):
        nt.step(cams[i], gts[i], cam_key=i)
        nt.synchronize()
        assert nt.redone == 0
        assert nt._lib.sgr_trainer_acc_dirty(nt._h) == 0
        assert not _acc_of(nt).any()
    assert float(nt.denom.max()) == 3.0
    _close(pb.flat, pa.flat, start)
    n = pa.n_small
    z = torch.zeros_like(start)
    _close(nt.exp_avg[:n], ref.opt.exp_avg[:n], z[:n], least=0.0)
    _close(nt.exp_avg_sq[:n], ref.opt.exp_avg_sq[:n], z[:n], least=0.0)


def test_an_invalid_forward_leaves_the_accumulator_clean_and_the_repeated_step_matches():
    from sugar_amd.train_step import GaussianParams, NativeTrainer
    dev = torch.device(DEV)
    scene = _scene(60013)[0]
    cams = _device_cams()
    gt = torch.rand(3, H, W, generator=torch.Generator().manual_seed(0)).to(dev)
    flats = []
    for capacity in (None, 1000):
        p = GaussianParams(scene, dev)
        start = p.flat.clone()
        nt = NativeTrainer(p, torch.zeros(3), W, H, capacity=capacity)
        nt.step(cams[0], gt, cam_key=0)   # (capacity 1000: the list does not fit, every kernel of the step is a no-op)
        torch.cuda.synchronize()
        assert not _acc_of(nt).any()
        if capacity:
            assert torch.equal(p.flat, start)
        nt.synchronize()                  # validates the step and repeats it with a larger list
        assert nt.redone == (1 if capacity else 0)
        assert not _acc_of(nt).any()
        nt.step(cams[1], gt, cam_key=1)
        nt.synchronize()
        assert not _acc_of(nt).any()
        flats.append(p.flat.clone())
    _close(flats[1], flats[0], start)


def test_a_step_that_stopped_between_the_two_halves_costs_the_next_one_a_reset():
    """the blend half alone leaves the table dirty and the trainer knows it: the next full step resets the table -- its flat
    gradient would hold every sum twice otherwise (Adam's first step moves a parameter by lr * sign(g) and would not show it) --
    and trains like a trainer that never stopped half-way"""
    from sugar_amd.train_step import GaussianParams, NativeTrainer
    dev = torch.device(DEV)
    scene = _scene(10000)[0]
    cams = _device_cams()
    gt = torch.rand(3, H, W, generator=torch.Generator().manual_seed(0)).to(dev)
    flats, grads = [], []
    for half in (False, True):
        p = GaussianParams(scene, dev)
        start = p.flat.clone()
        nt = NativeTrainer(p, torch.zeros(3), W, H)
        if half:
            nt._call(cams[0], gt, 0, 1, None)   # forward, loss and blend backward only
            torch.cuda.synchronize()
            assert nt._lib.sgr_trainer_acc_dirty(nt._h) == 1
            assert _acc_of(nt).any()
        nt.step(cams[0], gt, cam_key=0)
        nt.synchronize()
        assert nt._lib.sgr_trainer_acc_dirty(nt._h) == 0 and not _acc_of(nt).any()
        flats.append(p.flat.clone()); grads.append(p.flat_grad[: p.n_small].clone())
    # run-to-run float atomics move the gradient by ~1e-5 of its norm; sums counted twice would move it by its whole norm
    assert float(grads[0].norm()) > 0 and float((grads[1] - grads[0]).norm() / grads[0].norm()) < 1e-3
    _close(flats[1], flats[0], start)
