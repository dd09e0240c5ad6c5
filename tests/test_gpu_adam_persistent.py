"""GPU tests of the persistent form of the zero-gradient SH-Adam half (csrc/sh_adam_update.h: sgr_sh_adam_zero_persistent): n_adam
waves, wave w over the 64-Gaussian blocks w, w + n_adam, ..., loads of the next round in flight while the current one is computed.
Through sgr_sh_adam_zero_grad_persistent every unflagged row must carry the bits of the dense sgr_sh_adam_from_views (whose colour
gradient is +0 there) and every flagged row the bits it had; through the trainer, a step with the ride-along equals a step without."""
import ctypes as C

import numpy as np
import pytest
import torch

from sugar_amd import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
LR_DC, LR_REST, B1, B2, EPS = 0.0025, 0.0025 / 20.0, 0.9, 0.999, 1e-15
PATTERNS = ("none", "all", "alternating", "blocks", "first_rows", "seeded20")
# n_adam = 8: waves with 3 or 4 blocks and a last block of 17 rows (prologue, steady state and epilogue of the pipeline all run);
# waves with 0 or 1 block; waves with 1 or 2 blocks and a last block of one row; one row
SHAPES = [(64 * (8 * 3 + 5) + 17, 8), (64 * (8 * 3 + 5) + 17, 16), (64 * 3, 8), (64 * 12 + 1, 8), (1, 8)]


def _lib():
    from sugar_amd import _lib
    return _lib.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _flags(P, pattern):
    f = np.zeros(P, np.uint8)
    if pattern == "all":
        f[:] = 1
    elif pattern == "alternating":
        f[::2] = 1
    elif pattern == "blocks":          # whole blocks set among unset ones: a wave's only, second and last block (n_adam = 8)
        for b in (1, 9, 26):
            f[64 * b: 64 * b + 64] = 1
    elif pattern == "first_rows":      # the first row of every block: the redirect target moves to the block's second row
        f[::64] = 1
        f[65::128] = 1                 # ... and to its third in every other block
    elif pattern == "seeded20":
        f[np.random.default_rng(20).random(P) < 0.2] = 1
    return f


def _inputs(P, flags, seed):
    """unflagged rows: colour gradient +0; flagged rows: seeded.  Moments with 0, -0.0, 1e-40 and v = 0, m != 0."""
    g = np.random.default_rng(seed)
    means = g.standard_normal((P, 3)).astype(F)
    campos = np.array([[0.3, -2.5, 1.1]], F)
    dcolor = (g.standard_normal((P, 3)) * 1e-3).astype(F)
    dcolor[flags == 0] = 0
    sh = g.standard_normal((P, 16, 3)).astype(F)
    m = (g.standard_normal((P, 16, 3)) * 1e-4).astype(F)
    v = (g.random((P, 16, 3)) * 1e-7).astype(F)
    pick = g.integers(0, 6, (P, 16, 3))
    m[pick == 0] = 0
    m[pick == 1] = -0.0
    m[pick == 2] = 1e-40
    v[pick == 0] = 0
    v[pick == 2] = 1e-40
    v[pick == 3] = 0
    return means, campos, dcolor, sh, m, v


def _dense(P, ops, step, gs):
    means, campos, dcolor, sh, m, v = (_dev(a) for a in ops)
    rc = _lib().sgr_sh_adam_from_views(P, 1, 3, 16, means.data_ptr(), campos.data_ptr(), dcolor.data_ptr(), 0, sh.data_ptr(), m.data_ptr(),
                                       v.data_ptr(), LR_DC, LR_REST, B1, B2, EPS, step, gs, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    return sh, m, v


def _persistent(P, ops, flags, step, gs, header, cap, n_adam):
    sh, m, v = (_dev(a) for a in ops[3:])
    fl = _dev(flags)
    hp = header.data_ptr() if header is not None else None
    rc = _lib().sgr_sh_adam_zero_grad_persistent(P, 16, sh.data_ptr(), m.data_ptr(), v.data_ptr(), fl.data_ptr(), LR_DC, LR_REST, B1, B2, EPS,
                                                 step, gs, hp, cap, n_adam, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    return sh, m, v, fl


@pytest.mark.parametrize("P,n_adam", SHAPES)
def test_persistent_waves_equal_dense_bit_for_bit(P, n_adam):
    valid = torch.zeros(16, dtype=torch.int32, device=DEV)
    valid[0] = 5                              # R = 5 <= capacity 10, no hint miss, no level-1 overflow
    invalid = valid.clone()
    invalid[0] = 100                          # R = 100 > capacity 10
    moved = False
    for pi, pattern in enumerate(PATTERNS):
        flags = _flags(P, pattern)
        keep = torch.from_numpy(flags != 0)
        ops = _inputs(P, flags, 1000 * P + pi)
        for step, gs in ((1, 1.0), (1000, 0.5)):
            want = _dense(P, ops, step, gs)
            got = _persistent(P, ops, flags, step, gs, valid if gs == 1.0 else None, 10, n_adam)
            for name, a, b, before in zip(("sh", "exp_avg", "exp_avg_sq"), got, want, ops[3:]):
                a, b = a.cpu().view(torch.int32), b.cpu().view(torch.int32)
                assert torch.equal(a[~keep], b[~keep]), (P, pattern, step, gs, name, "unflagged rows differ from the dense kernel")
                assert torch.equal(a[keep], torch.from_numpy(before).view(torch.int32)[keep]), (P, pattern, step, gs, name, "a flagged row moved")
                moved |= bool((~keep).any()) and not torch.equal(b[~keep], torch.from_numpy(before).view(torch.int32)[~keep])
            assert np.array_equal(got[3].cpu().numpy(), flags)   # the zero half only reads the flags
        sh, m, v, fl = _persistent(P, ops, flags, 1, 1.0, invalid, 10, n_adam)
        for a, b in zip((sh, m, v), ops[3:]):
            assert np.array_equal(_bits(a), b.view(np.uint32)), (P, pattern, "an invalid forward's optimiser step wrote")
    assert moved                              # (the comparison above is not between two no-ops)


def test_persistent_entry_point_checks_its_arguments():
    lib = _lib()
    P = 65
    flags = _flags(P, "alternating")
    ops = _inputs(P, flags, 3)
    sh, m, v = (_dev(a) for a in ops[3:])
    fl = _dev(flags)
    before = _bits(sh).copy()
    call = lambda M, n, p_sh: lib.sgr_sh_adam_zero_grad_persistent(P - 1, M, p_sh, m.data_ptr(), v.data_ptr(), fl.data_ptr(), LR_DC, LR_REST, B1,
                                                                  B2, EPS, 1, 1.0, None, 0, n, _stream())
    assert call(9, 8, sh.data_ptr()) == -1        # M != 16
    assert call(16, 8, sh.data_ptr() + 4) == -1   # unaligned
    assert call(16, 0, sh.data_ptr()) == -1       # n_adam: a multiple of 8 from 8 on
    assert call(16, 12, sh.data_ptr()) == -1
    torch.cuda.synchronize()
    assert np.array_equal(_bits(sh), before)


# ---- through the trainer: tests/test_gpu_adam_overlap.py's ride-along case, with eight persistent workgroups (59 blocks each) ------
W, H = 400, 240


def _close(a, b, start):
    """the bar of tests/test_gpu_native_trainer.py"""
    upd = float((b - start).abs().max())
    assert upd > 1e-4
    assert float(((a - b).abs() > 1e-2 * upd).float().mean()) < 1e-4
    assert float((a - b).norm() / (b - start).norm()) < 1e-3


@pytest.mark.parametrize("waves", ["8", None])
def test_a_step_with_the_persistent_ride_along_equals_a_step_without(monkeypatch, waves):
    from sugar_amd.train_step import GaussianParams, NativeTrainer
    lib = _lib()
    if waves is None:
        monkeypatch.delenv("SGR_ADAM_OVERLAP_WAVES", raising=False)   # the default: more workgroups than this scene has blocks
    else:
        monkeypatch.setenv("SGR_ADAM_OVERLAP_WAVES", waves)
    mode_before = lib.sgr_get_adam_overlap()
    try:
        dev = torch.device(DEV)
        scene = syn.make_scene(30000, 5, 0.01, 0.06)
        cams = [c._replace(viewmatrix=c.viewmatrix.to(dev), projmatrix=c.projmatrix.to(dev), campos=c.campos.to(dev))
                for c in syn.orbit_cameras(W, H)]
        gts = [torch.rand(3, H, W, generator=torch.Generator().manual_seed(i)).to(DEV) for i in range(4)]
        p = GaussianParams(scene, dev)
        start = p.flat.clone()
        lib.sgr_set_adam_overlap(1)
        nt = NativeTrainer(p, torch.zeros(3), W, H)
        off_b = int(lib.sgr_geom_reach_offset_bytes(p.P))
        table = nt._geom[off_b: off_b + p.P]
        for i in range(3):
            nt.step(cams[i], gts[i], cam_key=i)
        nt.synchronize()
        assert not table.any()
        snap = (p.flat.clone(), nt.exp_avg.clone(), nt.exp_avg_sq.clone(), nt.t)

        def one_step(mode):
            lib.sgr_set_adam_overlap(mode)
            with torch.no_grad():
                p.flat.copy_(snap[0]); nt.exp_avg.copy_(snap[1]); nt.exp_avg_sq.copy_(snap[2])
            nt.t = snap[3]
            table.zero_()
            nt.step(cams[3], gts[3], cam_key=3)
            nt.synchronize()
            assert nt.redone == 0
            return p.flat.clone(), nt.exp_avg.clone(), nt.exp_avg_sq.clone(), table.clone()

        one_step(0)                            # (leaves camera 3 its walk hint: the runs below are all hinted)
        off = one_step(0)
        flagged = one_step(2)[3] != 0          # which rows this step's forward flags
        on = one_step(1)
        assert not on[3].any()
        rows = ~flagged
        assert 0.05 < float(rows.float().mean()) < 0.95
        sh = lambda t: p.split_flat(t)["features"].reshape(p.P, 48)
        for a, b in zip(on[:3], off[:3]):      # unflagged rows: parameters and both moments of the SH block, bit for bit
            assert torch.equal(sh(a)[rows].view(torch.int32), sh(b)[rows].view(torch.int32))
        assert not torch.equal(sh(on[0])[rows], sh(snap[0])[rows])
        _close(on[0], off[0], start)           # every parameter (the flagged rows' gradients come from float atomics)
    finally:
        lib.sgr_set_adam_overlap(mode_before)
