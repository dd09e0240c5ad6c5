"""GPU tests of SH-Adam split by reach flag (csrc/sh_adam_update.h): the forward blend flags every Gaussian the blend backward can
reach, the zero-gradient Adam step of the others rides in the blend backward's launch, the masked kernel updates the flagged ones
and clears the flags.  Together they must leave the bits of the dense kernel."""
import ctypes as C

import numpy as np
import pytest
import torch

from sugar_amd import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
LR_DC, LR_REST, B1, B2, EPS = 0.0025, 0.0025 / 20.0, 0.9, 0.999, 1e-15
PATTERNS = ("none", "all", "alternating", "seeded20", "row0", "last")


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
    elif pattern == "seeded20":
        f[np.random.default_rng(20).random(P) < 0.2] = 1
    elif pattern == "row0":
        f[0] = 1
    elif pattern == "last":
        f[-1] = 1
    return f


def _inputs(P, flags, seed):
    """unflagged rows: colour gradient +0; flagged rows: seeded, a third of them zero.  Moments with 0, -0.0, 1e-40 and v = 0, m != 0."""
    g = np.random.default_rng(seed)
    means = g.standard_normal((P, 3)).astype(F)
    campos = np.array([[0.3, -2.5, 1.1]], F)
    dcolor = (g.standard_normal((P, 3)) * 1e-3).astype(F)
    dcolor[g.random(P) < 0.33] = 0
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
    v[pick == 3] = 0          # (m != 0 there)
    return means, campos, dcolor, sh, m, v


def _dense(P, ops, step, gs):
    means, campos, dcolor, sh, m, v = (_dev(a) for a in ops)
    rc = _lib().sgr_sh_adam_from_views(P, 1, 3, 16, means.data_ptr(), campos.data_ptr(), dcolor.data_ptr(), 0, sh.data_ptr(), m.data_ptr(),
                                       v.data_ptr(), LR_DC, LR_REST, B1, B2, EPS, step, gs, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    return sh, m, v


def _split(P, ops, flags, step, gs, header, cap):
    means, campos, dcolor, sh, m, v = (_dev(a) for a in ops)
    fl = _dev(flags)
    hp = header.data_ptr() if header is not None else None
    lib = _lib()
    rc = lib.sgr_sh_adam_zero_grad(P, 16, sh.data_ptr(), m.data_ptr(), v.data_ptr(), fl.data_ptr(), LR_DC, LR_REST, B1, B2, EPS, step, gs, hp,
                                   cap, _stream())
    assert rc == 0
    rc = lib.sgr_sh_adam_from_views_masked(P, 1, 3, 16, means.data_ptr(), campos.data_ptr(), dcolor.data_ptr(), 0, sh.data_ptr(),
                                           m.data_ptr(), v.data_ptr(), LR_DC, LR_REST, B1, B2, EPS, step, gs, fl.data_ptr(), hp, cap, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    return sh, m, v, fl


@pytest.mark.parametrize("P", [1, 63, 64, 65, 209])
def test_split_equals_dense_bit_for_bit(P):
    """zero-gradient launch + masked launch == one dense sgr_sh_adam_from_views, on the uint32 views of sh, exp_avg and exp_avg_sq;
    the flags are all zero afterwards; an invalid forward in the guard makes both launches no-ops."""
    valid = torch.zeros(16, dtype=torch.int32, device=DEV)
    valid[0] = 5                              # R = 5 <= capacity 10, no hint miss, no level-1 overflow
    invalid = valid.clone()
    invalid[0] = 100                          # R = 100 > capacity 10
    for pi, pattern in enumerate(PATTERNS):
        flags = _flags(P, pattern)
        ops = _inputs(P, flags, 1000 * P + pi)
        for step in (1, 1000):
            for gs in (1.0, 0.5):
                want = _dense(P, ops, step, gs)
                got = _split(P, ops, flags, step, gs, valid if gs == 1.0 else None, 10)
                for name, a, b in zip(("sh", "exp_avg", "exp_avg_sq"), got, want):
                    assert np.array_equal(_bits(a), _bits(b)), (P, pattern, step, gs, name)
                assert not got[3].any(), (P, pattern, "flags left set")
        sh, m, v, fl = _split(P, ops, flags, 1, 1.0, invalid, 10)
        for a, b in zip((sh, m, v), ops[3:]):
            assert np.array_equal(_bits(a), b.view(np.uint32)), (P, pattern, "an invalid forward's optimiser step wrote")
        assert np.array_equal(fl.cpu().numpy(), flags)
    # the dense kernel's own update must have moved everything (the comparison above is not between two no-ops)
    assert not np.array_equal(_bits(want[0]), ops[3].view(np.uint32))


def test_the_split_needs_sixteen_aligned_coefficients():
    lib = _lib()
    P = 65
    flags = _flags(P, "alternating")
    means, campos, dcolor, sh, m, v = (_dev(a) for a in _inputs(P, flags, 3))
    fl = _dev(flags)
    before = _bits(sh).copy()
    assert lib.sgr_sh_adam_zero_grad(P, 9, sh.data_ptr(), m.data_ptr(), v.data_ptr(), fl.data_ptr(), LR_DC, LR_REST, B1, B2, EPS, 1, 1.0, None, 0,
                                     _stream()) == -1
    assert lib.sgr_sh_adam_from_views_masked(P, 1, 2, 9, means.data_ptr(), campos.data_ptr(), dcolor.data_ptr(), 0, sh.data_ptr(), m.data_ptr(),
                                             v.data_ptr(), LR_DC, LR_REST, B1, B2, EPS, 1, 1.0, fl.data_ptr(), None, 0, _stream()) == -1
    assert lib.sgr_sh_adam_zero_grad(P - 1, 16, sh.data_ptr() + 4, m.data_ptr(), v.data_ptr(), fl.data_ptr(), LR_DC, LR_REST, B1, B2, EPS, 1, 1.0,
                                     None, 0, _stream()) == -1
    torch.cuda.synchronize()
    assert np.array_equal(_bits(sh), before) and np.array_equal(fl.cpu().numpy(), flags)


# ---- through the trainer --------------------------------------------------------------------------------------------------------
W, H = 400, 240


def _cams():
    dev = torch.device(DEV)
    return [c._replace(viewmatrix=c.viewmatrix.to(dev), projmatrix=c.projmatrix.to(dev), campos=c.campos.to(dev))
            for c in syn.orbit_cameras(W, H)]


def _gts(n=8):
    return [torch.rand(3, H, W, generator=torch.Generator().manual_seed(i)).to(DEV) for i in range(n)]


def _close(a, b, start):
    """the bar of tests/test_gpu_native_trainer.py"""
    upd = float((b - start).abs().max())
    assert upd > 1e-4
    assert float(((a - b).abs() > 1e-2 * upd).float().mean()) < 1e-4
    assert float((a - b).norm() / (b - start).norm()) < 1e-3


def _table(nt):
    """the trainer's reach flags, a view into its geometry scratch"""
    off = int(nt._lib.sgr_geom_reach_offset_bytes(nt.params.P))
    return nt._geom[off: off + nt.params.P]


@pytest.fixture
def overlap():
    lib = _lib()
    before = lib.sgr_get_adam_overlap()
    yield lib.sgr_set_adam_overlap
    lib.sgr_set_adam_overlap(before)


def test_the_flag_is_a_superset_of_every_touched_row(overlap):
    """Mode 2: the forward flags, the dense kernel runs and nothing consumes the table.  Every Gaussian with a non-zero row in the flat
    gradient buffer or in the masked colours has its flag set -- for each of the 8 orbit cameras, and again on their second visit,
    which runs with the walk hint."""
    from sugar_amd.train_step import GaussianParams, NativeTrainer
    overlap(2)
    dev = torch.device(DEV)
    scene = syn.make_scene(30000, 5, 0.01, 0.06)
    cams, gts = _cams(), _gts()
    p = GaussianParams(scene, dev)
    nt = NativeTrainer(p, torch.zeros(3), W, H)
    assert not _table(nt).any()            # a new trainer starts from a clear table
    shares = []
    for i in range(16):
        _table(nt).zero_()
        nt.step(cams[i % 8], gts[i % 8], cam_key=i % 8)
        nt.synchronize()
        assert nt.redone == 0
        if i >= 8:
            assert nt._last_hinted
        flag = _table(nt) != 0
        touched = nt._send[:p.P].ne(0).any(dim=1)
        for k, g in p.split_flat(p.flat_grad).items():
            if k != "features":
                touched |= g.reshape(p.P, -1).ne(0).any(dim=1)
        assert int(touched.sum()) > 100
        assert not bool((touched & ~flag).any()), (i, int((touched & ~flag).sum()))
        shares.append((float(flag.float().mean()), float(touched.float().mean())))
    print("flagged / touched share per step:", shares)
    assert max(s[0] for s in shares) < 0.9   # the flag says something on this scene


def test_the_ride_along_equals_the_stand_alone_launch_and_touches_no_other_row(overlap):
    from sugar_amd.train_step import GaussianParams, NativeTrainer
    dev = torch.device(DEV)
    scene = syn.make_scene(30000, 5, 0.01, 0.06)
    cams, gts = _cams(), _gts(4)
    p = GaussianParams(scene, dev)
    start = p.flat.clone()
    overlap(1)
    nt = NativeTrainer(p, torch.zeros(3), W, H)
    for i in range(3):
        nt.step(cams[i], gts[i], cam_key=i)
    nt.synchronize()
    assert not _table(nt).any()            # the masked kernel put every flag back
    snap = (p.flat.clone(), nt.exp_avg.clone(), nt.exp_avg_sq.clone(), nt.t)

    def one_step(mode):
        overlap(mode)
        with torch.no_grad():
            p.flat.copy_(snap[0]); nt.exp_avg.copy_(snap[1]); nt.exp_avg_sq.copy_(snap[2])
        nt.t = snap[3]
        _table(nt).zero_()
        nt.step(cams[3], gts[3], cam_key=3)
        nt.synchronize()
        assert nt.redone == 0
        return p.flat.clone(), nt.exp_avg.clone(), nt.exp_avg_sq.clone(), _table(nt).clone()

    one_step(0)                            # (leaves camera 3 its walk hint: the three runs below are all hinted)
    off = one_step(0)
    assert not off[3].any()                # switch off: the forward does not flag
    flagged = one_step(2)[3] != 0          # which rows this step's forward flags
    on = one_step(1)
    assert not on[3].any()
    rows = ~flagged
    assert 0.05 < float(rows.float().mean()) < 0.95
    sh = lambda t: p.split_flat(t)["features"].reshape(p.P, 48)
    for a, b in zip(on[:3], off[:3]):      # unflagged rows: parameters and both moments of the SH block, bit for bit
        assert torch.equal(sh(a)[rows].view(torch.int32), sh(b)[rows].view(torch.int32))
    # ... and bit-equal to the stand-alone zero-gradient launch on a copy of the saved state
    cp = [sh(t).clone().contiguous() for t in snap[:3]]
    fl = flagged.to(torch.uint8).contiguous()
    rc = _lib().sgr_sh_adam_zero_grad(p.P, 16, cp[0].data_ptr(), cp[1].data_ptr(), cp[2].data_ptr(), fl.data_ptr(), p.LRS["features"], p.REST_LR,
                                      B1, B2, EPS, snap[3] + 1, 1.0, None, 0, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    for a, b, s0 in zip(on[:3], cp, snap[:3]):
        assert torch.equal(sh(a)[rows].view(torch.int32), b[rows].view(torch.int32))
        assert torch.equal(b[flagged].view(torch.int32), sh(s0)[flagged].view(torch.int32))   # the zero half leaves flagged rows alone
    assert not torch.equal(sh(on[0])[rows], sh(snap[0])[rows])
    _close(on[0], off[0], start)


def test_skipped_and_repaired_steps_update_once(overlap):
    """(a) twelve steps over the 8 cameras from a list capacity of 1000: the first forward overflows, the device skips that step --
    ride-along included -- and the host repeats it; (b) walk hints cut to one entry at step 10: the tiles are repaired in place (the
    repair kernel flags too).  Switch on against off."""
    from sugar_amd.train_step import GaussianParams, NativeTrainer
    dev = torch.device(DEV)
    scene = syn.make_scene(30000, 5, 0.01, 0.06)
    cams, gts = _cams(), _gts()
    out = {}
    for mode in (1, 0):
        overlap(mode)
        p = GaussianParams(scene, dev)
        start = p.flat.clone()
        nt = NativeTrainer(p, torch.zeros(3), W, H, capacity=1000)
        losses = []
        for i in range(12):
            loss = nt.step(cams[i % 8], gts[i % 8], cam_key=i % 8)
            nt.synchronize()
            losses.append(float(loss))
        assert nt.redone >= 1 and nt.capacity > 1000
        q = GaussianParams(scene, dev)
        nh = NativeTrainer(q, torch.zeros(3), W, H)
        hint_losses = []
        for i in range(16):
            if i == 10:
                nh.synchronize()
                for ent in nh._hints.values():
                    ent[0].fill_(1)
            # (no host wait between the steps, as the test this follows has none: the copy is enqueued behind the step, and no step of
            # this run is repeated -- redone == 0 below --, so every one of these losses belongs to a valid forward)
            hint_losses.append(nh.step(cams[i % 8], gts[i % 8], cam_key=i % 8).clone())
        nh.synchronize()
        assert nh.redone == 0 and nh.repaired_tiles > 100
        if mode == 1:
            assert not _table(nt).any() and not _table(nh).any()
        out[mode] = (losses, p.flat.clone(), q.flat.clone(), [float(x) for x in hint_losses])
    assert np.allclose(out[1][0], out[0][0], rtol=2e-4), (out[1][0], out[0][0])
    assert np.allclose(out[1][3], out[0][3], rtol=2e-4), (out[1][3], out[0][3])
    _close(out[1][1], out[0][1], start)
    _close(out[1][2], out[0][2], start)


def test_where_the_path_is_off_the_table_stays_untouched(overlap, monkeypatch):
    """an M != 16 trainer, a step with SGR_BWD_DENSE, a step called phase by phase, and a view that asks for the eight-wave blend
    kernel (which does not flag) run the dense kernel: a sentinel written to the table before the step is still there after it"""
    from sugar_amd import _lib as L
    from sugar_amd.train_step import GaussianParams, NativeTrainer
    overlap(1)
    dev = torch.device(DEV)
    scene = syn.make_scene(30000, 5, 0.01, 0.06)
    cams, gts = _cams(), _gts(2)

    def sentinel(nt):
        _table(nt).fill_(0x5A)

    def untouched(nt):
        torch.cuda.synchronize()
        return bool((_table(nt) == 0x5A).all())

    # M = 9
    p9 = GaussianParams(scene._replace(shs=scene.shs[:, :9].contiguous()), dev)
    nt = NativeTrainer(p9, torch.zeros(3), W, H, sh_degree=2)
    before = p9.flat.clone()
    sentinel(nt)
    nt.step(cams[0], gts[0], cam_key=0)
    nt.synchronize()
    assert untouched(nt) and not torch.equal(p9.split_flat(p9.flat)["features"], p9.split_flat(before)["features"])
    # SGR_BWD_DENSE
    p = GaussianParams(scene, dev)
    nt = NativeTrainer(p, torch.zeros(3), W, H)
    before = p.flat.clone()
    monkeypatch.setenv("SGR_BWD_DENSE", "1")
    sentinel(nt)
    nt.step(cams[0], gts[0], cam_key=0)
    nt.synchronize()
    monkeypatch.delenv("SGR_BWD_DENSE")
    assert untouched(nt) and not torch.equal(p.split_flat(p.flat)["features"], p.split_flat(before)["features"])
    # phase by phase
    before = p.flat.clone()
    sentinel(nt)
    nt.t += 1
    ex = L.TrainExchange(1, None, 0, None, 1.0, nt.t)
    for ph in (1, 2, 4, 8):
        nt._call(cams[1], gts[1], 1, ph, ex if ph >= 4 else None)
    ok, _, _ = nt._valid()
    assert ok
    assert untouched(nt) and not torch.equal(p.split_flat(p.flat)["features"], p.split_flat(before)["features"])
    # a view with deep lists: the camera's second visit, once its hint has a tile above the threshold
    lib = L.load()
    deep_before = lib.sgr_get_deep_min()
    lib.sgr_set_deep_min(1)
    try:
        pd = GaussianParams(scene, dev)
        nd = NativeTrainer(pd, torch.zeros(3), W, H)
        nd.step(cams[0], gts[0], cam_key=0)
        nd.synchronize()
        assert not _table(nd).any()        # first visit, no hint yet: the split ran and cleared its flags
        before = pd.flat.clone()
        sentinel(nd)
        nd.step(cams[0], gts[0], cam_key=0)
        nd.synchronize()
        assert nd._last_hinted and nd._hints[0][5] > 1
        assert untouched(nd) and not torch.equal(pd.split_flat(pd.flat)["features"], pd.split_flat(before)["features"])
    finally:
        lib.sgr_set_deep_min(deep_before)
