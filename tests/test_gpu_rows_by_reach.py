"""GPU tests of the backward preprocess by reach flag (SGR_BWD_ROWS_BY_REACH / SGR_BWD_ROWS_UNKNOWN, sgr_set_rows_by_reach).

A. The kernel alone, bit for bit: the harness of tests/test_gpu_preprocess_bwd_rows.py (its scene, sums written into the accumulator
   table, phase 0 over a zero image gradient so that dL_dcolor is written too).  Every case runs once WITHOUT the bit into buffers
   full of a NaN-payload sentinel: that is the kernel's behaviour before the mode existed, and the reference of every comparison.
   With the bit the call runs k_preprocess_bwd_packed: one workgroup per 256 Gaussians, which lists its flagged rows -- or, from 192
   flagged rows on, takes them in order (both sides of that switch are patterns of their own).
B. Through the trainer (the recipe of tests/test_gpu_adam_overlap.py): rows left non-zero by another camera's step, changes of path
   inside one trainer, skipped and repaired steps, and the densification statistics."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from sugar_amd import synthetic as syn
from tests import bwd_rows_utils as br
from tests import parity_utils as pu
from tests.test_gpu_adam_overlap import _cams, _close, _gts, _table, H, W
from tests.test_gpu_preprocess_bwd_rows import _Case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0x7FC0BEEF  # a quiet NaN with a payload no arithmetic produces
OUTPUTS = dict(opacity=1, color=3, mean3D=3, mean2D=3, conic=4, scale=3, rot=4)  # floats per row of every output of the call
STATS = ("max_radii", "accum", "denom")
PATTERNS = ("none", "all", "alternating", "one-per-wave", "last", "dense-wave", "listed-191", "in-order-192")
DIRTY = ("zeros", "ones", "random")


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _case(P, raw):
    return _Case(raw=raw, P=P)


def _flags(P, pattern):
    i = np.arange(P)
    if pattern == "none":
        f = np.zeros(P, bool)
    elif pattern == "all":
        f = np.ones(P, bool)
    elif pattern == "alternating":
        f = i % 2 == 1
    elif pattern == "one-per-wave":
        f = i % 64 == min(7, P - 1)
    elif pattern == "last":
        f = i == P - 1
    elif pattern in ("listed-191", "in-order-192"):  # of every workgroup's 256 rows: the last count that is listed, the first that is not
        f = i % 256 < int(pattern[-3:])
    else:  # wave 0 entirely flagged (32 or more of its records dirty, below), wave 1 not at all, a random half of the others
        f = np.random.default_rng(31).random(P) < 0.5
        f[:64] = True
        f[64:128] = False
    # (any non-zero byte is a set flag)
    return np.where(f, np.where(i % 3 == 0, 0x5A, 1), 0).astype(np.uint8)


def _sums(case, flags, pattern):
    """non-zero in flagged rows only -- the superset invariant --, and +0 elsewhere (the table is clean between backwards)"""
    sums = case.sums.copy()
    if pattern == "dense-wave":
        n = min(case.P, 40)
        sums[:n] = np.random.default_rng(32).standard_normal((n, 9)).astype(np.float32)
    sums[flags == 0] = 0.0
    sums[sums == 0] = 0.0  # (-0 -> +0: "all zero" below is a statement about bits)
    return sums


def _dirty(P, kind):
    if kind == "zeros":
        return np.zeros(P, np.uint8)
    if kind == "ones":
        return np.ones(P, np.uint8)
    return (np.random.default_rng(33).random(P) < 0.5).astype(np.uint8)


class _Harness:
    """one case of the scene: the byte tables inside its geometry scratch, and sgr_backward_ex into buffers the test prepared"""

    def __init__(self, case):
        self.case, self.run = case, case.run
        run, P = case.run, case.P
        lib, geom = run.lib, run.scratch["geom"]
        o_r, o_d = int(lib.sgr_geom_reach_offset_bytes(P)), int(lib.sgr_geom_rowdirty_offset_bytes(P))
        assert o_r + P <= o_d and o_d + P <= geom.numel() and o_d % 256 == 0
        self.reach, self.rowdirty = geom[o_r:o_r + P], geom[o_d:o_d + P]
        o_h = int(lib.sgr_img_header_offset(run.W, run.H))
        self.header = run.scratch["img"][o_h:o_h + 32].view(torch.int32)
        self.dpix = torch.zeros(3, run.H, run.W, device=DEV)

    def buffers(self, zero_rows=None):
        """every output full of the sentinel, rows `zero_rows` (bool [P]) as +0"""
        P = self.case.P
        out = {k: torch.full((P, n), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32) for k, n in OUTPUTS.items()}
        if zero_rows is not None:
            z = torch.as_tensor(zero_rows).to(DEV)
            for t in out.values():
                t[z] = 0.0
        return out

    def call(self, out, sums, flags, reach, rowdirty, stats=True):
        """phase 0 over a zero image gradient (the blend backward adds zeros to the injected sums), SGR_BWD_ACC_CLEAN.
        -> the three statistics (or None)"""
        case, run, L = self.case, self.run, self.run.L
        case.inject(sums)
        self.reach.copy_(torch.as_tensor(reach).to(DEV))
        self.rowdirty.copy_(torch.as_tensor(rowdirty).to(DEV))
        dens = [torch.as_tensor(t).to(DEV).float().clone() for t in case.dens0] if stats else None
        bo = L.BackwardOpts(*([t.data_ptr() for t in dens] if stats else [None] * 3), None, int(flags) | L.SGR_BWD_ACC_CLEAN)
        p = pu.Run.ptr
        g, b, i = (run.scratch[k] for k in ("geom", "binning", "img"))
        rc = run.lib.sgr_backward_ex((pu.MODE_RAW if run.raw else 0), run.P, run.D, run.M, run.R, p(run.bg), run.W, run.H, p(run.means),
                                     p(run.shs), None, p(run.scales), run.mod, p(run.rots), None, p(run.vm), p(run.pm), p(run.cp),
                                     run.tx, run.ty, p(run.radii), p(g), p(b), p(i), p(self.dpix), p(out["mean2D"]), p(out["conic"]),
                                     p(out["opacity"]), p(out["color"]), p(out["mean3D"]), None, None, p(out["scale"]), p(out["rot"]),
                                     0, run.stream, C.byref(bo))
        assert rc >= 0, L.last_error()
        torch.cuda.synchronize()
        return dict(zip(STATS, dens)) if stats else None


def _assert_equal(got, ref, label, rows=None):
    for k in ref:
        a, b = _bits(got[k]), _bits(ref[k])
        if rows is not None:
            a, b = a[rows], b[rows]
        assert torch.equal(a, b), (label, k, int((a != b).reshape(len(a), -1).any(1).sum()))


def _one_pattern(hs, pattern, dirty_kinds, *, stats=True, invalid=False):
    case, run, L = hs.case, hs.run, hs.run.L
    P = case.P
    flags = _flags(P, pattern)
    flagged = flags != 0
    sums = _sums(case, flags, pattern)
    full = flagged & (case.rec["radii"] > 0) & br.touched(sums) & (not invalid)  # the rows that take the full backward
    if pattern == "dense-wave" and P >= 64:
        assert int((flagged & br.touched(sums))[:64].sum()) >= 32 and (P < 128 or not flagged[64:128].any())
    if pattern == "all" and P >= 63:
        assert int((~br.touched(sums)).sum()) > 0  # some flagged rows have zero sums
    # the reference: the call without the bit, every buffer full of the sentinel
    ref = hs.buffers()
    ref_stats = hs.call(ref, sums, 0, flags, _dirty(P, "random"), stats)
    for k, t in ref.items():
        assert not bool((_bits(t) == SENTINEL).any()), (pattern, k)  # every row written
        # the precondition: no unflagged row holds a non-zero (bit) in the reference
        assert not bool(_bits(t)[torch.as_tensor(~flagged).to(DEV)].any()), (pattern, k)
        if invalid:
            assert not bool(_bits(t).any()), (pattern, k)
    if invalid and stats:
        for k, t0 in zip(STATS, case.dens0):
            assert torch.equal(ref_stats[k].cpu(), torch.as_tensor(t0).float()), (pattern, k)
    full_t = torch.as_tensor(full.astype(np.uint8)).to(DEV)
    flags_t = torch.as_tensor(flags).to(DEV)
    for kind in dirty_kinds:
        dirty = _dirty(P, kind)
        quiet = ~flagged & (dirty == 0)  # the rows the mode neither loads nor stores
        label = f"{pattern}/{kind}/P{P}"
        print(f"{label}: flagged {int(flagged.sum())} full {int(full.sum())} dirty {int(dirty.sum())} quiet {int(quiet.sum())}")
        # (1) quiet rows hold +0 on entry: every buffer comes out as the reference
        out = hs.buffers(quiet)
        st = hs.call(out, sums, L.SGR_BWD_ROWS_BY_REACH, flags, dirty, stats)
        _assert_equal(out, ref, label)
        if stats:
            _assert_equal(st, ref_stats, label + " statistics")
        assert not bool(_bits(run.acc()[:, :9]).any()), label
        assert torch.equal(hs.reach, flags_t), label
        assert torch.equal(hs.rowdirty, full_t), (label, "rowdirty is 1 exactly on the rows that took the full backward")
        # (2) the sentinel in the quiet rows survives: they are not stored to; every other row as the reference
        out = hs.buffers()
        st = hs.call(out, sums, L.SGR_BWD_ROWS_BY_REACH, flags, dirty, stats)
        q = torch.as_tensor(quiet).to(DEV)
        _assert_equal(out, ref, label + " loud rows", rows=~q)
        for k, t in out.items():
            assert bool((_bits(t)[q] == SENTINEL).all()), (label, k, "a quiet row was stored to")
        if stats:
            _assert_equal(st, ref_stats, label + " statistics")
        assert torch.equal(hs.rowdirty, full_t) and torch.equal(hs.reach, flags_t), label
        # (3) SGR_BWD_ROWS_UNKNOWN: every row counts as dirty, whatever the table says
        out = hs.buffers()
        st = hs.call(out, sums, L.SGR_BWD_ROWS_BY_REACH | L.SGR_BWD_ROWS_UNKNOWN, flags, dirty, stats)
        _assert_equal(out, ref, label + " unknown")
        if stats:
            _assert_equal(st, ref_stats, label + " unknown statistics")
        assert torch.equal(hs.rowdirty, full_t) and torch.equal(hs.reach, flags_t), label
        assert not bool(_bits(run.acc()[:, :9]).any()), label


@pytest.mark.parametrize("P", (1, 63, 64, 65, 257, 1010))
def test_the_kernel_alone_equals_the_call_without_the_bit(P):
    """raw-compact, the trainer's mode: six flag patterns x three row-dirty tables x {+0 in the quiet rows, the sentinel in them,
    SGR_BWD_ROWS_UNKNOWN}, with the densification statistics and without"""
    hs = _Harness(_case(P, True))
    for pattern in PATTERNS:
        _one_pattern(hs, pattern, DIRTY)
        _one_pattern(hs, pattern, DIRTY, stats=False)  # (only without statistics does a workgroup list its flagged rows)


def test_the_kernel_alone_without_statistics_and_with_activated_parameters():
    """the headline step asks for no statistics (no word of an unflagged row's record is read); and one non-raw case"""
    hs = _Harness(_case(1010, True))
    for pattern in PATTERNS:
        _one_pattern(hs, pattern, ("random",), stats=False)
    hs = _Harness(_case(1010, False))
    for pattern in PATTERNS:
        _one_pattern(hs, pattern, ("random",))


@pytest.mark.parametrize("P", (65, 1010))
def test_an_invalid_forward_leaves_zeros_and_the_statistics_alone(P):
    """the header says that the forward did not happen (walk hint missed): all outputs zero, statistics untouched, no row dirty"""
    hs = _Harness(_case(P, True))
    word = hs.header[hs.run.L.HDR_HINT_MISS:hs.run.L.HDR_HINT_MISS + 1]
    saved = word.clone()
    word.fill_(1)
    try:
        for pattern in ("none", "alternating", "dense-wave"):
            _one_pattern(hs, pattern, DIRTY, invalid=True)
    finally:
        word.copy_(saved)
        torch.cuda.synchronize()


def test_the_mode_refuses_what_it_cannot_serve():
    """with dL_dsh the whole wave's rows leave through one staged stream, and SGR_BWD_DENSE sends unreached rows through the arithmetic"""
    case = _case(65, True)
    L = case.run.L
    for kw in (dict(store_sh=True, flags=L.SGR_BWD_ROWS_BY_REACH), dict(store_sh=False, flags=L.SGR_BWD_ROWS_BY_REACH | L.SGR_BWD_DENSE)):
        with pytest.raises(AssertionError, match="SGR_BWD_ROWS_BY_REACH"):
            case.run.backward(2, kw["store_sh"], flags=kw["flags"])


# ---- through the trainer --------------------------------------------------------------------------------------------------------
@pytest.fixture
def switches():
    """(set_adam_overlap, set_rows_by_reach), both put back afterwards"""
    from sugar_amd import _lib
    lib = _lib.load()
    before = lib.sgr_get_adam_overlap(), lib.sgr_get_rows_by_reach()
    yield lib.sgr_set_adam_overlap, lib.sgr_set_rows_by_reach
    lib.sgr_set_adam_overlap(before[0])
    lib.sgr_set_rows_by_reach(before[1])


def _rows(nt):
    """[P, 14] bits: the 11 gradient floats of every Gaussian in the flat gradient buffer and its masked colours"""
    p = nt.params
    parts = [g.reshape(p.P, -1) for k, g in p.split_flat(p.flat_grad).items() if k != "features"]
    t = torch.cat(parts + [nt._send[:p.P]], dim=1)
    assert t.shape == (p.P, 14)
    return _bits(t)


def test_the_switch_defaults_to_on_and_reads_back(switches):
    from sugar_amd import _lib
    lib = _lib.load()
    assert lib.sgr_get_rows_by_reach() == 1
    switches[1](0)
    assert lib.sgr_get_rows_by_reach() == 0
    switches[1](5)
    assert lib.sgr_get_rows_by_reach() == 1


def test_rows_left_by_another_camera_are_zero_after_the_step(switches):
    """camera k + 4's step leaves non-zero rows that camera k's forward does not flag: the step on camera k owes them zeros"""
    from sugar_amd.train_step import GaussianParams, NativeTrainer
    overlap, by_reach = switches
    dev = torch.device(DEV)
    scene = syn.make_scene(30000, 5, 0.01, 0.06)
    cams, gts = _cams(), _gts()
    p = GaussianParams(scene, dev)
    start = p.flat.clone()
    overlap(1); by_reach(1)
    nt = NativeTrainer(p, torch.zeros(3), W, H)
    for i in range(8):  # (every camera gets its walk hint: all runs below are hinted)
        nt.step(cams[i], gts[i], cam_key=i)
    nt.synchronize()
    assert not _table(nt).any()
    snap = (p.flat.clone(), nt.exp_avg.clone(), nt.exp_avg_sq.clone(), nt.t)

    def one_step(mode, on, cam):
        overlap(mode); by_reach(on)
        with torch.no_grad():
            p.flat.copy_(snap[0]); nt.exp_avg.copy_(snap[1]); nt.exp_avg_sq.copy_(snap[2])
        nt.t = snap[3]
        _table(nt).zero_()
        nt.step(cams[cam], gts[cam], cam_key=cam)
        nt.synchronize()
        assert nt.redone == 0
        return p.flat.clone(), _rows(nt).clone(), _table(nt).clone()

    for k in (0, 2):
        flagged = one_step(2, 1, k)[2] != 0      # which rows camera k's forward flags
        off = one_step(1, 0, k)
        assert not off[2].any()
        prev = one_step(1, 1, k + 4)             # (the first step by reach flag after a dense one: every row counts as dirty)
        on = one_step(1, 1, k)                   # ... and this one goes by the table
        assert not on[2].any()
        stale = prev[1].ne(0).any(dim=1) & ~flagged
        print(f"camera {k}: flagged {int(flagged.sum())}, non-zero after camera {k + 4} and unflagged now {int(stale.sum())}")
        assert int(stale.sum()) > 100
        assert not bool(on[1][~flagged].any())   # +0, bit for bit
        assert torch.equal(on[1][flagged].ne(0).any(dim=1), off[1][flagged].ne(0).any(dim=1))
        assert not bool(off[1][~flagged].any())
        _close(on[0], off[0], start)


def test_changes_of_path_inside_one_trainer(switches, monkeypatch):
    """on / on / SGR_BWD_DENSE / on / phase by phase / on / overlap off / on / another trainer / on / a torch write / on / on: after every
    step by reach flag the rows its forward did
    not flag hold +0.  The flags of a step come from a second trainer that runs the same forward (same parameters, no walk hint on
    either side) in the verification mode, which leaves them in the table."""
    from sugar_amd import _lib as L
    from sugar_amd.train_step import GaussianParams, NativeTrainer
    overlap, by_reach = switches
    dev = torch.device(DEV)
    scene = syn.make_scene(30000, 5, 0.01, 0.06)
    cams, gts = _cams(), _gts()
    p, q = GaussianParams(scene, dev), GaussianParams(scene, dev)
    overlap(1); by_reach(1)
    nt = NativeTrainer(p, torch.zeros(3), W, H, walk_hint=False)
    probe = NativeTrainer(q, torch.zeros(3), W, H, walk_hint=False)

    def flags_of(cam):
        overlap(2)
        with torch.no_grad():
            q.flat.copy_(p.flat)
        _table(probe).zero_()
        probe.step(cams[cam], gts[cam], cam_key=cam)
        probe.synchronize()
        overlap(1)
        assert probe.redone == 0
        return _table(probe) != 0

    def on(cam):
        flagged = flags_of(cam)
        before = _rows(nt).clone()
        nt.step(cams[cam], gts[cam], cam_key=cam)
        nt.synchronize()
        assert nt.redone == 0 and not _table(nt).any()
        rows = _rows(nt)
        stale = before.ne(0).any(dim=1) & ~flagged
        print(f"camera {cam}: flagged {int(flagged.sum())} stale {int(stale.sum())} non-zero rows {int(rows.ne(0).any(dim=1).sum())}")
        assert not bool(rows[~flagged].any())
        assert int(rows.ne(0).any(dim=1).sum()) > 100
        return int(stale.sum())

    on(0)
    assert on(4) > 100
    monkeypatch.setenv("SGR_BWD_DENSE", "1")
    nt.step(cams[1], gts[1], cam_key=1)
    nt.synchronize()
    monkeypatch.delenv("SGR_BWD_DENSE")
    assert on(5) > 100
    nt.t += 1
    ex = L.TrainExchange(1, None, 0, None, 1.0, nt.t)
    for ph in (1, 2, 4, 8):
        nt._call(cams[2], gts[2], 2, ph, ex if ph >= 4 else None)
    assert nt._valid()[0]
    torch.cuda.synchronize()
    assert on(6) > 100
    overlap(0)
    nt.step(cams[3], gts[3], cam_key=3)
    nt.synchronize()
    overlap(1)
    assert on(7) > 100
    # another trainer over the same parameters writes the same flat gradient buffer (bench.py --full builds one for its
    # densification leg), and torch writes it behind the library's back: NativeTrainer tells the library (sgr_trainer_invalidate_rows)
    other = NativeTrainer(p, torch.zeros(3), W, H, densify_stats=True, walk_hint=False)
    other.step(cams[0], gts[0], cam_key=0)
    other.synchronize()
    assert on(2) > 100
    with torch.no_grad():
        p.flat_grad.fill_(7.0)
        nt._send.fill_(7.0)
    assert on(3) > 100
    assert on(1) > 100


def test_skipped_and_repaired_steps_update_once(switches):
    """the recipe of tests/test_gpu_adam_overlap.py with the SH-Adam split on in both runs: by reach flag against every row"""
    from sugar_amd.train_step import GaussianParams, NativeTrainer
    overlap, by_reach = switches
    dev = torch.device(DEV)
    scene = syn.make_scene(30000, 5, 0.01, 0.06)
    cams, gts = _cams(), _gts()
    overlap(1)
    out = {}
    for mode in (1, 0):
        by_reach(mode)
        p = GaussianParams(scene, dev)
        start = p.flat.clone()
        nt = NativeTrainer(p, torch.zeros(3), W, H, capacity=1000)
        losses = []
        for i in range(12):
            loss = nt.step(cams[i % 8], gts[i % 8], cam_key=i % 8)
            nt.synchronize()
            losses.append(float(loss))
        assert nt.redone >= 1 and nt.capacity > 1000 and nt.t == 12
        q = GaussianParams(scene, dev)
        nh = NativeTrainer(q, torch.zeros(3), W, H)
        hint_losses = []
        for i in range(16):
            if i == 10:
                nh.synchronize()
                for ent in nh._hints.values():
                    ent[0].fill_(1)
            hint_losses.append(nh.step(cams[i % 8], gts[i % 8], cam_key=i % 8).clone())
        nh.synchronize()
        assert nh.redone == 0 and nh.repaired_tiles > 100 and nh.t == 16
        assert not _table(nt).any() and not _table(nh).any()
        out[mode] = (losses, p.flat.clone(), q.flat.clone(), [float(x) for x in hint_losses])
    assert np.allclose(out[1][0], out[0][0], rtol=2e-4), (out[1][0], out[0][0])
    assert np.allclose(out[1][3], out[0][3], rtol=2e-4), (out[1][3], out[0][3])
    _close(out[1][1], out[0][1], start)
    _close(out[1][2], out[0][2], start)


def test_the_densification_statistics_are_bit_equal(switches):
    """eight steps, each from the same parameters (so that both trainers run the same forwards): denom and max_radii2D count an
    unflagged, rendered Gaussian exactly as the dense rows do"""
    from sugar_amd.train_step import GaussianParams, NativeTrainer
    overlap, by_reach = switches
    dev = torch.device(DEV)
    scene = syn.make_scene(30000, 5, 0.01, 0.06)
    cams, gts = _cams(), _gts()
    overlap(1)
    got = {}
    for mode in (1, 0):
        by_reach(mode)
        p = GaussianParams(scene, dev)
        nt = NativeTrainer(p, torch.zeros(3), W, H, densify_stats=True, walk_hint=False)
        snap = (p.flat.clone(), nt.exp_avg.clone(), nt.exp_avg_sq.clone())
        for i in range(8):
            with torch.no_grad():
                p.flat.copy_(snap[0]); nt.exp_avg.copy_(snap[1]); nt.exp_avg_sq.copy_(snap[2])
            nt.step(cams[i], gts[i], cam_key=i)
            nt.synchronize()
            assert nt.redone == 0
        got[mode] = (nt.denom.clone(), nt.max_radii2D.clone(), nt.xyz_gradient_accum.clone(), nt.viewspace_grad.clone())
    assert float(got[0][0].max()) >= 2 and float(got[0][1].max()) > 1   # (rendered in several views)
    assert torch.equal(_bits(got[1][0]), _bits(got[0][0]))
    assert torch.equal(_bits(got[1][1]), _bits(got[0][1]))
    # the last step's screen-space gradient: the same rows are zero, and zero means +0 where the row was not flagged
    assert torch.equal(got[1][3].ne(0).any(dim=1), got[0][3].ne(0).any(dim=1))
    assert torch.allclose(got[1][2], got[0][2], rtol=1e-3, atol=1e-7)
