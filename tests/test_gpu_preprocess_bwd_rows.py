"""GPU tests of k_preprocess_bwd row by row against a float64 reference (oracle/torch_cpu_rasterizer.py::preprocess_backward_ref).

The technique: one forward through sgr_forward_ex, then the nine sums of every Gaussian are WRITTEN into the accumulator table
(sgr_geom_acc_offset_bytes) and the preprocess half runs alone (phase 2) -- no blend backward, no float atomics, so every output
row is compared on its own.  The scene (tests/bwd_rows_utils.py, 1010 Gaussians at 128 x 96) reaches every branch of the kernel; the
CPU test tests/test_preprocess_bwd_reference.py asserts that it does.

Tolerances are measured, not chosen: err(row) = max|got - ref64| / max|ref64 row| over the rendered, touched rows; the float32 C
oracle (orc_preprocess_backward, fed the same record and sums) gives the yardstick; the kernel's worst row must lie within 4 x the
oracle's worst row and its median within 2 x the oracle's median (FMA contraction, another order of the sums, device expf / sqrtf:
two bits).  Both distributions are printed (profiles/preprocess_bwd_rows.txt holds a recorded run)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import torch_cpu_rasterizer as tcr
from sugar_amd import synthetic as syn
from tests import bwd_rows_utils as br
from tests import parity_utils as pu

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ULP = 2.0 ** -24
PAD = float("nan")  # slots 9..15 of a record are padding: no output may depend on them


def _scene_for_run(sc, P, raw):
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a[:P]))
    if raw:
        return syn.Scene(t(sc.means3D), t(sc.raw_scales), t(sc.raw_rot), t(sc.raw_opac[:, None]), t(sc.shs))
    return syn.Scene(t(sc.means3D), t(sc.scales), t(sc.rot_given), t(sc.opac[:, None]), t(sc.shs))


class _Case:
    """the scene (or a prefix of it) in one mode: inputs of the reference, one forward on the GPU, its record"""

    def __init__(self, *, raw=False, P=None, cam_i=0, shuffled=True, mode="sh", D=3, M=16, cov=False, scale_modifier=1.0):
        self.sc = sc = br.scene(shuffled)
        self.raw = raw
        self.P = P = P or br.P_FULL
        cam = br.camera(cam_i)
        self.kw = kw = br.inputs(sc, cam, raw=raw, P=P, mode=mode, D=D, M=M, cov=cov, scale_modifier=scale_modifier)
        self.run = pu.Run(_scene_for_run(sc, P, raw), cam, torch.zeros(3), raw, raw_given=True, D=D, M=M,
                          colors=kw.get("colors_precomp"), cov=kw.get("cov3D_precomp"), scale_modifier=scale_modifier, device=DEV)
        r = self.run.record()
        self.rec = dict(opacity=r[:, 5].copy(), conic=r[:, [2, 3, 4]].copy(), radii=r[:, 7].copy().view(np.int32),
                        clamped=((r[:, 11].copy().view(np.uint32)[:, None] >> np.arange(3, dtype=np.uint32)) & 1).astype(bool))
        assert np.array_equal(self.rec["radii"], self.run.radii.cpu().numpy())
        self.sums = sc.sums[:P]
        rng = np.random.default_rng(24)  # the statistics start from non-trivial values (radii here go from 1 to beyond 100)
        self.dens0 = (rng.random(P).astype(np.float32) * 40, rng.random(P).astype(np.float32) * 5,
                      rng.integers(0, 10, P).astype(np.float32))

    def inject(self, sums=None):
        sums = self.sums if sums is None else sums
        table = torch.full((self.P, 16), PAD)
        table[:, :9] = torch.as_tensor(sums)
        self.run.acc().copy_(table.to(DEV))
        torch.cuda.synchronize()

    def backward(self, store_sh, sums=None, phase=2, **kw):
        """phase 2: the preprocess half over the injected table.  phase 0 (the only one that writes dL_dcolor in every mode): the
        blend backward runs too, over a zero image gradient and WITHOUT the table's reset (SGR_BWD_ACC_CLEAN) -- it adds zeros."""
        self.inject(sums)
        if phase == 0:
            kw["flags"] = kw.get("flags", 0) | self.run.L.SGR_BWD_ACC_CLEAN
            kw["dpix"] = torch.zeros(3, br.H, br.W, device=DEV)
        out = self.run.backward(phase, store_sh, dens0=self.dens0, **kw)
        return {k: v.cpu().numpy() for k, v in out.items()}

    @functools.cached_property
    def oracle_state(self):
        return br.oracle_forward(self.sc, self.kw, self.raw)[0]

    def reference(self, sums=None, **kw):
        return tcr.preprocess_backward_ref(self.rec, self.sums if sums is None else sums, raw=self.raw, **self.kw, **kw)

    def yardstick(self, sums=None):
        return br.oracle_rows(self.sc, self.kw, self.raw, self.oracle_state, self.rec, self.sums if sums is None else sums)


@functools.lru_cache(maxsize=None)
def _full(raw):
    """the full scene in SH mode with dL_dsh: its outputs (what the prefixes must reproduce), reference and yardstick"""
    case = _Case(raw=raw)
    return case, case.backward(True), case.reference(), case.yardstick()


def _bad_rows(err, rows, bound):
    o = np.argsort(err)[::-1]
    return [(int(rows[i]), float(err[i])) for i in o if err[i] > bound][:8]


def _check(case, out, *, store_sh, label, sums=None, phase=2, ref=None, yard=None, yard_err=None, statistics=True,
           masked_colour=None, medians=True):
    """everything every case must hold.  ref / yard: computed here unless given; yard_err: the oracle's row errors themselves (a
    prefix is measured with the full scene's)"""
    sums = case.sums if sums is None else sums
    P, rec, raw = case.P, case.rec, case.raw
    ref = case.reference(sums) if ref is None else ref
    yard = case.yardstick(sums) if yard is None and yard_err is None else yard
    vis = rec["radii"] > 0
    live = vis & br.touched(sums)
    rows = np.flatnonzero(live)
    print(f"{label}: P {P} rendered {int(vis.sum())} touched {len(rows)}")
    # coverage: no NaN anywhere; culled rows and zero rows are exactly zero in every output
    for k, v in out.items():
        assert not np.isnan(v).any(), (label, k)
        if k not in ("denom", "max_radii", "accum"):
            assert not v.reshape(P, -1)[~live].any(), (label, k)
    # gradients against the float64 reference, the float32 oracle as the yardstick
    names = [k for k in br.GRADS if k in ref and k in out] + (["opacity"] if raw else [])
    assert set(names) >= {"mean3D"} and (("sh" in names) == bool(store_sh))
    for k in names:
        e_orc = yard_err[k] if yard_err is not None else br.row_err(yard[k], ref[k], rows)[0]
        e_gpu, at = br.row_err(out[k], ref[k], rows)
        print("  " + br.describe(f"{label} oracle dL_d{k}", e_orc))
        print("  " + br.describe(f"{label} kernel dL_d{k}", e_gpu))
        if not len(e_gpu):
            continue
        assert e_gpu.max() <= 4 * e_orc.max(), (label, k, "rows over 4 x the oracle's worst", _bad_rows(e_gpu, at, 4 * e_orc.max()))
        if medians:
            assert np.median(e_gpu) <= 2 * np.median(e_orc), (label, k, float(np.median(e_gpu)), float(np.median(e_orc)))
    # the finishing step: four float32 roundings, doubled for contraction and order
    if "mean2D" in out:
        for got, want, mag, name in ((out["mean2D"][:, :2], ref["mean2D"], ref["mean2D_mag"], "mean2D"),
                                     (out["conic"][:, [0, 1, 3]], ref["conic"], ref["conic_mag"], "conic")):
            over = np.abs(got.astype(np.float64) - want) > 8 * ULP * mag
            assert not over.any(), (label, name, "rows", np.flatnonzero(over.any(1))[:8])
        assert not out["mean2D"][:, 2].any() and not out["conic"][:, 2].any()
    if not raw:
        assert np.array_equal(out["opacity"][rows].view(np.uint32), sums[rows, 3].view(np.uint32)), (label, "opacity")
    if phase == 0:
        want = np.where(rec["clamped"], np.float32(0), sums[:, :3]) if masked_colour else sums[:, :3]
        bad = np.flatnonzero((out["color"][rows].view(np.uint32) != np.ascontiguousarray(want[rows]).view(np.uint32)).any(1))
        assert not len(bad), (label, "color rows", rows[bad][:8])
    else:
        assert "color" not in out
    if statistics:
        r0, a0, d0 = case.dens0
        assert np.array_equal(out["denom"], d0 + vis), label
        assert np.array_equal(out["max_radii"], np.where(vis, np.maximum(r0, rec["radii"].astype(np.float32)), r0)), label
        assert np.array_equal(out["accum"][~live], a0[~live]), label
        if "mean2D" in out:
            x, y = out["mean2D"][:, 0], out["mean2D"][:, 1]
            want = a0 + np.sqrt(x * x + y * y)   # (float32 throughout)
            over = np.abs(out["accum"] - want) > 2 * np.spacing(want)
            assert not over[live].any(), (label, "accum rows", np.flatnonzero(over & live)[:8])
    return ref, yard


MODES = {
    "nonraw-sh": dict(raw=False, store_sh=True), "nonraw-compact": dict(raw=False, store_sh=False),
    "raw-sh": dict(raw=True, store_sh=True), "raw-compact": dict(raw=True, store_sh=False),
    "cov3D": dict(raw=False, store_sh=True, cov=True), "colors": dict(raw=False, store_sh=False, mode="colors"),
    "modifier-nonraw-sh": dict(raw=False, store_sh=True, scale_modifier=0.7),
    "modifier-raw-compact": dict(raw=True, store_sh=False, scale_modifier=0.7),
    "camera3-nonraw-sh": dict(raw=False, store_sh=True, cam_i=3),
    "blocks-raw-sh": dict(raw=True, store_sh=True, shuffled=False),
}


@pytest.mark.parametrize("name", list(MODES))
def test_every_row_against_the_float64_reference(name):
    opts = dict(MODES[name])
    store_sh = opts.pop("store_sh")
    case = _Case(**opts)
    _check(case, case.backward(store_sh), store_sh=store_sh, label=name)


@pytest.mark.parametrize("name", ("nonraw-sh", "raw-compact", "colors"))
def test_phase_0_writes_the_colour_gradient(name):
    """dL_dcolor: the three colour sums bit for bit -- clamp-masked in the compact mode --, and every other output as in phase 2"""
    opts = dict(MODES[name])
    store_sh = opts.pop("store_sh")
    case = _Case(**opts)
    out = case.backward(store_sh, phase=0)
    _check(case, out, store_sh=store_sh, label=name + "-phase0", phase=0, masked_colour=(name == "raw-compact"))
    two = case.backward(store_sh)
    for k in two:
        assert np.array_equal(two[k].view(np.uint32), out[k].view(np.uint32)), k


@pytest.mark.parametrize("D,M", ((0, 16), (1, 16), (2, 16), (0, 1), (1, 4), (2, 9)))
def test_sh_layouts(D, M):
    case = _Case(D=D, M=M)
    out = case.backward(True)
    ref, _ = _check(case, out, store_sh=True, label=f"D{D}-M{M}")
    assert out["sh"].shape == (case.P, M, 3) and not out["sh"][:, (D + 1) ** 2:].any()
    assert not ref["sh"][:, (D + 1) ** 2:].any() and np.abs(ref["sh"][:, (D + 1) ** 2 - 1]).max() > 0


@pytest.mark.parametrize("raw", (False, True))
def test_unaligned_dL_dsh_takes_the_scalar_stores_and_equals_the_staged_run(raw):
    case, aligned, _, _ = _full(raw)
    out = case.backward(True, sh_offset=1)
    assert case.run._sh_buf.data_ptr() % 16 == 0 and case.run._sh_buf[1:].data_ptr() % 16 == 4
    assert np.isnan(case.run._sh_buf[:1].cpu().numpy()).all()  # (the float before the first row is not written)
    for k in aligned:
        assert np.array_equal(aligned[k].view(np.uint32), out[k].view(np.uint32)), k


def test_the_full_scene_in_both_parameterisations():
    for raw in (False, True):
        case, out, ref, yard = _full(raw)
        _check(case, out, store_sh=True, label="full-raw" if raw else "full-nonraw", ref=ref, yard=yard)


@pytest.mark.parametrize("raw", (False, True))
@pytest.mark.parametrize("P", (1, 63, 64, 65, 255, 257))
def test_prefixes_of_the_scene(P, raw):
    """the last wave is partial and so is the staged epilogue; the forward is re-run.  A row does not depend on its neighbours: a
    prefix reproduces the full run's rows bit for bit; its yardstick is the full scene's (a handful of rows has no distribution)"""
    full, full_out, full_ref, full_yard = _full(raw)
    case = _Case(raw=raw, P=P)
    for k in case.rec:
        assert np.array_equal(case.rec[k], full.rec[k][:P]), k
    rows = np.flatnonzero((full.rec["radii"] > 0) & br.touched(full.sums))
    yard_err = {k: br.row_err(full_yard[k], full_ref[k], rows)[0] for k in full_yard}
    label = f"prefix-{P}-{'raw' if raw else 'nonraw'}"
    if not br.touched(case.sums).any():  # (P = 1: the scene's first row is a zero row -- so also with sums of its own)
        sums = np.random.default_rng(26).standard_normal((P, 9)).astype(np.float32)
        _check(case, case.backward(True, sums), store_sh=True, sums=sums, label=label + "-touched", yard_err=yard_err, medians=False)
    out = case.backward(True)
    _check(case, out, store_sh=True, label=label, yard_err=yard_err, medians=False)
    for k in out:
        if k not in ("denom", "max_radii", "accum"):
            assert np.array_equal(out[k].view(np.uint32), np.ascontiguousarray(full_out[k][:P]).view(np.uint32)), k


@pytest.mark.parametrize("store_sh", (False, True))
def test_without_the_intermediate_outputs_everything_else_is_bit_equal(store_sh):
    case = _full(True)[0]
    both = case.backward(store_sh)
    out = case.backward(store_sh, intermediates=False)
    assert set(both) - set(out) == {"mean2D", "conic"}
    for k in out:
        assert np.array_equal(both[k].view(np.uint32), out[k].view(np.uint32)), k
    _check(case, out, store_sh=store_sh, label=f"no-intermediates-{store_sh}")


@pytest.mark.parametrize("raw", (False, True))
@pytest.mark.parametrize("store_sh", (False, True))
def test_the_dense_switch_equals_the_default_on_every_row(store_sh, raw):
    case = _full(raw)[0]
    sparse = case.backward(store_sh)
    dense = case.backward(store_sh, flags=case.run.L.SGR_BWD_DENSE)
    for k in sparse:
        assert not np.isnan(dense[k]).any() and np.array_equal(sparse[k], dense[k]), k  # (as values: a zero may change its sign)
    live = (case.rec["radii"] > 0) & br.touched(case.sums)
    for k in sparse:
        assert np.array_equal(sparse[k][live].view(np.uint32), dense[k][live].view(np.uint32)), k


def _block_sums(P):
    """31, 32 and 33 dirty records in the first three waves (both sides of the wave-wide cleaning's >= 32 switch), a mixture in the
    others, and the last, partial wave entirely dirty (the row0 + (j >> 2) < P guard)"""
    rng = np.random.default_rng(25)
    sums = rng.standard_normal((P, 9)).astype(np.float32)
    sums[rng.random(P) < 0.5] = 0.0
    for wave, n in enumerate((31, 32, 33)):
        w = sums[64 * wave:64 * wave + 64]
        w[:] = 0.0
        at = rng.permutation(64)[:n]
        w[at] = rng.standard_normal((n, 9)).astype(np.float32)
        w[at[0]] = 0.0; w[at[0], 8] = 1.5      # (one of them dirty in its ninth float alone)
    last = (P // 64) * 64
    sums[last:] = rng.standard_normal((P - last, 9)).astype(np.float32)
    return sums


@pytest.mark.parametrize("store_sh", (False, True))
def test_the_self_cleaning_table(store_sh):
    case = _full(True)[0]
    P = case.P
    sums = _block_sums(P)
    dirty = br.touched(sums).reshape(-1)
    assert [int(dirty[64 * w:64 * w + 64].sum()) for w in range(3)] == [31, 32, 33] and P % 64 and dirty[(P // 64) * 64:].all()
    plain = case.backward(store_sh, sums)
    assert np.array_equal(case.run.acc()[:, :9].contiguous().cpu().numpy().view(np.uint32), sums.view(np.uint32))  # (read only)
    geom = case.run.scratch["geom"]
    o = case.run.lib.sgr_geom_acc_offset_bytes(P)
    assert o + P * 64 <= geom.numel()
    case.inject(sums)
    before = geom.clone()
    clean = case.run.backward(2, store_sh, flags=case.run.L.SGR_BWD_ACC_CLEAN, dens0=case.dens0)
    for k in plain:
        assert np.array_equal(plain[k].view(np.uint32), clean[k].cpu().numpy().view(np.uint32)), k
    assert not case.run.acc()[:, :9].contiguous().view(torch.int32).any()
    # nothing outside the table's P records is written: neither before it nor in the scratch behind its last record
    assert torch.equal(geom[:o], before[:o]) and torch.equal(geom[o + P * 64:], before[o + P * 64:])
    print(f"geometry scratch: {geom.numel()} bytes, table at {o} .. {o + P * 64}, {geom.numel() - o - P * 64} bytes behind it compared")
    _check(case, plain, store_sh=store_sh, sums=sums, label=f"block-sums-{store_sh}")


def test_sh_direction_elsewhere():
    """compact mode with SGR_MODE_SH_DIR_ELSEWHERE: dL_dmean3D lacks the term through the view direction, and
    sgr_sh_adam_from_views_ex forms that term from this run's dL_dcolor.  Each part is compared with its float64 counterpart, and
    their sum with the full gradient, on the scale of the full gradient's row (the two parts may cancel) within the yardstick of
    dL_dmean3D."""
    case = _full(True)[0]
    P, run = case.P, case.run
    ref, yard = case.reference(), case.yardstick()
    ref_det = dict(case.reference(detach_direction=True))
    out = case.backward(False, phase=0, mode=pu.MODE_SH_DIR_ELSEWHERE)
    checked = dict(out); checked["mean3D"] = np.zeros_like(out["mean3D"])  # (compared below)
    ref_z = dict(ref_det); ref_z["mean3D"] = np.zeros_like(ref["mean3D"])
    yard_z = dict(yard); yard_z["mean3D"] = np.zeros_like(yard["mean3D"])
    _check(case, checked, store_sh=False, label="sh-dir-elsewhere", phase=0, masked_colour=True, ref=ref_z, yard=yard_z)
    sh0 = run.shs.clone()
    m, v = torch.zeros_like(sh0), torch.zeros_like(sh0)
    extra = torch.full((P, 3), float("nan"), device=DEV)
    dcol = torch.as_tensor(out["color"]).to(DEV)
    p = pu.Run.ptr
    rc = run.lib.sgr_sh_adam_from_views_ex(P, 1, 3, 16, p(run.means), p(run.cp), p(dcol), 0, p(sh0), p(m), p(v), 0.0, 0.0, 0.9, 0.999,
                                           1e-15, 1, 1.0, p(extra), run.stream)
    assert rc >= 0, run.L.last_error()
    torch.cuda.synchronize()
    assert torch.equal(sh0.view(torch.int32), run.shs.view(torch.int32))  # both learning rates 0: the parameters come back bit-equal
    extra = extra.cpu().numpy()
    assert not np.isnan(extra).any()
    live = (case.rec["radii"] > 0) & br.touched(case.sums)
    rows = np.flatnonzero(live)
    assert not extra[~live].any()
    top = np.abs(ref["mean3D"][rows]).max(1)
    keep = top > 0
    e_orc, _ = br.row_err(yard["mean3D"], ref["mean3D"], rows)
    parts = dict(detached=(out["mean3D"], ref_det["mean3D"]), direction=(extra, ref["mean3D"] - ref_det["mean3D"]),
                 total=(out["mean3D"].astype(np.float64) + extra, ref["mean3D"]))
    assert (np.abs(parts["direction"][1][rows]).max(1) > 1e-3 * top).mean() > 0.5  # (the direction part is no rounding error)
    for name, (got, want) in parts.items():
        err = np.abs(got[rows] - want[rows]).max(1)[keep] / top[keep]
        print("  " + br.describe(f"sh-dir-elsewhere {name} (oracle full: max {e_orc.max():.3e} median {np.median(e_orc):.3e})", err))
        assert err.max() <= 4 * e_orc.max(), (name, _bad_rows(err, rows[keep], 4 * e_orc.max()))
        assert np.median(err) <= 2 * np.median(e_orc), name
        assert not np.asarray(got)[rows][~keep].any()
