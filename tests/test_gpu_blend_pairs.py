"""The blend kernels per pixel and per Gaussian against float64 (tests/blend_pairs.py; the CPU half: tests/test_blend_pairs_cpu.py).

Each case is scene x alpha mode x forward route: ONE forward through the C ABI with SGR_FLAG_REACH (tests/parity_utils.py::Run), the
records, lists and ranges read back and shown to equal the C oracle's bit for bit -- the premise: reference and yardstick are then the
ones tests/blend_pairs.py::case evaluated from exactly those inputs --, then one phase-1 backward (accumulator reset, blend backward,
masked colours) over the fragile-masked pixel gradient.  The accumulator table is the blend backward's own output.

Routes: (a) plain; (b) hinted: a first forward writes tile_need_out, the forward under test takes it as tile_need; (c) repaired:
tile_need = 1 everywhere, so k_blend_fwd_repair blends the tiles again and writes their masks and flags.  The scratch of every forward
starts as 0xFF bytes (parity_utils._PatternScratch): final_T, n_contrib, tile_maxc and the masks are what the kernels wrote.

Figures of the run that set nothing (the bars come from the float32 yardstick): profiles/blend_pairs.txt."""
import functools

import numpy as np
import pytest
import torch

import sugar_amd
from sugar_amd import _lib
from tests import blend_pairs as bp
from tests import parity_utils as pu

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROUTES = ("plain", "hinted", "repaired")
# (b) and (c) on `mixed` and `built`; (b) on `opaque` too, with the tiles' own walked counts as the hint: only there do most pixels
# stop early, so that a hint cuts lists short
CASES = [(s, "plain") for s in bp.SCENES] + [(s, r) for r in ROUTES[1:] for s in ("mixed", "built")] + [("opaque", "hinted")]


def _forward(name, route):
    scene, cam, bg = bp.scene(name), bp.camera(), bp.bg_tensor()
    T = bp.GX * bp.GY
    kw = dict(flags=_lib.SGR_FLAG_REACH, header_host=True)
    if route == "hinted":
        hint = torch.zeros(T, dtype=torch.int32, device=DEV)
        first = pu.Run(scene, cam, bg, False, tile_need_out=hint, **kw)
        torch.cuda.synchronize()
        if name == "opaque":   # the tightest hint the contract allows: what the tiles walked, without tile_need_out's margin of 25 % + 64
            hint = torch.as_tensor(np.maximum(first.tile_walked().astype(np.int32), 1)).to(DEV)
        kw["tile_need"] = hint
    elif route == "repaired":
        kw["tile_need"] = torch.ones(T, dtype=torch.int32, device=DEV)
    run = pu.Run(scene, cam, bg, False, **kw)
    torch.cuda.synchronize()
    return run


def _forward_outputs(run):
    return dict(color=run.color.cpu().numpy(), final_T=run.final_T().copy(), n_contrib=run.n_contrib().copy())


@functools.lru_cache(maxsize=None)
def _plain_outputs(name, exact):
    """route (a)'s image, final_T and n_contrib in this alpha mode (the caller has set it): what (b) and (c) must equal bit for bit"""
    return _forward_outputs(_forward(name, "plain"))


def _check(name, exact, route):
    c = bp.case(name)
    ref, inp, st = c.ref, c.inp, c.st
    P = inp.xy.shape[0]
    label = f"{name}/{'exact' if exact else 'fast'}/{route}"
    run = _forward(name, route)
    hdr = run.header.numpy().astype(np.int64)
    assert hdr[8 + _lib.HDR_HINT_MISS] == 0 and hdr[8 + _lib.HDR_R] == st["num_rendered"], hdr
    if route == "repaired":
        assert hdr[8 + _lib.HDR_REPAIR] > 0, hdr
        print(f"{label}: {hdr[8 + _lib.HDR_REPAIR]} tiles repaired")

    # 1. the premise: what the blend read is what the C oracle computed, bit for bit
    rec = run.record()
    pl, ts = run.point_list(), run.tile_start().astype(np.int64)
    assert int(ts[-1]) == st["num_rendered"] and np.array_equal(pl, st["point_list"])
    lens = st["ranges"][:, 1].astype(np.int64) - st["ranges"][:, 0]
    assert np.array_equal(ts[1:] - ts[:-1], lens)
    assert np.array_equal(ts[:-1][lens > 0], st["ranges"][:, 0][lens > 0])
    if (name, route) == ("opaque", "hinted"):
        short = int((run.tile_need.cpu().numpy().astype(np.int64) < lens).sum())
        print(f"{label}: the hint is shorter than the list in {short} of {len(lens)} tiles")
        print(f"{label}: hint {run.tile_need.cpu().numpy().tolist()}, the reference's walked {c.ref['walked'].tolist()}, repaired {hdr[8 + _lib.HDR_REPAIR]}")
        assert short >= 3
    listed = np.unique(pl)
    mine = bp.inputs_from_record(rec, pl, ts)
    for k in ("xy", "conic", "op", "rgb"):
        a, b = getattr(mine, k)[listed], getattr(inp, k)[listed]
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (label, k)
    clamp_bits = rec[:, pu.REC_CLAMPED].view(np.uint32)
    assert np.array_equal(((clamp_bits[listed, None] >> np.arange(3)) & 1).astype(bool), st["clamped"][listed].astype(bool))
    radius = rec[:, pu.REC_RADIUS].view(np.int32)
    assert np.array_equal(run.radii.cpu().numpy(), st["radii"]) and np.array_equal(radius[listed], st["radii"][listed])

    # one backward: phase 1 = accumulator reset, blend backward, masked colours
    out = run.backward(1, False, dpix=torch.as_tensor(c.dpix).to(DEV))
    acc = run.acc().cpu().numpy()
    got = dict(_forward_outputs(run), sums=acc[:, :9])

    # 2. + 3. per pixel and per Gaussian, on the condition magnitudes, within 4x / 2x the float32 yardstick
    fails, figs = bp.compare(ref, c.bar, got, label)
    for line in bp.table(label, c.bar, figs):
        print(line)
    nc = got["n_contrib"].reshape(bp.H, bp.W)
    want_maxc = [int(nc[py, px].max()) for px, py in map(bp.tile_pixels, range(bp.GX * bp.GY))]
    assert np.array_equal(run.tile_maxc().astype(np.int64), np.array(want_maxc)), (label, "tile_maxc")
    assert not fails, "\n".join(fails)
    assert not acc[:, 9:].view(np.uint32).any(), (label, "the padding of the accumulator records was written")
    dead = ~(ref["mag"] > 0).any(1)
    assert not acc[dead, :9].any(), label

    # 4. the masked colours are the first three sums, bit for bit, zero where the record says clamped (or culled)
    want = acc[:, :3].copy()
    want[((clamp_bits[:, None] >> np.arange(3)) & 1).astype(bool)] = 0.0
    want[radius <= 0] = 0.0
    assert np.array_equal(out["color"].cpu().numpy().view(np.uint32), want.view(np.uint32)), (label, "dL_dcolor")

    # 5. reach: a superset of what the backward can touch
    flagged = run.reach() != 0
    live = ~dead
    assert flagged[live].all(), (label, "unflagged Gaussians with a non-zero magnitude", np.flatnonzero(live & ~flagged)[:8])
    assert not acc[~flagged, :9].any(), label
    print(f"{label}: flagged {int(flagged.sum())} of {P}, reached {int(live.sum())}, flagged but unreached "
          f"{int((flagged & ~live).sum())} = {100.0 * (flagged & ~live).sum() / max(1, flagged.sum()):.1f} % of the flagged; "
          f"pairs {ref['pairs']}, fragile pixels left out {int(ref['fragile'].sum())}")

    # 6. the routes agree bit for bit
    if route != "plain":
        plain = _plain_outputs(name, exact)
        for k, v in plain.items():
            assert np.array_equal(v.view(np.uint32), got[k].view(np.uint32)), (label, k, "differs from the plain route")


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "fast"])
@pytest.mark.parametrize("name,route", CASES, ids=[f"{s}-{r}" for s, r in CASES])
def test_the_blend_kernels_pair_by_pair(name, route, exact):
    sugar_amd.set_exact_alpha(exact)
    try:
        _check(name, exact, route)
    finally:
        sugar_amd.set_exact_alpha(True)
