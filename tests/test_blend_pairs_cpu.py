"""CPU half of the per-pixel / per-Gaussian tests of the blend kernels (tests/blend_pairs.py; GPU half: tests/test_gpu_blend_pairs.py).

1. The float64 reference against two independent implementations: the float32 C oracle (walk and hand-derived backward) and float64
   autograd over oracle/torch_cpu_rasterizer.py::render.
2. The fragile share of every scene is at most 1 %.
3. Every case the scenes were built for is populated.
4. The comparator the GPU test calls rejects the float32 yardstick with one defect at a time, and accepts it without."""
import numpy as np
import pytest
import torch

from oracle import cpu_oracle as orc
from oracle import torch_cpu_rasterizer as tcr
from tests import blend_pairs as bp

# Reference (float64) against the C oracle (float32 terms, double sums), per pixel and per row on the condition magnitude.  The bar is
# measured, not derived: the numpy float32 walk of tests/blend_pairs.py (`own`: its own forward, its float32 pixel-order sums) is a third
# implementation of the same arithmetic, and the oracle may be off by at most ORACLE_MARGIN times that walk's worst error.  (A bound
# derived from the roundings of a 270-step chain comes to 1.2e-4, a hundred times what either shows, and would let a term pass that is
# wrong by 1e-4 of its magnitude.)
ORACLE_MARGIN = 4.0


def _rows(fin, mag, got, k):
    n = len(fin[k])
    want, m, have = fin[k].reshape(n, -1), mag[k].reshape(n, -1), np.asarray(got[k], np.float64).reshape(n, -1)
    live = m > 0
    assert not have[~live].any(), k
    return np.abs(have - want)[live] / m[live], int(live.any(1).sum())


@pytest.mark.parametrize("name", bp.SCENES)
def test_the_reference_agrees_with_the_c_oracle(name):
    c = bp.case(name)
    st, ref = c.st, c.ref
    keep = ~ref["fragile"]
    assert np.array_equal(st["n_contrib"].astype(np.int64)[keep], ref["n_contrib"][keep])
    e = bp.errors(ref, dict(color=st["color"], final_T=st["final_T"], sums=ref["sums"]))
    y = bp.errors(ref, c.own)
    for k in ("color", "final_T"):
        print(f"{name}: {k} worst {e[k].max():.3e}, the float32 walk's {y[k].max():.3e}")
        assert e[k].max() <= ORACLE_MARGIN * y[k].max(), (name, k)
    # entries walked per tile, in the tiles that hold no fragile pixel
    clear = np.array([not ref["fragile"][py * bp.W + px].any() for px, py in map(bp.tile_pixels, range(bp.GX * bp.GY))])
    assert clear.sum() >= bp.GX * bp.GY - int(ref["fragile"].sum()) and clear.sum() >= 9
    assert np.array_equal(st["walked"].astype(np.int64)[clear], ref["walked"][clear]), name
    g = orc.backward(st, c.dpix)
    fin, mag = bp.finish(c.inp, ref["sums"]), bp.finish_mag(c.inp, ref["mag"])
    got = dict(color=g["dL_dcolors"], opacity=g["dL_dopacity"].reshape(-1), mean2D=g["dL_dmeans2D"][:, :2],
               conic=g["dL_dconic"].reshape(-1, 4)[:, [0, 1, 3]])
    walk = bp.finish(c.inp, c.own["sums"])   # the float32 walk's sums through the same finishing step
    for k in fin:
        err, n = _rows(fin, mag, got, k)
        err_y, _ = _rows(fin, mag, walk, k)
        print(f"{name}: {k} rows {n} worst {err.max():.3e} median {np.median(err):.3e}, the float32 walk's worst {err_y.max():.3e}")
        assert err.max() <= ORACLE_MARGIN * err_y.max(), (name, k)


def test_the_analytic_recurrence_agrees_with_autograd():
    """`mixed`: forward_ref / backward_ref fed the float64 preprocess of oracle/torch_cpu_rasterizer.py, against its render() under
    float64 autograd -- image and opacity gradient to 1e-10"""
    c = bp.case("mixed")
    scene, cam, st = bp.scene("mixed"), bp.camera(), c.st
    d = lambda t: t.double()
    kw = dict(shs=d(scene.shs), scales=d(scene.scales), rotations=d(scene.rotations), viewmatrix=d(cam.viewmatrix), projmatrix=d(cam.projmatrix),
              campos=d(cam.campos), W=bp.W, H=bp.H, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy)
    opac = d(scene.opacities).clone().requires_grad_(True)
    means2D = torch.zeros(len(opac), 3, dtype=torch.float64)
    img, ncon = tcr.render(d(scene.means3D), means2D, opac, bg=d(bp.bg_tensor()), point_list=st["point_list"], ranges=st["ranges"],
                           radii=st["radii"], **kw)
    dpix = torch.as_tensor(c.dpix.astype(np.float64))
    (grad,) = torch.autograd.grad((img * dpix).sum(), [opac])
    pp = tcr.preprocess(d(scene.means3D), **kw)
    pix = ((pp["p_proj"][:, :2] + 1.0) * torch.tensor([bp.W, bp.H], dtype=torch.float64) - 1.0) * 0.5
    inp = c.inp._replace(xy=pix.numpy(), conic=pp["conic"].numpy(), op=opac.detach().numpy().reshape(-1), rgb=pp["color"].numpy())
    ref = bp.forward_ref(inp)
    ref.update(bp.backward_ref(inp, ref, c.dpix))
    assert np.array_equal(ncon.numpy().reshape(-1), ref["n_contrib"])
    err_img = np.abs(img.detach().numpy() - ref["color"]).max()
    err_op = (np.abs(grad.numpy().reshape(-1) - ref["sums"][:, 3]) / (1.0 + ref["mag"][:, 3])).max()
    print(f"image {err_img:.3e} opacity gradient {err_op:.3e}")
    assert err_img <= 1e-10 and err_op <= 1e-10


@pytest.mark.parametrize("name", bp.SCENES)
def test_the_fragile_share_is_at_most_one_percent(name):
    c = bp.case(name)
    share = c.ref["fragile"].mean()
    print(f"{name}: fragile pixels {int(c.ref['fragile'].sum())} of {bp.W * bp.H} = {100 * share:.3f} %")
    assert share <= 0.01
    assert not c.dpix[:, c.ref["fragile"].reshape(bp.H, bp.W)].any()


def test_the_scenes_hold_the_cases_they_were_made_for():
    cen = {name: bp.census(bp.case(name)) for name in bp.SCENES}
    for name, v in cen.items():
        print(name, v)
    m, f, o = cen["mixed"], cen["faint"], cen["opaque"]
    assert m["longest_list"] > 256 and m["tiles_over_256"] >= 1              # more than four 64-entry batches
    assert f["pixels_stopped_early"] == 0 and f["occluded"] == 0             # every list walked to its end, nothing left unreached
    assert o["clamped_pairs"] > 0 and o["pixels_stopped_early"] > 0.5 * o["pixels"]
    assert 0.05 <= o["occluded"] / o["listed"] <= 0.95                       # listed, would pass the tests, but every such pixel stopped before
    assert o["unreached_listed"] >= o["occluded"]


def test_the_built_scene_holds_every_constructed_case():
    c = bp.case("built")
    _, groups, stack_tile = bp._built()
    lens = c.inp.ranges[:, 1] - c.inp.ranges[:, 0]
    for tile, n in zip(bp.STACK_TILES, bp.STACK_LENGTHS):                    # the list lengths, exactly, and nothing but the stack in them
        assert lens[tile] == n, (tile, int(lens[tile]), n)
        r0 = int(c.inp.ranges[tile, 0])
        assert set(c.inp.point_list[r0:r0 + n].tolist()) == set(stack_tile[tile].tolist())
    assert set(bp.STACK_TILES) | set(bp.OTHER_TILES) == set(range(bp.GX * bp.GY))
    assert c.st["radii"][groups["stack"]].max() <= 4 and c.st["radii"][groups["stack"]].min() >= 1   # 3 sigma < 5 pixels
    listed = np.unique(c.inp.point_list)
    assert len(np.unique(c.st["depths"][listed])) == len(listed)                  # distinct depths: one order, whatever the sort
    t65 = bp.STACK_TILES[bp.STACK_LENGTHS.index(65)]
    for tile, n in zip(bp.STACK_TILES, bp.STACK_LENGTHS):                    # the entries on both sides of every batch boundary contribute
        tl = c.ref["tiles"][tile]
        for pos in (0, 62, 63, 64, 65, 126, 127, 128, 129, 191, 192):
            if pos < n:
                assert tl["contrib"][:, pos].any(), (tile, pos)
    assert c.ref["tiles"][t65]["contrib"][:, 64].any()
    con = {g: bp.group_pairs(c, idx) for g, idx in groups.items()}
    print({g: v for g, v in con.items()})
    for g in ("stack", "needle", "centre", "border", "corner", "subpixel_one", "op_above", "op_5pc", "op_full"):
        assert con[g][0] >= 1 and con[g][1] >= 1, g                          # contributing and listed-but-not-contributing pairs
    for g in ("subpixel_none", "op_below"):                                  # listed everywhere, contributing nowhere
        assert con[g][0] == 0 and con[g][1] >= 1, g
    for i in groups["subpixel_one"]:
        assert bp.group_pairs(c, [i])[0] == 1
    for i in groups["needle"]:                                               # the bounding box covers >= 4 blocks, the ellipse >= 2 and fewer
        box, hit = bp.blocks_reached(c, i)
        assert box >= 4 and 2 <= hit < box, (i, box, hit)
    xy = c.inp.xy[groups["centre"]].astype(np.float64)                       # on the pixel centres at block corners and edges
    want = np.repeat(np.array([(7.0, 7.0), (8.0, 8.0), (7.5, 7.5), (15.5, 8.0)]), 2, axis=0)
    assert np.abs(xy - want).max() <= 1e-5
    on = groups["border"][np.isin(groups["border"], listed)]                 # (two of the sixteen lie so far out that no tile lists them)
    bx, by = c.inp.xy[on].T                                                  # outside each of the four borders, by up to a radius
    r = c.st["radii"][on]
    for k, side in enumerate((bx < -0.5, by < -0.5, bx > bp.W - 0.5, by > bp.H - 0.5)):
        assert side.sum() >= 3
        dist = np.maximum.reduce([-0.5 - bx, -0.5 - by, bx - (bp.W - 0.5), by - (bp.H - 0.5)])[side]
        # left and top: a rectangle that ends before pixel 1 holds no tile, so the list ends at radius - 1.5; right and bottom: the radius
        assert dist.min() < 1.0 and dist.max() > (r[side].max() - 2.0 if k < 2 else r[side].max() - 0.5), (k, dist)
    cx, cy = c.inp.xy[groups["corner"]].T                                    # around the bottom-right tile's partial blocks
    assert ((cx > bp.W - 0.5) | (cy > bp.H - 0.5)).sum() >= 6 and ((cx >= 72) & (cy >= 40)).sum() >= 1
    ops = c.inp.op.astype(np.float64)
    for g, v in (("op_below", (1 - 1e-3) / 255), ("op_above", (1 + 1e-3) / 255), ("op_5pc", 1.05 / 255), ("op_full", 0.9999)):
        assert np.allclose(ops[groups[g]], v, rtol=1e-6), g
    assert (ops[groups["op_below"]] < 1 / 255).all() and (ops[groups["op_above"]] > 1 / 255).all()
    assert c.ref["fragile"].sum() <= 0.01 * bp.W * bp.H


# ---- the comparator can fail --------------------------------------------------------------------------------------------------------
def _rejects(c, got, what):
    fails, _ = bp.compare(c.ref, c.bar, got, what)
    print(f"{what}: {len(fails)} failures" + (f", first: {fails[0]}" if fails else ""))
    assert fails, f"the comparator accepted: {what}"
    return fails


@pytest.mark.parametrize("name", bp.SCENES)
def test_the_comparator_accepts_the_unmodified_yardstick(name):
    c = bp.case(name)
    for got in (c.yard, c.own):   # the oracle's forward beside the yardstick's sums; the yardstick's own forward
        fails, figs = bp.compare(c.ref, c.bar, got, name)
        assert not fails, fails
    for line in bp.table(name + " yardstick, own forward", c.bar, figs):
        print(line)


def test_the_comparator_rejects_a_lost_block():
    """all pairs of one 8x8 block removed from a Gaussian for which that block carries >= 1 % of a slot's magnitude: the (Gaussian,
    block) whose largest share is the smallest such one"""
    c = bp.case("mixed")
    with np.errstate(invalid="ignore", divide="ignore"):
        share = np.nan_to_num(c.ref["block_mag"] / c.ref["mag"][:, None, :]).max(axis=2)     # [P, blocks]
    share = np.where(share >= 0.01, share, np.inf)
    g, b = np.unravel_index(np.argmin(share), share.shape)
    assert np.isfinite(share[g, b])
    print(f"Gaussian {g}, block {b}: largest share of a slot's magnitude {share[g, b]:.4f}")
    got = dict(c.yard, sums=bp.yardstick(c.inp, c.dpix, drop_block=(int(g), int(b)))["sums"])
    assert not np.array_equal(got["sums"][g], c.yard["sums"][g])
    _rejects(c, got, "lost block")


def test_the_comparator_rejects_a_lost_lane():
    """lane 0 of the second batch of the 65-entry tile (list position 64) dropped from both walks"""
    c = bp.case("built")
    tile = bp.STACK_TILES[bp.STACK_LENGTHS.index(65)]
    got = bp.yardstick(c.inp, c.dpix, drop_entries={(tile, 64)})
    fails = _rejects(c, got, "lost lane")
    lost = int(c.inp.point_list[int(c.inp.ranges[tile, 0]) + 64])
    assert not got["sums"][lost].any() and (c.ref["mag"][lost] > 0).any()
    # ... and by the sums alone: the Gaussian's row is zero where its magnitudes are not
    assert bp.compare(c.ref, c.bar, dict(c.yard, sums=got["sums"]), "lost lane, sums only")[0]
    assert len(fails) >= 2


def test_the_comparator_rejects_n_contrib_off_by_one():
    c = bp.case("mixed")
    pixel = int(np.flatnonzero(~c.ref["fragile"] & (c.ref["n_contrib"] > 0))[7])
    for delta in (1, -1):
        nc = c.yard["n_contrib"].astype(np.int64)
        nc[pixel] += delta
        _rejects(c, dict(c.yard, n_contrib=nc), f"n_contrib {delta:+d} at pixel {pixel}")


def test_the_comparator_rejects_another_stop_threshold():
    c = bp.case("opaque")
    _rejects(c, bp.yardstick(c.inp, c.dpix, stop=2e-4), "stop at 2e-4")


def test_the_comparator_rejects_a_missing_clamp():
    c = bp.case("opaque")
    _rejects(c, bp.yardstick(c.inp, c.dpix, clamp=False), "no 0.99 clamp")


@pytest.mark.parametrize("name", bp.SCENES)
def test_the_comparator_rejects_a_missing_background_term(name):
    c = bp.case(name)
    _rejects(c, dict(c.yard, sums=bp.yardstick(c.inp, c.dpix, bg_term=False)["sums"]), "no background term in dL_dalpha")
