"""CPU tests of the float64 restatements of the optimiser side (oracle/optim_reference.py) over the case table of
tests/optim_cases.py: Adam against torch.optim.Adam in float64, the SH gradient and the activations against float64 autograd,
|result| <= condition magnitude, segment_lr against a brute-force loop, the intended-double rule, and the conditions
tests/test_gpu_optim_elements.py relies on (the yardsticks' normalised errors exist and are finite).  Run with -s for the yardsticks'
error distributions."""
import numpy as np
import pytest
import torch

from oracle import optim_reference as orf
from tests import optim_cases as oc

SMALL_ADAM = [c.name for c in oc.ADAM_CASES if c.n <= oc.N_TABLE + 200]


def test_the_intended_double_rule():
    for text in ("0.9", "0.999", "0.0", "0.5", "0.95", "0.8", "0.99"):
        assert orf.intended_double(np.float32(float(text))) == float(text), text
    assert orf.intended_double(np.float32(0.999)) != float(np.float32(0.999))
    x = np.float32(1.0) / np.float32(3.0)   # nine digits at the most, and they round back
    assert np.float32(orf.intended_double(x)) == x


def test_the_case_table():
    assert all(c.path for c in oc.ADAM_CASES) and all(c.path for c in oc.SH_CASES)
    assert oc.BIG == 8192 * 256 * 4 + 3 * 1024 + 3 and oc.BIG_MULTI == 4096 * 256 * 4 + 1027
    assert {c.n for c in oc.ADAM_CASES} >= set(oc.SIZES) | {oc.BIG} and set(oc.SIZES) == {1, 3, 4, 5, 7, 255, 256, 257, 1027}
    segs, n = oc.gaussian_layout(67, 16)
    assert n == 4224 and [s[0] for s in segs] == [0, 256, 384, 640, 960] and segs[-1][1] == 960 + 67 * 48 and segs[-1][4:] == (48, 3)
    assert len(oc.TABLES["eight"](oc.N_TABLE)) == 8
    for n in oc.SIZES:   # every element of the size sweep has a learning rate, and from n = 5 on both of them
        lr = oc.adam_inputs(f"n{n}-sweep-p0")["lr"]
        assert lr.all() and (n < 5 or len(set(lr)) == 2)
    big = oc.TABLES["big"](oc.BIG)
    assert oc.TURN < big[0][1] < big[1][0] < oc.BIG and big[1][0] % 2 == 1   # the boundary and the periodic segment lie in the second turn
    assert {c.extra_n for c in oc.ADAM_CASES} >= {None, 0, 1, 201, oc.N_TABLE - 1, oc.N_TABLE}
    assert {c.grad_scale for c in oc.ADAM_CASES} >= {1.0, 0.25, 0.0} and {c.step for c in oc.ADAM_CASES} >= {1, 2, 1000, 30000}
    assert {c.family for c in oc.ADAM_CASES} == set(oc.FAMILIES)
    i = oc.adam_inputs("n1027-periodic48-tiny21")
    v1 = orf.adam_step_f32(i["p"], i["g"], i["m"], i["v"], i["lr"], 0.9, 0.999, 1e-15, 3)[2]
    assert 0 < v1.max() < 2.0 ** -126 and (i["g"] != 0).all()            # v' is subnormal
    i = oc.adam_inputs("n1027-periodic48-tiny25")
    assert not (i["g"] * i["g"]).any() and (i["g"] != 0).all()           # g * g underflows
    i = oc.adam_inputs("n1027-periodic48-decades")
    assert np.log10(np.abs(i["g"][:256]).max() / np.abs(i["g"][:256]).min()) > 11 and (i["g"][:256] < 0).any() and (i["g"][:256] > 0).any()
    assert {(c.P, c.D, c.M) for c in oc.SH_CASES} >= {(P, D, M) for P in (1, 63, 64, 65, 130) for D, M in oc.DEGREES}
    assert {c.V for c in oc.SH_CASES} == {1, 3, 4} and {c.stride for c in oc.SH_CASES} == {0, "P", "P+1"}
    d = oc.sh_inputs("P130-some")["dcolor"]
    assert ((d == 0).all(2).any(0) & (d != 0).any(2).any(0)).any() and not oc.sh_inputs("P130-none")["dcolor"].any()
    a = oc.act_inputs(257, "edges")
    n = np.linalg.norm(a["rotation"].astype(np.float64), axis=1)
    assert (n[1::4] == 0).all() and (abs(n[2::4] - 3e-13) < 1e-19).all() and (abs(n[3::4] - 1e-25) < 1e-31).all() and (n[0::4] > 0.1).all()
    assert np.signbit(a["opacity"][1, 0]) and a["opacity"][1, 0] == 0
    a = oc.act_inputs(257, "saturating")
    assert set(np.unique(a["scaling"])) == {np.float32(v) for v in (88.7, -88.7, 104, -104)} and set(np.unique(a["opacity"])) == {-90, 90}


@pytest.mark.parametrize("table", list(oc.TABLES))
def test_segment_lr_against_a_brute_force_loop(table):
    n = oc.BIG if table == "big" else 4224 if table == "layout" else oc.N_TABLE
    segments = oc.TABLES[table](n)
    lr = orf.segment_lr(n, segments)
    assert lr.dtype == np.float32 and lr.shape == (n,)
    probe = range(n) if n < 10000 else list(range(0, 4096)) + list(range(oc.TURN - 300, n))
    for e in probe:
        want = 0.0
        for begin, end, la, lb, period, split in segments:   # the last listed segment that holds e wins
            if begin <= e < end:
                want = la if (e - begin) % max(period, 1) < split else lb
        assert lr[e] == np.float32(want), (table, e)
    if table == "far":
        assert lr[0] == np.float32(oc.LR_A if (2 ** 32 + 12345) % 48 < 3 else oc.LR_B) and len(set(lr)) == 2
    if table in ("periodic7", "periodic48", "far", "big"):
        assert (oc.other_lr(n, segments) != lr)[segments[-1][0] if segments[-1][0] > 0 else 0:].all()


def _reference_groups(P, rng):
    """the reference's six groups (gaussian_model.py:152-166): xyz, f_dc, f_rest, opacity, scaling, rotation"""
    shapes = dict(xyz=(P, 3), f_dc=(P, 1, 3), f_rest=(P, 15, 3), opacity=(P, 1), scaling=(P, 3), rotation=(P, 4))
    lrs = dict(xyz=0.00016, f_dc=0.0025, f_rest=0.0025 / 20.0, opacity=0.05, scaling=0.005, rotation=0.001)
    return {k: (rng.standard_normal(s).astype(np.float32), lrs[k]) for k, s in shapes.items()}


def test_adam_against_torch_adam_in_float64_over_five_chained_steps():
    """six groups shaped like the reference's, the position learning rate changed before the third step (update_learning_rate); the
    learning rates are float32 values, as the C ABI carries them: parameters, m and v agree to 1e-12 relative after every step"""
    rng = np.random.default_rng(12)
    groups = {k: (a, float(np.float32(lr))) for k, (a, lr) in _reference_groups(23, rng).items()}
    params = {k: torch.from_numpy(a.astype(np.float64)).requires_grad_(True) for k, (a, _) in groups.items()}
    opt = torch.optim.Adam([dict(params=[params[k]], lr=lr, name=k) for k, (_, lr) in groups.items()], lr=0.0, eps=float(np.float32(1e-15)),
                           foreach=False)
    state = {k: (a.astype(np.float64), np.zeros(a.shape), np.zeros(a.shape)) for k, (a, _) in groups.items()}
    lrs = {k: lr for k, (_, lr) in groups.items()}
    for step in range(1, 6):
        if step == 3:
            lrs["xyz"] = float(np.float32(0.00011))
            opt.param_groups[0]["lr"] = lrs["xyz"]
        for k in params:
            g = (0.01 * rng.standard_normal(params[k].shape)).astype(np.float32)
            params[k].grad = torch.from_numpy(g.astype(np.float64))
            p, m, v = state[k]
            state[k] = orf.adam_step(p, g, m, v, np.full(g.shape, lrs[k]), 0.9, 0.999, 1e-15, step)[:3]
        opt.step()
        for k in params:
            st = opt.state[params[k]]
            for got, want in zip(state[k], (params[k].detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy())):
                assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (k, step)


@pytest.mark.parametrize("name", SMALL_ADAM + ["big-p0"])
def test_adam_yardsticks(name):
    """|result| <= magnitude; the yardsticks' errors exist, are finite and small; their distributions are printed"""
    c, i = oc.ADAM[name], oc.adam_inputs(name)
    s = slice(max(0, c.n - 8192), c.n)   # (of the big case: its end)
    p1, m1, v1, mags = orf.adam_step(i["p"][s], i["g"][s], i["m"][s], i["v"][s], i["lr"][s], extra=i["extra"], **oc.adam_args(c))
    assert (np.abs(m1) <= mags["m"] * (1 + 1e-12)).all() and (np.abs(p1) <= mags["p"] * (1 + 1e-12)).all() and (v1 >= 0).all()
    if c.family == "overflow":
        ya, yb = oc.adam_yardsticks(name)
        # (omb2 * g * g is (omb2 * g) * g: 1e37 at |g| = 1e20, inf at 1e21, where the update is m' / inf = 0)
        assert np.isinf(ya[2][1::2]).all() and np.isfinite(ya[2][0::2]).all() and np.isfinite(ya[0]).all() and np.isfinite(ya[1]).all()
        assert np.array_equal(ya[0][1::2], i["p"][1::2]) and i["lr"][1:].all()
        return
    if c.family == "zero":
        for y in oc.adam_yardsticks(name):
            assert np.array_equal(y[0], i["p"]) and not y[1].any() and not y[2].any()
    bars = oc.adam_bar(name)
    for k in "pmvu":
        for line in bars[k].lines:
            print(line)
        # (m' and v' are sums of two terms; the update divides by them: where b1 m and (1 - b1) g cancel, a rounding of m' is a large
        # part of the update, for the kernel as for the yardsticks: p' has no bound of its own here)
        assert np.isfinite(bars[k].worst) and (k == "p" or bars[k].worst <= 4 * 64 * oc.ULP), (name, k, bars[k].worst)
    if (i["lr"] == 0).any():
        for y in oc.adam_yardsticks(name):
            assert np.array_equal(y[0][i["lr"] == 0], i["p"][i["lr"] == 0])


@pytest.mark.parametrize("name", [c.name for c in oc.SH_CASES])
def test_sh_gradient_against_float64_autograd(name):
    c, i = oc.SH[name], oc.sh_inputs(name)
    ref = oc.sh_reference(name)
    t = lambda k: torch.from_numpy(i[k]).double()
    sh = t("sh").requires_grad_(True)
    (orf.sh_colors(c.D, sh, t("means"), t("campos")) * t("dcolor")).sum().backward()
    top = max(np.abs(ref["grad"]).max(), 1e-300)
    assert np.abs(sh.grad.numpy() - ref["grad"]).max() <= 1e-12 * top
    assert (np.abs(ref["grad"]) <= ref["grad_mag"] * (1 + 1e-12)).all() and not ref["grad"][:, (c.D + 1) ** 2:].any()
    if c.colour == "none":
        assert not ref["grad_mag"].any() and not ref["grad_a"].any() and not ref["grad_b"].any()
    p1, m1, v1, mags = ref["adam"]
    assert (np.abs(m1) <= mags["m"] * (1 + 1e-12)).all() and (v1 <= mags["v"] * (1 + 1e-12)).all() and (np.abs(p1) <= mags["p"] * (1 + 1e-12)).all()
    for k, bar in oc.sh_bars(name).items():
        for line in bar.lines:
            print(line)
        # (a basis value such as xx - yy cancels within itself: |b_k| is no bound on its own rounding, for the yardsticks as for the kernel)
        assert np.isfinite(bar.worst) and bar.median <= 2 * 4 * oc.ULP, (name, k, bar)
    if c.M == 16:   # the direction term exists and its float32 yardstick is close
        d64 = orf.sh_direction_term(i["means"], i["campos"], i["dcolor"], c.D, i["sh"])
        d32 = orf.sh_direction_term(i["means"], i["campos"], i["dcolor"], c.D, i["sh"], dtype=torch.float32)
        err = oc.row_err(d32, d64)
        print(oc.describe(f"{name} dmean_extra yardstick (float32 autograd)", err))
        assert not len(err) or err.max() < 1e-4
        assert (d64 != 0).any() == (c.D > 0 and c.colour != "none")


@pytest.mark.parametrize("P,family", oc.ACT_CASES)
def test_activations_against_float64_autograd(P, family):
    a = [oc.act_inputs(P, family)[k] for k in oc.ACT_ORDER]
    ref = oc.act_reference(P, family)
    fwd, bwd = orf.activations_torch(*a, dtype=torch.float64)
    for k in ref["fwd"]:
        assert np.abs(ref["fwd"][k] - fwd[k]).max() <= 1e-12 * max(np.abs(fwd[k]).max(), 1e-300), k
        assert (np.abs(ref["fwd"][k]) <= ref["fwd_mag"][k] * (1 + 1e-12)).all()
    for k in ref["bwd"]:
        assert np.abs(ref["bwd"][k] - bwd[k]).max() <= 1e-12 * max(np.abs(bwd[k]).max(), 1e-300), k
        assert (np.abs(ref["bwd"][k]) <= ref["bwd_mag"][k] * (1 + 1e-12)).all()
    if family == "edges":
        assert not ref["fwd"]["rotations"][1::4].any() and np.array_equal(ref["bwd"]["rotation"][1::4], a[4][1::4].astype(np.float64) / 1e-12)
    fa, ba = ref["a"]
    fb, bb = ref["b"]
    for got_a, got_b in ((fa, fb), (ba, bb)):
        for k in got_a:   # the two yardsticks agree on what is finite
            assert np.array_equal(np.isfinite(got_a[k]), np.isfinite(got_b[k])), (family, k)
            assert family == "saturating" or np.isfinite(got_a[k]).all()
    for way, bars in oc.act_bars(P, family).items():
        for k, bar in bars.items():
            for line in bar.lines:
                print(line)
            # (a sigmoid that has rounded to 1 has the derivative 0 in float32, in the yardsticks as in the kernel: d_opacity has no
            # bound of its own here)
            assert np.isfinite(bar.worst)
            assert family == "saturating" or k == "opacity" or bar.worst <= 4 * 64 * oc.ULP, (way, k, bar.worst)
