"""The case table of the optimiser tests (tests/test_optim_reference.py on the CPU, tests/test_gpu_optim_elements.py on the GPU):
Adam through the flat and the per-tensor entry points, the SH gradient over views with its fused Adam, and the activations.  Every
entry names the code path it is there for.  For every case: the inputs (seeded by the case's name), the float64 restatement
(oracle/optim_reference.py), the two float32 yardsticks and their error distributions, computed once and shared (nobody writes into
what these functions return).

err = |got - ref64| / max(magnitude, 2^-126): below the smallest normal float32 the format itself resolves no finer than 2^-149, so a
subnormal result is held to roundings of 2^-126, not of itself.  Where a magnitude is exactly 0 the value must be exactly 0."""
import collections
import functools
import zlib

import numpy as np
import torch

from oracle import optim_reference as orf

ULP = 2.0 ** -24
TINY = 2.0 ** -126
MIN_ELEMENTS = 64   # below this a case has no distribution of its own: its yardstick is its family's over the size sweep
F = np.float32

# ---- Adam through sgr_adam_step / _ex (k_adam) ---------------------------------------------------------------------------------
TURN = 8192 * 256 * 4            # elements one turn of k_adam's grid-stride loop covers (the grid is capped at 8192 workgroups)
BIG = TURN + 3 * 1024 + 3        # three more workgroups' worth in the second turn, and a tail of three
LR_A, LR_B = 2.5e-3, 2.5e-3 / 20.0
SIZES = (1, 3, 4, 5, 7, 255, 256, 257, 1027)
N_TABLE = 4099                   # 16 waves of 64 float4 and a tail of three: room for the boundaries at 5, 1030 and 2048
LAYOUT_P, LAYOUT_M = 67, 16


def gaussian_layout(P, M):
    """GaussianParams._layout and FlatAdam's segment table: five tensors, each padded to a multiple of 64 floats -> (segments, n)"""
    from sugar_amd.train_step import GaussianParams as G
    sizes = dict(xyz=3 * P, features=3 * M * P, opacity=P, scaling=3 * P, rotation=4 * P)
    segs, off = [], 0
    for k in G.NAMES:
        segs.append((off, off + sizes[k], G.LRS[k], G.REST_LR, 3 * M, 3) if k == "features" else (off, off + sizes[k], G.LRS[k], G.LRS[k], 1, 1))
        off += (sizes[k] + 63) // 64 * 64
    return segs, off


TABLES = {
    "none": lambda n: [],
    "one": lambda n: [(0, n, 1e-3, 1e-3, 1, 1)],
    "layout": lambda n: gaussian_layout(LAYOUT_P, LAYOUT_M)[0],
    "bounds": lambda n: [(0, 5, 1e-3, 1e-3, 1, 1), (5, 1030, 5e-2, 5e-2, 1, 1), (1030, 2048, 1.6e-4, 1.6e-4, 1, 1), (2048, n, 5e-3, 5e-3, 1, 1)],
    "sweep": lambda n: [(-3, n, LR_A, LR_B, 7, 2)],   # (the size sweep's: from an odd element before the buffer, so n = 1 has a learning rate)
    "periodic7": lambda n: [(3, n, LR_A, LR_B, 7, 2)],
    "periodic48": lambda n: [(1, n, LR_A, LR_B, 48, 3)],
    "periodic_eq": lambda n: [(1, n, LR_A, LR_A, 48, 3)],
    "eight": lambda n: [(0, 64, 1e-3, 1e-3, 1, 1), (64, 100, LR_A, LR_B, 7, 2), (100, 1030, 5e-2, 5e-2, 1, 1), (1000, 1100, 2e-3, 2e-3, 1, 1),
                        (1100, 2048, 1.6e-4, 1.6e-4, 1, 1), (2048, 2049, 7e-3, 7e-3, 1, 1), (2101, 3000, LR_A, LR_B, 48, 3),
                        (3500, n, 5e-3, 5e-3, 0, 1)],
    "far": lambda n: [(-(2 ** 32) - 12345, n, LR_A, LR_B, 48, 3)],
    "big": lambda n: [(0, TURN + 1030, 1e-3, 1e-3, 1, 1), (TURN + 1031, n, LR_A, LR_B, 48, 3)],
}

AdamCase = collections.namedtuple("AdamCase", "name n table family extra_n grad_scale step betas eps path")
FAMILIES = ("normal", "p0", "zero", "tiny25", "tiny21", "decades", "overflow")


def _adam(name, n, table, family, path, extra_n=None, grad_scale=1.0, step=3, betas=(0.9, 0.999), eps=1e-15):
    return AdamCase(name, n, table, family, extra_n, grad_scale, step, betas, eps, path)


def _adam_cases():
    out = []
    paths = {1: "n4 = 0: the tail alone", 3: "n4 = 0: a tail of three", 4: "one float4, no tail", 5: "one float4 and a tail of one",
             7: "one float4 and a tail of three", 255: "a partial wave and a tail", 256: "exactly one wave of float4s",
             257: "one wave and a tail of one", 1027: "two workgroups; the tail runs in the first"}
    for n in SIZES:
        for fam in ("normal", "p0"):
            out.append(_adam(f"n{n}-sweep-{fam}", n, "sweep", fam, paths[n] + "; period 7, split 2, phase 3 at element 0"))
    why = dict(none="n_seg = 0: every learning rate 0, p bit-equal, m and v still move", one="one segment over everything",
               layout="GaussianParams' layout for P = 67, M = 16: gaps padded to 64 (lr 0 there), the SH tensor periodic (48, 3)",
               bounds="boundaries at 5 (splits a float4), 1030 (inside a wave, off a float4 boundary), 2048 (a wave boundary)",
               periodic7="period 7, split 2, from the odd element 3", periodic48="period 48, split 3, from the odd element 1",
               periodic_eq="a periodic segment with lr_a == lr_b: the early return",
               eight="eight segments (the maximum): overlap (the last wins), gaps, a one-element segment, period 0 (counts as 1)",
               far="begin more than 2^32 elements before element 0: the 64-bit remainder of lr_of4")
    for table, text in why.items():
        n = gaussian_layout(LAYOUT_P, LAYOUT_M)[1] if table == "layout" else N_TABLE
        for fam in ("normal", "p0"):
            out.append(_adam(f"{table}-{fam}", n, table, fam, text))
    out.append(_adam("big-p0", BIG, "big", "p0", "the second turn of the grid-stride loop, with a segment boundary, a gap and a periodic "
                     "segment inside it, and the tail"))
    for x, text in ((0, "sgr_adam_step_ex with extra_n = 0"), (1, "the first element alone"), (3 * LAYOUT_P, "3 * 67 = 201: ends inside a float4"),
                    (N_TABLE - 1, "ends inside the tail"), (N_TABLE, "every element")):
        out.append(_adam(f"extra{x}-p0", N_TABLE, "bounds", "p0", "extra: " + text, extra_n=x, grad_scale=0.25))
    for gs in (0.25, 0.0):
        out.append(_adam(f"gradscale{gs:g}-p0", 1027, "periodic48", "p0", f"grad_scale = {gs:g}", grad_scale=gs))
    for step in (1, 2, 1000, 30000):
        out.append(_adam(f"step{step}-p0", 1027, "periodic48", "p0", f"the bias corrections at step {step}", step=step))
    out.append(_adam("betas0-p0", 1027, "periodic48", "p0", "betas (0, 0.5): m' = g", betas=(0.0, 0.5)))
    out.append(_adam("eps1e-8-p0", 1027, "periodic48", "p0", "eps = 1e-8", eps=1e-8))
    out.append(_adam("eps1e-8-tiny21", 1027, "periodic48", "tiny21", "eps = 1e-8 over a subnormal v", eps=1e-8))
    texts = dict(zero="g = m = v = 0 exactly: the update is exactly 0, not NaN", tiny25="|g| = 1e-25: g * g underflows to 0",
                 tiny21="|g| in 1e-21 .. 1e-20: v is subnormal, sqrtf meets a subnormal",
                 decades="signs and magnitudes over 12 decades in one wave",
                 overflow="|g| = 1e20 and, at the odd elements, 1e21, where omb2 * g * g is inf: only the finite / non-finite pattern and the finite values, against yardstick (a)")
    for fam, text in texts.items():
        out.append(_adam(f"n1027-periodic48-{fam}", 1027, "periodic48", fam, text))
    return out


ADAM_CASES = _adam_cases()
ADAM = {c.name: c for c in ADAM_CASES}
assert len(ADAM) == len(ADAM_CASES)


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _signed(r, n, lo, hi):
    """random signs, magnitudes log-uniform in 10^lo .. 10^hi"""
    return (np.where(r.random(n) < 0.5, -1.0, 1.0) * 10.0 ** r.uniform(lo, hi, n)).astype(F)


@functools.lru_cache(maxsize=None)
def adam_inputs(name):
    """-> dict(p, g, m, v, extra (or None), lr, segments) float32; m and v are what one earlier step on a gradient g0 leaves"""
    c = ADAM[name]
    r, n = _rng(name), c.n
    with np.errstate(all="ignore"):
        if c.family in ("normal", "p0"):
            g, g0 = (0.01 * r.standard_normal(n)).astype(F), (0.01 * r.standard_normal(n)).astype(F)
        elif c.family == "zero":
            g = g0 = np.zeros(n, F)
        elif c.family == "tiny25":
            g, g0 = _signed(r, n, -25, -24.7), _signed(r, n, -25, -24.7)
        elif c.family == "tiny21":
            g, g0 = _signed(r, n, -21, -20), _signed(r, n, -21, -20)
        elif c.family == "decades":
            g, g0 = _signed(r, n, -9, 3), _signed(r, n, -9, 3)
        elif c.family == "overflow":
            g, g0 = _signed(r, n, 20, 20), _signed(r, n, 14, 14)
            g[1::2] *= F(10)   # (omb2 * g * g is formed as (omb2 * g) * g: finite at 1e20, inf at 1e21)
        m, v = F(0.1) * g0, F(0.001) * g0 * g0
        p = np.zeros(n, F) if c.family in ("p0", "tiny25", "tiny21", "decades") else r.standard_normal(n).astype(F)
    extra = None if c.extra_n is None else (0.01 * r.standard_normal(c.extra_n)).astype(F)
    segments = TABLES[c.table](n)
    return dict(p=p, g=g, m=m, v=v, extra=extra, segments=segments, lr=orf.segment_lr(n, segments))


def other_lr(n, segments):
    """the learning rate an element would get had its periodic segment chosen the other way"""
    return orf.segment_lr(n, [(b, e, lb, la, period, split) for b, e, la, lb, period, split in segments])


def adam_args(c, step=None):
    return dict(beta1=c.betas[0], beta2=c.betas[1], eps=c.eps, step=c.step if step is None else step, grad_scale=c.grad_scale)


def element_err(got, ref, mag):
    """the module docstring's err over the elements with magnitude > 0 (flat)"""
    got, ref, mag = (np.asarray(a, np.float64).reshape(-1) for a in (got, ref, mag))
    live = mag > 0
    assert not got[~live].any(), ("an element whose magnitude is exactly 0 must be exactly 0", np.flatnonzero(~live & (got != 0))[:8])
    return np.abs(got - ref)[live] / np.maximum(mag[live], TINY)


CHUNK = 1 << 20


def adam_err(name, got, state=None, step=None):
    """got = (p', m', v') of one step of case `name` (at `step`, default the case's) from `state` (p, m, v; default: the case's inputs)
    -> dict(p, m, v, u) of element errors.  In chunks: the float64 restatement of the 8.4M-element case is never whole in memory."""
    c, i = ADAM[name], adam_inputs(name)
    p, m, v = state if state is not None else (i["p"], i["m"], i["v"])
    errs = dict(p=[], m=[], v=[], u=[])   # u: p' again, on the scale on which the update is well conditioned (mags["p_cond"])
    for a in range(0, c.n, CHUNK):
        b = min(a + CHUNK, c.n)
        ex = None if i["extra"] is None else i["extra"][a:b]   # (extra covers a prefix: a chunk's share is a prefix of the chunk)
        p1, m1, v1, mags = orf.adam_step(p[a:b], i["g"][a:b], m[a:b], v[a:b], i["lr"][a:b], extra=ex, **adam_args(c, step))
        for k, j, ref, mag in (("p", 0, p1, "p"), ("m", 1, m1, "m"), ("v", 2, v1, "v"), ("u", 0, p1, "p_cond")):
            errs[k].append(element_err(got[j][a:b], ref, mags[mag]))
    return {k: np.concatenate(e) for k, e in errs.items()}


def adam_yardsticks(name, state=None, step=None):
    """-> (yardstick (a)'s (p', m', v'), yardstick (b)'s)"""
    c, i = ADAM[name], adam_inputs(name)
    p, m, v = state if state is not None else (i["p"], i["m"], i["v"])
    args = (p, i["g"], m, v, i["lr"])
    return orf.adam_step_f32(*args, extra=i["extra"], **adam_args(c, step)), orf.adam_step_torch(*args, extra=i["extra"], **adam_args(c, step))


def adam_bar_from(name, state, step):
    """the bars of one step of a chain: both yardsticks start from `state`, as the kernel did"""
    ya, yb = adam_yardsticks(name, state, step)
    ea, eb = adam_err(name, ya, state, step), adam_err(name, yb, state, step)
    return {k: _bar(f"{name} step {step} {k}'", ea[k], eb[k]) for k in "pmvu"}


Bar = collections.namedtuple("Bar", "worst median lines pooled")


def _bar(label, ea, eb, pooled=False):
    """Y = the worse of the two yardsticks, floored at one rounding -> the kernel's bar: worst <= 4 x Y's worst, median <= 2 x Y's"""
    where = " (the family over the size sweep)" if pooled else ""
    lines = [describe(f"{label} yardstick (a){where}", ea), describe(f"{label} yardstick (b){where}", eb)]
    if not len(ea):
        return Bar(4 * ULP, 2 * ULP, lines, pooled)
    return Bar(4 * max(ea.max(), eb.max(), ULP), 2 * max(np.median(ea), np.median(eb), ULP), lines, pooled)


@functools.lru_cache(maxsize=None)
def _adam_yardstick_err(name):
    ya, yb = adam_yardsticks(name)
    return adam_err(name, ya), adam_err(name, yb)


@functools.lru_cache(maxsize=None)
def adam_bar(name):
    """-> dict(p, m, v, u) of Bar.  A case with fewer than MIN_ELEMENTS elements takes the errors of its family over the whole size sweep"""
    c = ADAM[name]
    names = [name]
    pooled = c.n < MIN_ELEMENTS
    if pooled:
        names = sweep_names(name)
    errs = [_adam_yardstick_err(k) for k in names]
    if c.n > CHUNK:
        _adam_yardstick_err.cache_clear()   # (the big case's arrays are not worth keeping)
    return {k: _bar(f"{name} {k}'", np.concatenate([e[0][k] for e in errs]), np.concatenate([e[1][k] for e in errs]), pooled) for k in "pmvu"}


def bar_from(label, ref, mag, ya, yb):
    """the bar of one output from its two yardstick values"""
    return _bar(label, element_err(ya, ref, mag), element_err(yb, ref, mag))


def describe(name, err):
    if not len(err):
        return f"{name}: no elements"
    return f"{name}: elements {len(err)} max {err.max():.3e} median {np.median(err):.3e} p99 {np.quantile(err, 0.99):.3e}"


def check(label, err, bar, out=print, pool=None):
    """print the three distributions, then hold the kernel's to the bar.  pool: the kernel's errors over the same cases the bar's
    yardsticks were pooled over (a case of fewer than MIN_ELEMENTS elements): the median of three or four elements is no estimate of a
    distribution's median and is not compared with that of 1815; the case's own elements face the worst-element bar, and the median is
    taken over the pool on both sides"""
    for line in bar.lines:
        out(line)
    out(describe(f"{label} kernel", err))
    if not len(err):
        return
    assert err.max() <= bar.worst, (label, "worst element", float(err.max()), "at", int(np.argmax(err)), "bar", bar.worst)
    if pool is not None:
        out(describe(f"{label} kernel (the family over the size sweep)", pool))
        err = pool
    assert np.median(err) <= bar.median, (label, "median", float(np.median(err)), "bar", bar.median)


def sweep_names(name):
    """the cases a case of fewer than MIN_ELEMENTS elements is pooled with: its family over the size sweep"""
    c = ADAM[name]
    names = [f"n{n}-{c.table}-{c.family}" for n in SIZES]
    assert name in names, name
    return names


# ---- Adam over several tensors (k_adam_multi) ----------------------------------------------------------------------------------
BIG_MULTI = 4096 * 256 * 4 + 1027   # k_adam_multi caps a tensor at 4096 workgroups: the second turn of its loop, and a tail
MULTI_CASES = {
    "one": ((14997,), "one tensor"),
    "six": ((14997, 0, 1, 3, 4, 1027), "six tensors as the reference has, an empty one among them; 14997 = 4999 * 3"),
    "eight": ((4, 14997, 3, 0, BIG_MULTI, 1, 257, 5), "eight tensors (the maximum); the fifth turns the grid-stride loop a second time"),
}


@functools.lru_cache(maxsize=None)
def multi_inputs(name):
    """-> list of dict(p, g, m, v, lr, beta1, beta2, eps, step) per tensor: every argument differs from tensor to tensor"""
    r = _rng("multi-" + name)
    out = []
    for t, n in enumerate(MULTI_CASES[name][0]):
        g, g0 = (0.01 * r.standard_normal(n)).astype(F), (0.01 * r.standard_normal(n)).astype(F)
        out.append(dict(p=np.zeros(n, F) if t % 2 else r.standard_normal(n).astype(F), g=g, m=F(0.1) * g0, v=F(0.001) * g0 * g0,
                        lr=1e-3 * (t + 1), beta1=(0.9, 0.8, 0.0, 0.95)[t % 4], beta2=(0.999, 0.99, 0.5, 0.9)[t % 4],
                        eps=(1e-15, 1e-8, 1e-12)[t % 3], step=(1, 2, 7, 1000, 30000)[t % 5]))
    return out


# ---- the SH gradient over views and its Adam (k_sh_grad_from_views, k_sh_adam_from_views) ------------------------------------------
ShCase = collections.namedtuple("ShCase", "name P V stride D M offset lr_dc lr_rest colour path")
SH_ARGS = dict(beta1=0.9, beta2=0.999, eps=1e-15, step=7, grad_scale=0.5)
DEGREES = ((0, 1), (1, 4), (2, 9), (3, 16), (2, 16), (0, 16))


def _sh_cases():
    out = []
    add = lambda *a: out.append(ShCase(*a))
    for P in (1, 63, 64, 65, 130):
        for D, M in DEGREES:
            add(f"P{P}-D{D}M{M}", P, 3, 0, D, M, 0, LR_A, LR_B, "random",
                f"{'the 64 x 48 panel walk' if M == 16 else 'n_sh != 48: the scalar loop'}; "
                f"{'one full wave' if P == 64 else 'a partial last wave'}" + ("; coefficients above the degree get gradient 0" if M > (D + 1) ** 2 else ""))
    for V in (1, 4):
        for stride in ("P", "P+1"):
            add(f"P65-V{V}-stride{stride}", 65, V, stride, 3, 16, 0, LR_A, LR_B, "random", f"{V} views, view_stride = {stride}")
    for P in (65, 130):
        add(f"P{P}-misaligned", P, 3, 0, 3, 16, 4, LR_A, LR_B, "random", "sh, exp_avg, exp_avg_sq one float past 16-byte alignment: the scalar loop at M = 16")
    add("P65-lr0", 65, 3, 0, 3, 16, 0, 0.0, 0.0, "random", "both learning rates 0: sh bit-equal, m and v move")
    for colour, text in (("some", "all three colour gradients exactly 0 in some views"), ("none", "exactly 0 in every view"),
                         ("channel", "one channel only")):
        add(f"P130-{colour}", 130, 4, "P+1", 3, 16, 0, LR_A, LR_B, colour, text)
    return out


SH_CASES = _sh_cases()
SH = {c.name: c for c in SH_CASES}
assert len(SH) == len(SH_CASES)


def sh_view_stride(c):
    return {0: 0, "P": c.P, "P+1": c.P + 1}[c.stride]


@functools.lru_cache(maxsize=None)
def sh_inputs(name):
    """-> dict(means [P, 3], campos [V, 3], dcolor [V, P, 3], sh, m, v [P, M, 3]) float32; |mean - campos| >= 1.4"""
    c = SH[name]
    r = _rng("sh-" + name)
    means = np.clip(0.5 * r.standard_normal((c.P, 3)), -1.5, 1.5).astype(F)
    campos = r.standard_normal((c.V, 3))
    campos = (4.0 * campos / np.linalg.norm(campos, axis=1, keepdims=True)).astype(F)
    dcolor = (0.01 * r.standard_normal((c.V, c.P, 3))).astype(F)
    if c.colour == "some":
        dcolor[r.random((c.V, c.P)) < 0.4] = 0
        dcolor[0, 0] = dcolor[c.V - 1, c.P - 1] = 0
    elif c.colour == "none":
        dcolor[:] = 0
    elif c.colour == "channel":
        dcolor[..., 0] = dcolor[..., 2] = 0
    assert np.linalg.norm(means[None] - campos[:, None], axis=2).min() >= 0.1
    shape = (c.P, c.M, 3)
    return dict(means=means, campos=campos, dcolor=dcolor, sh=(0.3 * r.standard_normal(shape)).astype(F),
                m=(1e-3 * r.standard_normal(shape)).astype(F), v=(1e-6 * r.random(shape)).astype(F))


def sh_lr(c):
    lr = np.full((c.P, c.M, 3), c.lr_rest, F)
    lr[:, 0] = c.lr_dc
    return lr


@functools.lru_cache(maxsize=None)
def sh_reference(name):
    """-> dict: grad, grad_mag (float64 [P, M, 3]); grad_a, grad_b (the yardsticks); adam = (p', m', v', mags) of the float64 step on the
    float64 gradient; adam_a, adam_b = the float32 steps on the yardsticks' own gradients"""
    c, i = SH[name], sh_inputs(name)
    t = lambda k: torch.from_numpy(i[k])
    grad, mag = (a.numpy() for a in orf.sh_grad_from_views(t("means"), t("campos"), t("dcolor"), c.D, c.M))
    grad_a = orf.sh_grad_from_views_f32(i["means"], i["campos"], i["dcolor"], c.D, c.M)
    grad_b = orf.sh_grad_from_views(t("means"), t("campos"), t("dcolor"), c.D, c.M, dtype=torch.float32)[0].numpy()
    lr = sh_lr(c)
    return dict(grad=grad, grad_mag=mag, grad_a=grad_a, grad_b=grad_b,
                adam=orf.adam_step(i["sh"], grad, i["m"], i["v"], lr, g_mag=mag, **SH_ARGS),
                adam_a=orf.adam_step_f32(i["sh"], grad_a, i["m"], i["v"], lr, **SH_ARGS),
                adam_b=orf.adam_step_torch(i["sh"], grad_b, i["m"], i["v"], lr, **SH_ARGS))


def sh_bars(name):
    """-> dict(grad, p, m, v) of Bar"""
    r = sh_reference(name)
    bars = dict(grad=bar_from(f"{name} dL_dsh", r["grad"], r["grad_mag"], r["grad_a"], r["grad_b"]))
    for j, k in enumerate("pmv"):
        bars[k] = bar_from(f"{name} {k}'", r["adam"][j], r["adam"][3][k], r["adam_a"][j], r["adam_b"][j])
    return bars


def row_err(got, ref):
    """per row (Gaussian): max |got - ref| on the scale of the row's largest |ref|; a row whose reference is all 0 must be all 0"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    top = np.abs(ref).max(1)
    assert not got[top == 0].any()
    return np.abs(got - ref).max(1)[top > 0] / np.maximum(top[top > 0], TINY)


# ---- activations (k_activations_fwd / _bwd) ------------------------------------------------------------------------------------
ACT_SIZES = (1, 255, 256, 257)
ACT_FAMILIES = {
    "typical": "scaling in [-12, 3], opacity in [-20, 20], quaternions scaled by 3.7",
    "edges": "quaternions exactly 0, of length 3e-13 (below the clamp), 1e-25 (the squares underflow); opacity -0.0",
    "saturating": "scaling +-88.7 and +-104, opacity +-90, quaternions of length 1e20: the finite / non-finite pattern of yardstick (b)",
}
ACT_CASES = [(P, fam) for P in ACT_SIZES for fam in ACT_FAMILIES]


@functools.lru_cache(maxsize=None)
def act_inputs(P, family):
    """-> dict(scaling [P, 3], rotation [P, 4], opacity [P, 1], d_scales, d_rotations, d_opacities) float32"""
    r = _rng(f"act-{P}-{family}")
    scaling = r.uniform(-12, 3, (P, 3)).astype(F)
    opacity = r.uniform(-20, 20, (P, 1)).astype(F)
    unit = r.standard_normal((P, 4))
    unit /= np.linalg.norm(unit, axis=1, keepdims=True)
    rotation = (3.7 * r.standard_normal((P, 4))).astype(F)
    rows = np.arange(P)
    if family == "edges":
        length = np.choose(rows % 4, [1.0, 0.0, 3e-13, 1e-25])[:, None]
        rotation = np.where(length == 1.0, rotation, unit * length).astype(F)
        opacity[rows % 3 == 1] = F(-0.0)
    elif family == "saturating":
        scaling = np.choose((rows[:, None] + np.arange(3)[None]) % 4, [88.7, -88.7, 104.0, -104.0]).astype(F)
        opacity = np.where(rows % 2 == 0, 90.0, -90.0).astype(F)[:, None]
        rotation = (unit * 1e20).astype(F)
    grads = {k: r.standard_normal(s).astype(F) for k, s in (("d_scales", (P, 3)), ("d_rotations", (P, 4)), ("d_opacities", (P, 1)))}
    return dict(scaling=scaling, rotation=rotation, opacity=opacity, **grads)


ACT_ORDER = ("scaling", "rotation", "opacity", "d_scales", "d_rotations", "d_opacities")


@functools.lru_cache(maxsize=None)
def act_reference(P, family):
    """-> dict(fwd, fwd_mag, bwd, bwd_mag float64; a = (fwd, bwd) of yardstick (a); b = of yardstick (b))"""
    a = [act_inputs(P, family)[k] for k in ACT_ORDER]
    fwd, fwd_mag = orf.activations_fwd(*a[:3])
    bwd, bwd_mag = orf.activations_bwd(*a)
    return dict(fwd=fwd, fwd_mag=fwd_mag, bwd=bwd, bwd_mag=bwd_mag, a=orf.activations_f32(*a), b=orf.activations_torch(*a))


def act_bars(P, family):
    """-> dict(fwd, bwd) of dict(output -> Bar); a case of fewer than MIN_ELEMENTS rows takes its family at every size"""
    sizes = ACT_SIZES if P < MIN_ELEMENTS else (P,)
    refs = [act_reference(s, family) for s in sizes]
    bars = {}
    for j, way in enumerate(("fwd", "bwd")):
        bars[way] = {}
        for k in refs[0][way]:
            ea = np.concatenate([finite_err(r["a"][j][k], r[way][k], r[way + "_mag"][k], r["b"][j][k]) for r in refs])
            eb = np.concatenate([finite_err(r["b"][j][k], r[way][k], r[way + "_mag"][k], r["b"][j][k]) for r in refs])
            bars[way][k] = _bar(f"{P}-{family} {way} {k}", ea, eb, len(sizes) > 1)
    return bars


def finite_err(got, ref, mag, pattern):
    """element_err over the elements at which `pattern` (yardstick (b)'s result) is finite"""
    keep = np.isfinite(np.asarray(pattern)).reshape(-1) & np.isfinite(np.asarray(ref, np.float64)).reshape(-1)
    sel = lambda a: np.asarray(a, np.float64).reshape(-1)[keep]
    return element_err(sel(got), sel(ref), sel(mag))
