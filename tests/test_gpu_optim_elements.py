"""GPU tests of the optimiser kernels element by element against the float64 restatements of oracle/optim_reference.py, over the case
table of tests/optim_cases.py, through the C ABI: k_adam (sgr_adam_step / _ex), k_adam_multi (sgr_adam_step_multi),
k_sh_grad_from_views and k_sh_adam_from_views<DIR> (sgr_sh_grad_from_views, sgr_sh_adam_from_views / _ex), k_activations_fwd / _bwd.

Every operand, inputs included, lies inside a larger buffer whose every byte is 0xFF before the call (four such bytes are a float
NaN).  Afterwards no guard byte has changed, the read-only operands are bit-equal to what went in and no NaN has come out of a finite
case.

Bars: err = |got - ref64| / condition magnitude per element (tests/optim_cases.py); the kernel's worst element must lie within 4 x the
worse yardstick's worst and its median within 2 x that yardstick's median, both floored at 2^-24: one differently rounded operation (a
contracted multiply-add in adam.hip, the device's expf) moves a result by one rounding of its magnitude, and yardstick (a) is exact in
many elements.  The yardsticks are float32 CPU evaluations of the same case, never the kernel.  What is claimed exactly is asserted as
bit equality.  All distributions are printed (profiles/optim_elements.txt holds a recorded run)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import optim_reference as orf
from tests import optim_cases as oc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ULP = oc.ULP
GUARD = 16384     # bytes before and after every operand
PATTERN = 0xFF
INVALID = -1      # SGR_E_INVALID
F = np.float32
bits = lambda a: np.ascontiguousarray(a, F).view(np.uint32)
same = lambda a, b: np.array_equal(bits(a), bits(b))


class _Guarded:
    """a float32 array starting `offset` bytes past a 256-byte boundary, GUARD bytes of PATTERN on either side; array=None: `nbytes`
    of PATTERN (an output)"""

    def __init__(self, array=None, offset=0, nbytes=None):
        self.src = None if array is None else np.ascontiguousarray(array, F)
        nbytes = self.src.nbytes if nbytes is None else nbytes
        self.buf = torch.full((2 * GUARD + 256 + offset + nbytes,), PATTERN, dtype=torch.uint8, device=DEV)
        self.a = (-self.buf.data_ptr()) % 256 + GUARD + offset
        self.b = self.a + nbytes
        self.address = self.buf.data_ptr() + self.a
        self.ptr = C.c_void_p(self.address)
        assert self.address % 256 == offset
        if self.src is not None and nbytes:
            self.buf[self.a:self.b].copy_(torch.from_numpy(self.src.reshape(-1).view(np.uint8)))

    def get(self, shape=None):
        out = self.buf[self.a:self.b].cpu().numpy().view(F)
        return out.reshape(self.src.shape if shape is None else shape)

    def intact(self):
        return bool((self.buf[:self.a] == PATTERN).all()) and bool((self.buf[self.b:] == PATTERN).all())

    def unchanged(self):
        return same(self.get(), self.src)


def _lib():
    from sugar_amd import _lib as L
    return L.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _after(operands, read_only=()):
    torch.cuda.synchronize()
    for name, buf in operands.items():
        assert buf.intact(), f"bytes around {name} were written"
    for name in read_only:
        assert operands[name].unchanged(), f"{name} was written"


# ---- k_adam --------------------------------------------------------------------------------------------------------------------
def _seg_arrays(segments, n_seg=None):
    n = max(len(segments), 1)
    cols = list(zip(*segments)) if segments else [(0,)] * 6
    types = (C.c_longlong, C.c_longlong, C.c_float, C.c_float, C.c_int, C.c_int)
    return (len(segments) if n_seg is None else n_seg, *[(t * n)(*col) for t, col in zip(types, cols)])


def _adam_call(p, g, m, v, segments, betas, eps, step, grad_scale, extra=None, extra_n=None, offsets=(0, 0, 0, 0), n_seg=None,
               expect=0, null_extra=False):
    """sgr_adam_step (extra_n None) or sgr_adam_step_ex on guarded copies -> (p', m', v') after the assertions every call must hold;
    expect = INVALID: the call is refused and nothing at all is written"""
    lib = _lib()
    n = len(p)
    ops = dict(p=_Guarded(p, offsets[0]), g=_Guarded(g, offsets[1]), m=_Guarded(m, offsets[2]), v=_Guarded(v, offsets[3]))
    n_seg, *seg = _seg_arrays(segments, n_seg)
    head = (n, ops["p"].ptr, ops["g"].ptr, ops["m"].ptr, ops["v"].ptr, n_seg, *seg, betas[0], betas[1], eps, step, grad_scale)
    if extra_n is None:
        rc = lib.sgr_adam_step(*head, _stream())
    else:
        ops["extra"] = _Guarded(extra if extra is not None else np.zeros(0, F))
        rc = lib.sgr_adam_step_ex(*head, None if null_extra else ops["extra"].ptr, extra_n, _stream())
    assert rc == expect, (rc, expect)
    _after(ops, read_only=("g", "extra") if "extra" in ops else ("g",))
    if expect != 0:
        assert ops["p"].unchanged() and ops["m"].unchanged() and ops["v"].unchanged(), "a refused call wrote"
    return ops["p"].get(), ops["m"].get(), ops["v"].get()


def _adam_run_uncached(name, state=None, step=None):
    c, i = oc.ADAM[name], oc.adam_inputs(name)
    p, m, v = state if state is not None else (i["p"], i["m"], i["v"])
    return _adam_call(p, i["g"], m, v, i["segments"], c.betas, c.eps, c.step if step is None else step, c.grad_scale, i["extra"], c.extra_n)


@functools.lru_cache(maxsize=None)
def _adam_run(name):
    return _adam_run_uncached(name)


def _delta64(name, lr, lo):
    """the float64 update of the elements from `lo` on under the learning rates `lr`, in chunks"""
    c, i = oc.ADAM[name], oc.adam_inputs(name)
    out = []
    for a in range(lo, c.n, oc.CHUNK):
        s = slice(a, min(a + oc.CHUNK, c.n))
        ex = None if i["extra"] is None else i["extra"][s]
        p1 = orf.adam_step(i["p"][s], i["g"][s], i["m"][s], i["v"][s], lr[s], extra=ex, **oc.adam_args(c))[0]
        out.append(i["p"][s].astype(np.float64) - p1)
    return np.concatenate(out)


ADAM_FINITE = [c.name for c in oc.ADAM_CASES if c.family != "overflow"]


@functools.lru_cache(maxsize=None)
def _adam_kernel_err(name):
    return oc.adam_err(name, _adam_run(name))


@pytest.mark.parametrize("name", ADAM_FINITE)
def test_adam_every_element(name):
    c, i = oc.ADAM[name], oc.adam_inputs(name)
    got = _adam_run(name)
    print(f"{name}: {c.path}")
    assert not any(np.isnan(a).any() for a in got), "NaN out of a finite case"
    errs, bars = (_adam_kernel_err(name) if c.n <= oc.CHUNK else oc.adam_err(name, got)), oc.adam_bar(name)
    for k in "pmvu":
        # (a case of fewer than 64 elements: its median is taken over the family at all sizes of the sweep, as its yardsticks' is.  Held
        # to the pooled yardsticks' median by themselves, the 3 elements of n3-sweep-p0 gave 1.707e-07 and the 4 of n4-sweep-p0
        # 1.240e-07 against 1.192e-07, with every element far inside the yardsticks' distribution: p99 1.5e-06)
        pool = np.concatenate([_adam_kernel_err(nm)[k] for nm in oc.sweep_names(name)]) if bars[k].pooled else None
        oc.check(f"{name} {k}'", errs[k], bars[k], pool=pool)
    still = i["lr"] == 0
    assert same(got[0][still], i["p"][still]), "p moved where the learning rate is 0"
    if c.table in ("none", "layout"):
        assert still.any() and (i["p"][still] != 0).any() == (c.family == "normal")
    if c.family == "zero":   # 0 / eps: exactly 0, not NaN
        assert same(got[0], i["p"]) and not got[1].any() and not got[2].any()
    if c.grad_scale == 0:    # m and v only decay
        assert same(got[1], F(c.betas[0]) * i["m"]) and same(got[2], F(c.betas[1]) * i["v"])
    other = oc.other_lr(c.n, i["segments"])
    lr = i["lr"]
    if c.family == "p0" and (other != lr).any():
        # which learning rate an element takes is a decision, not a rounding: with p = 0, p' = -delta, and no element's update may be
        # nearer the one its segment's other learning rate would have made
        lo = int(np.flatnonzero(other != lr)[0])   # (of the big case: the periodic segment lies in the second turn)
        own, alt = _delta64(name, lr, lo), _delta64(name, other, lo)
        sel = (other != lr)[lo:] & (own != 0)
        d = -got[0][lo:].astype(np.float64)
        wrong = sel & ~(np.abs(d - own) < np.abs(d - alt))
        print(f"{name}: {int(sel.sum())} elements of periodic segments, {int(wrong.sum())} nearer the other learning rate")
        assert sel.any() and not wrong.any(), ("elements that took the other learning rate", lo + np.flatnonzero(wrong)[:16])


def test_adam_overflow_family():
    """|g| = 1e20 and 1e21: only the finite / non-finite pattern and the finite values are compared, against yardstick (a).  The
    finite values to 4 roundings of their magnitude (a contracted multiply-add is one; the floor of the bars)"""
    name = "n1027-periodic48-overflow"
    c, i = oc.ADAM[name], oc.adam_inputs(name)
    got = _adam_run(name)
    ya, _ = oc.adam_yardsticks(name)
    p1, m1, v1, mags = orf.adam_step(i["p"], i["g"], i["m"], i["v"], i["lr"], **oc.adam_args(c))
    for k, g, y in zip("pmv", got, ya):
        assert np.array_equal(np.isfinite(g), np.isfinite(y)) and np.array_equal(np.isnan(g), np.isnan(y)), k
        fin = np.isfinite(y)
        assert np.array_equal(g[~fin], y[~fin])   # inf is inf, of the same sign
        err = np.abs(g[fin].astype(np.float64) - y[fin]) / mags[k][fin]
        print(oc.describe(f"{name} {k}' against yardstick (a), finite elements", err))
        assert err.max() <= 4 * ULP, (k, err.max())
    assert np.isinf(got[2][1::2]).all() and np.isfinite(got[2][0::2]).all() and same(got[0][1::2], i["p"][1::2])


def test_adam_three_chained_steps():
    """Steps 3, 4, 5 on one gradient.  Per step from the device's own state: the restatement and both yardsticks start from the
    device's p, m, v after the step before, so errors do not compound.  End to end: the device's p after the three steps against the
    float64 chain, on the scale |p0| + sum |delta_k|, within 4 x (worst) and 2 x (median) of torch.optim.Adam's float32 chain"""
    name = "periodic48-p0"
    c, i = oc.ADAM[name], oc.adam_inputs(name)
    state = (i["p"], i["m"], i["v"])
    s64, sb = tuple(a.astype(np.float64) for a in state), state
    scale = np.abs(s64[0])
    for step in (3, 4, 5):
        got = _adam_run_uncached(name, state, step)
        errs, bars = oc.adam_err(name, got, state, step), oc.adam_bar_from(name, state, step)
        for k in "pmvu":
            oc.check(f"{name} step {step} {k}'", errs[k], bars[k])
        state = got
        *s64, mags = orf.adam_step(s64[0], i["g"], s64[1], s64[2], i["lr"], **oc.adam_args(c, step))
        scale = scale + mags["delta"]
        sb = orf.adam_step_torch(sb[0], i["g"], sb[1], sb[2], i["lr"], **oc.adam_args(c, step))
    err, err_b = oc.element_err(state[0], s64[0], scale), oc.element_err(sb[0], s64[0], scale)
    bar = oc.Bar(4 * max(err_b.max(), ULP), 2 * max(np.median(err_b), ULP), [oc.describe(f"{name} three steps p yardstick (b)", err_b)], False)
    oc.check(f"{name} three steps p", err, bar)


@pytest.mark.parametrize("name", ["layout-normal", "eight-p0", "n7-sweep-normal", "extra201-p0"])
def test_adam_two_runs_give_identical_bits(name):
    a, b = _adam_run(name), _adam_run_uncached(name)
    assert all(same(x, y) for x, y in zip(a, b))


def test_adam_rejected_arguments_write_nothing():
    i = oc.adam_inputs("bounds-normal")
    n = oc.N_TABLE
    ok = dict(segments=i["segments"], betas=(0.9, 0.999), eps=1e-15, step=3, grad_scale=1.0)
    args = (i["p"], i["g"], i["m"], i["v"])
    nine = [(k * 100, k * 100 + 100, 1e-3, 1e-3, 1, 1) for k in range(9)]
    _adam_call(*args, **dict(ok, segments=nine), expect=INVALID)
    _adam_call(*args, **dict(ok, step=0), expect=INVALID)
    extra = np.ones(n + 1, F)
    _adam_call(*args, **ok, extra=extra, extra_n=n + 1, expect=INVALID)
    _adam_call(*args, **ok, extra=extra, extra_n=5, null_extra=True, expect=INVALID)
    for k in range(4):   # each of the four pointers one float off 16-byte alignment
        _adam_call(*args, **ok, offsets=tuple(4 * (j == k) for j in range(4)), expect=INVALID)
    _adam_call(*args, **ok, offsets=(16, 32, 48, 240))   # (16-byte alignment is all it asks for)


# ---- k_adam_multi --------------------------------------------------------------------------------------------------------------
def _multi_call(tensors, expect=0):
    lib = _lib()
    nt = len(tensors)
    ops = {f"{k}{t}": _Guarded(ten[k]) for t, ten in enumerate(tensors) for k in "pgmv"}
    ptrs = lambda k: (C.c_void_p * nt)(*[ops[f"{k}{t}"].address for t in range(nt)])
    floats = lambda k: (C.c_float * nt)(*[ten[k] for ten in tensors])
    rc = lib.sgr_adam_step_multi(nt, (C.c_longlong * nt)(*[len(ten["p"]) for ten in tensors]), ptrs("p"), ptrs("g"), ptrs("m"), ptrs("v"),
                                 floats("lr"), floats("beta1"), floats("beta2"), floats("eps"), (C.c_int * nt)(*[ten["step"] for ten in tensors]),
                                 _stream())
    assert rc == expect, rc
    _after(ops, read_only=[f"g{t}" for t in range(nt)])
    if expect != 0:
        assert all(ops[f"{k}{t}"].unchanged() for t in range(nt) for k in "pmv"), "a refused call wrote"
    return [tuple(ops[f"{k}{t}"].get() for k in "pmv") for t in range(nt)]


@pytest.mark.parametrize("name", list(oc.MULTI_CASES))
def test_adam_multi_is_one_adam_step_per_tensor_bit_for_bit(name):
    """sugar_raster.h's claim: sgr_adam_step_multi is bit-identical to one sgr_adam_step per tensor with a single segment of that
    tensor's learning rate, m and v included.  The per-tensor results up to 14997 elements are held to the bars as well"""
    tensors = oc.multi_inputs(name)
    print(f"multi-{name}: {oc.MULTI_CASES[name][1]}")
    multi = _multi_call(tensors)
    for t, ten in enumerate(tensors):
        n = len(ten["p"])
        if n == 0:
            continue
        single = _adam_call(ten["p"], ten["g"], ten["m"], ten["v"], [(0, n, ten["lr"], ten["lr"], 1, 1)], (ten["beta1"], ten["beta2"]),
                            ten["eps"], ten["step"], 1.0)
        for k, a, b in zip("pmv", multi[t], single):
            assert not np.isnan(a).any()
            assert same(a, b), (name, t, n, k, np.flatnonzero(bits(a) != bits(b))[:8])
        if n <= 14997:
            lr = np.full(n, ten["lr"], F)
            kw = dict(beta1=ten["beta1"], beta2=ten["beta2"], eps=ten["eps"], step=ten["step"])
            p1, m1, v1, mags = orf.adam_step(ten["p"], ten["g"], ten["m"], ten["v"], lr, **kw)
            ya, yb = (f(ten["p"], ten["g"], ten["m"], ten["v"], lr, **kw) for f in (orf.adam_step_f32, orf.adam_step_torch))
            if n >= oc.MIN_ELEMENTS:
                for j, (k, ref) in enumerate(zip("pmv", (p1, m1, v1))):
                    oc.check(f"multi-{name} tensor {t} {k}'", oc.element_err(multi[t][j], ref, mags[k]),
                             oc.bar_from(f"multi-{name} tensor {t} {k}'", ref, mags[k], ya[j], yb[j]))


def test_adam_multi_rejects_nine_tensors():
    one = oc.multi_inputs("one")[0]
    _multi_call([one] * 9, expect=INVALID)


# ---- k_sh_grad_from_views, k_sh_adam_from_views --------------------------------------------------------------------------------
def _sh_operands(name):
    """guarded operands of a case; the gathered colour gradients in their [V][view_stride][3] layout, the padding rows left NaN"""
    c, i = oc.SH[name], oc.sh_inputs(name)
    stride = oc.sh_view_stride(c) or c.P
    dcolor = np.full(((c.V - 1) * stride + c.P, 3), np.nan, F)
    dcolor.view(np.uint32)[:] = 0xFFFFFFFF
    for v in range(c.V):
        dcolor[v * stride: v * stride + c.P] = i["dcolor"][v]
    ops = dict(means=_Guarded(i["means"]), campos=_Guarded(i["campos"]), dcolor=_Guarded(dcolor))
    head = (c.P, c.V, c.D, c.M, ops["means"].ptr, ops["campos"].ptr, ops["dcolor"].ptr, oc.sh_view_stride(c))
    return c, i, ops, head


RO = ("means", "campos", "dcolor")


@functools.lru_cache(maxsize=None)
def _sh_grad_run(name):
    c, i, ops, head = _sh_operands(name)
    ops["dL_dsh"] = _Guarded(nbytes=4 * c.P * c.M * 3, offset=c.offset)
    assert _lib().sgr_sh_grad_from_views(*head, ops["dL_dsh"].ptr, _stream()) == 0
    _after(ops, RO)
    return ops["dL_dsh"].get((c.P, c.M, 3))


def _sh_adam_run(name, direction=False, expect=0, offset=None, state=None):
    c, i, ops, head = _sh_operands(name)
    off = c.offset if offset is None else offset
    sh, m, v = state if state is not None else (i["sh"], i["m"], i["v"])
    ops.update(sh=_Guarded(sh, off), m=_Guarded(m, off), v=_Guarded(v, off))
    a = oc.SH_ARGS
    tail = (ops["sh"].ptr, ops["m"].ptr, ops["v"].ptr, c.lr_dc, c.lr_rest, a["beta1"], a["beta2"], a["eps"], a["step"], a["grad_scale"])
    if direction:
        ops["dmean"] = _Guarded(nbytes=4 * c.P * 3)
        rc = _lib().sgr_sh_adam_from_views_ex(*head, *tail, ops["dmean"].ptr, _stream())
    else:
        rc = _lib().sgr_sh_adam_from_views(*head, *tail, _stream())
    assert rc == expect, rc
    _after(ops, RO)
    if expect != 0:
        assert ops["sh"].unchanged() and ops["m"].unchanged() and ops["v"].unchanged(), "a refused call wrote"
        assert not direction or (ops["dmean"].buf == PATTERN).all()
    return (ops["sh"].get(), ops["m"].get(), ops["v"].get()) + ((ops["dmean"].get((c.P, 3)),) if direction else ())


def _check_sh_adam(name, got, what):
    ref, bars = oc.sh_reference(name), oc.sh_bars(name)
    assert not any(np.isnan(a).any() for a in got[:3])
    for j, k in enumerate("pmv"):
        oc.check(f"{name} {what} {k}'", oc.element_err(got[j], ref["adam"][j], ref["adam"][3][k]), bars[k])


@pytest.mark.parametrize("name", [c.name for c in oc.SH_CASES])
def test_sh_gradient_and_its_adam_every_element(name):
    c, i = oc.SH[name], oc.sh_inputs(name)
    ref, bars = oc.sh_reference(name), oc.sh_bars(name)
    print(f"{name}: {c.path}")
    grad = _sh_grad_run(name)
    assert not np.isnan(grad).any()
    oc.check(f"{name} dL_dsh", oc.element_err(grad, ref["grad"], ref["grad_mag"]), bars["grad"])
    assert not grad[:, (c.D + 1) ** 2:].any()   # above the degree: exactly 0
    got = _sh_adam_run(name)
    _check_sh_adam(name, got, "fused")
    if c.lr_dc == 0 and c.lr_rest == 0:
        assert same(got[0], i["sh"]) and not same(got[1], i["m"])
    if c.M > (c.D + 1) ** 2:   # gradient exactly 0: m and v decay, and the parameter still moves by its decaying m
        hi = slice((c.D + 1) ** 2, None)
        assert same(got[1][:, hi], F(0.9) * i["m"][:, hi]) and same(got[2][:, hi], F(0.999) * i["v"][:, hi])
        assert (got[0][:, hi] != i["sh"][:, hi]).mean() > 0.9
    if c.M == 16 and c.offset == 0:
        with_dir = _sh_adam_run(name, direction=True)
        assert all(same(a, b) for a, b in zip(with_dir[:3], got)), "sh, m, v differ between the DIR and the plain kernel"
        d64 = orf.sh_direction_term(i["means"], i["campos"], i["dcolor"], c.D, i["sh"])
        d32 = orf.sh_direction_term(i["means"], i["campos"], i["dcolor"], c.D, i["sh"], dtype=torch.float32)
        assert not np.isnan(with_dir[3]).any()
        err, yard = oc.row_err(with_dir[3], d64), oc.row_err(d32, d64)
        # (rows of P = 1 have no distribution: the floor of 4 roundings of the row's largest value would not be a bar for a sum of 48
        # products per view that cancel in the projection; the family's rows at P = 130 stand in)
        if c.P < oc.MIN_ELEMENTS:
            j = oc.sh_inputs(f"P130-D{c.D}M{c.M}")
            yard = oc.row_err(orf.sh_direction_term(j["means"], j["campos"], j["dcolor"], c.D, j["sh"], dtype=torch.float32),
                              orf.sh_direction_term(j["means"], j["campos"], j["dcolor"], c.D, j["sh"]))
        if len(yard):
            bar = oc.Bar(4 * max(yard.max(), ULP), 2 * max(np.median(yard), ULP),
                         [oc.describe(f"{name} dmean_extra yardstick (float32 autograd)", yard)], c.P < oc.MIN_ELEMENTS)
            oc.check(f"{name} dmean_extra", err, bar)


@pytest.mark.parametrize("name", ["P65-D3M16", "P130-D2M16", "P130-some", "P1-D3M16"])
def test_sh_adam_fused_against_gradient_then_flat_adam(name):
    """sgr_sh_grad_from_views, then sgr_adam_step over the [P, 48] block with one periodic segment (48, 3): held to the same bars as
    the fused kernel (not bit for bit: sh_adam.hip is built without contraction, adam.hip with)"""
    c, i = oc.SH[name], oc.sh_inputs(name)
    a = oc.SH_ARGS
    grad = _sh_grad_run(name)
    n = c.P * 48
    got = _adam_call(i["sh"].reshape(-1), grad.reshape(-1), i["m"].reshape(-1), i["v"].reshape(-1), [(0, n, c.lr_dc, c.lr_rest, 48, 3)],
                     (a["beta1"], a["beta2"]), a["eps"], a["step"], a["grad_scale"])
    _check_sh_adam(name, tuple(x.reshape(c.P, 16, 3) for x in got), "gradient + flat Adam")


def test_sh_adam_two_runs_give_identical_bits():
    for name in ("P130-D3M16", "P65-misaligned"):
        assert all(same(a, b) for a, b in zip(_sh_adam_run(name), _sh_adam_run(name)))
        assert all(same(a, b) for a, b in zip(_sh_adam_run("P130-D3M16", True), _sh_adam_run("P130-D3M16", True)))


def test_sh_direction_needs_sixteen_aligned_coefficients():
    _sh_adam_run("P65-D2M9", direction=True, expect=INVALID)
    _sh_adam_run("P65-D3M16", direction=True, expect=INVALID, offset=4)


# ---- activations ---------------------------------------------------------------------------------------------------------------
def _act_run(P, family, offset=0, expect=0):
    i = oc.act_inputs(P, family)
    lib = _lib()
    ops = {k: _Guarded(i[k], offset if "rot" in k else 0) for k in oc.ACT_ORDER}
    outs = dict(scales=(P, 3), rotations=(P, 4), opacities=(P, 1), scaling=(P, 3), rotation=(P, 4), opacity=(P, 1))
    for k, shape in outs.items():
        ops["out_" + k] = _Guarded(nbytes=4 * int(np.prod(shape)))
    raw = [ops[k].ptr for k in oc.ACT_ORDER]
    rc = lib.sgr_activations_forward(P, *raw[:3], ops["out_scales"].ptr, ops["out_rotations"].ptr, ops["out_opacities"].ptr, _stream())
    assert rc == expect, rc
    rc = lib.sgr_activations_backward(P, *raw, ops["out_scaling"].ptr, ops["out_rotation"].ptr, ops["out_opacity"].ptr, _stream())
    assert rc == expect, rc
    _after(ops, oc.ACT_ORDER)
    if expect != 0:
        assert all((ops["out_" + k].buf == PATTERN).all() for k in outs), "a refused call wrote"
        return None
    fwd = {k: ops["out_" + k].get(outs[k]) for k in ("scales", "rotations", "opacities")}
    bwd = {k: ops["out_" + k].get(outs[k]) for k in ("scaling", "rotation", "opacity")}
    return fwd, bwd


@functools.lru_cache(maxsize=None)
def _act_kernel(P, family):
    return _act_run(P, family)


def _act_err(P, family, j, way, k):
    ref = oc.act_reference(P, family)
    return oc.finite_err(_act_kernel(P, family)[j][k], ref[way][k], ref[way + "_mag"][k], ref["b"][j][k])


@pytest.mark.parametrize("P,family", oc.ACT_CASES)
def test_activations_every_element(P, family):
    ref, bars = oc.act_reference(P, family), oc.act_bars(P, family)
    print(f"{P}-{family}: {oc.ACT_FAMILIES[family]}")
    got = _act_kernel(P, family)
    for j, way in enumerate(("fwd", "bwd")):
        for k, g in got[j].items():
            yb = ref["b"][j][k]
            if family != "saturating":
                assert np.isfinite(g).all(), (way, k)
            # the finite / non-finite pattern is yardstick (b)'s; the finite values are compared
            assert np.array_equal(np.isfinite(g), np.isfinite(yb)) and np.array_equal(np.isnan(g), np.isnan(yb)), (way, k)
            assert np.array_equal(g[np.isinf(g)], yb[np.isinf(g)]), (way, k)
            pool = np.concatenate([_act_err(s, family, j, way, k) for s in oc.ACT_SIZES]) if bars[way][k].pooled else None
            oc.check(f"{P}-{family} {way} {k}", _act_err(P, family, j, way, k), bars[way][k], pool=pool)
    if family == "edges":   # a zero quaternion: 0 forward, g / 1e-12 backward
        assert not got[0]["rotations"][1::4].any()
    again = _act_run(P, family)
    assert all(same(got[j][k], again[j][k]) for j in (0, 1) for k in got[j])


def test_activations_reject_an_unaligned_quaternion_pointer():
    _act_run(257, "typical", offset=4, expect=INVALID)
