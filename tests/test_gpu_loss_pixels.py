"""GPU tests of the L1 + D-SSIM loss kernels (sugar_amd/csrc/loss.hip) pixel by pixel against the float64 reference
(oracle/loss_reference.py::l1_ssim_ref), over the case table of tests/loss_cases.py, through the C ABI (NULL pointers and offsets).

Every call goes through `_run`: the two images, the gradient, the scratch and the three loss values each lie inside a larger buffer
whose every byte is 0xFF before the calls -- four such bytes are a float NaN, so the scratch, `grad_img` and `loss_out` start as NaN and
so does everything around the operands.  Afterwards no output holds a NaN (every pixel of the maps was written before it was read,
nothing was read from beyond an image), every guard byte is unchanged (nothing was written outside an operand, and
sgr_l1_ssim_scratch_bytes was enough) and the images are as they were.

Tolerances are tied to the yardsticks, not to the kernel: err(pixel) = |got - ref64| / grad_mag over the pixels with grad_mag > 0
(grad_mag: the gradient's expression with every term replaced by its absolute value); where grad_mag == 0 the kernel's value must be
0.  Y = the larger of the two float32 CPU yardsticks (the reference's five-convolution formulation through autograd; the separable
pair formulation with true division) on the same case -- for a case with fewer than 64 such pixels, on the family at all shapes.  The
kernel's worst pixel must lie within 4 x Y's worst and its median within 2 x Y's median (FMA contraction, another order of the sums,
v_rcp_f32: two bits; the convention of tests/test_gpu_preprocess_bwd_rows.py).  All distributions are printed
(profiles/loss_pixels.txt holds a recorded run).  Only public outputs are read: the layout of the scratch is the kernels' own."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import loss_cases as lc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ULP = 2.0 ** -24
GUARD = 16384     # bytes before and after every operand
PATTERN = 0xFF
SHAPES = [s for s, _ in lc.SHAPES]
ids = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s)
bits = lambda a: np.ascontiguousarray(a).view(np.uint32)


class _Guarded:
    """`nbytes` starting `offset` bytes past a 256-byte boundary, GUARD bytes of PATTERN on either side (and PATTERN inside)"""

    def __init__(self, nbytes, offset=0):
        self.buf = torch.full((2 * GUARD + 256 + offset + nbytes,), PATTERN, dtype=torch.uint8, device=DEV)
        self.a = (-self.buf.data_ptr()) % 256 + GUARD + offset
        self.b = self.a + nbytes
        self.ptr = C.c_void_p(self.buf.data_ptr() + self.a)
        assert (self.buf.data_ptr() + self.a) % 256 == offset

    def floats(self, shape):
        return self.buf[self.a:self.b].view(torch.float32).view(shape)

    def intact(self):
        return bool((self.buf[:self.a] == PATTERN).all()) and bool((self.buf[self.b:] == PATTERN).all())


def _run(img, gt, lam, grad_loss=None, *, offset=0, from_backward=False):
    """forward + backward on CPU float32 images [C, H, W].  grad_loss: None = NULL, or the value of a device scalar.  offset: bytes
    past a 256-byte boundary at which img, gt and grad_img start.  from_backward: sgr_l1_ssim_forward(loss_out = NULL), then
    sgr_l1_ssim_backward_ex(loss_out).  -> dict(grad float32 [C, H, W], loss float32 [3]) after the assertions every case must hold"""
    from sugar_amd import _lib
    lib = _lib.load()
    Cn, H, W = img.shape
    n_bytes = 4 * img.numel()
    x, y, dx = _Guarded(n_bytes, offset), _Guarded(n_bytes, offset), _Guarded(n_bytes, offset)
    scratch, loss = _Guarded(lib.sgr_l1_ssim_scratch_bytes(Cn, W, H)), _Guarded(12)
    x.floats(img.shape).copy_(img)
    y.floats(img.shape).copy_(gt)
    assert torch.isnan(dx.floats(img.shape)).all() and torch.isnan(loss.floats((3,))).all() and torch.isnan(scratch.floats((-1,))).all()
    g = None if grad_loss is None else torch.tensor([grad_loss], dtype=torch.float32, device=DEV)
    gp = None if g is None else C.c_void_p(g.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    if from_backward:
        assert lib.sgr_l1_ssim_forward(Cn, W, H, x.ptr, y.ptr, lam, scratch.ptr, None, stream) == 0
        assert lib.sgr_l1_ssim_backward_ex(Cn, W, H, x.ptr, y.ptr, lam, scratch.ptr, gp, dx.ptr, loss.ptr, stream) == 0
    else:
        assert lib.sgr_l1_ssim_forward(Cn, W, H, x.ptr, y.ptr, lam, scratch.ptr, loss.ptr, stream) == 0
        assert lib.sgr_l1_ssim_backward(Cn, W, H, x.ptr, y.ptr, lam, scratch.ptr, gp, dx.ptr, stream) == 0
    torch.cuda.synchronize()
    out = dict(grad=dx.floats(img.shape).cpu().numpy(), loss=loss.floats((3,)).cpu().numpy())
    assert not np.isnan(out["grad"]).any(), ("NaN in the gradient at", np.argwhere(np.isnan(out["grad"]))[:8])
    assert not np.isnan(out["loss"]).any(), out["loss"]
    for name, buf in (("img", x), ("gt", y), ("grad_img", dx), ("scratch", scratch), ("loss_out", loss)):
        assert buf.intact(), f"bytes around {name} were written"
    assert torch.equal(x.floats(img.shape).cpu(), img) and torch.equal(y.floats(img.shape).cpu(), gt)
    if g is not None:
        assert float(g) == grad_loss
    return out


@functools.lru_cache(maxsize=None)
def _kernel(shape, family, lam, grad_loss=None):
    """one run of a case of the table, shared by the tests (nobody writes into it)"""
    img, gt = lc.images(shape, family)
    return _run(img, gt, lam, grad_loss)


def _check_pixels(got, shape, family, lam, g=1.0, what="kernel"):
    """the per-pixel bar of the module docstring"""
    ref = lc.reference(shape, family, lam, g)["ref"]
    err = lc.pixel_err(got, ref)
    y_max, y_med, ea, eb, pooled = lc.yardstick_bar(shape, family, lam, g)
    name = lc.label(shape, family, lam, g)
    where = " (the family at all shapes)" if pooled else ""
    print(lc.describe(f"{name} yardstick (a){where}", ea))
    print(lc.describe(f"{name} yardstick (b){where}", eb))
    print(lc.describe(f"{name} {what}", err))
    if not len(err):
        return
    if err.max() > 4 * y_max:
        live = np.argwhere(ref["grad_mag"] > 0)
        worst = [(tuple(int(v) for v in live[i]), float(err[i])) for i in np.argsort(err)[::-1][:8] if err[i] > 4 * y_max]
        raise AssertionError((name, "pixels over 4 x the yardsticks' worst", 4 * y_max, worst))
    assert np.median(err) <= 2 * y_med, (name, "median", float(np.median(err)), "yardsticks", y_med)


@pytest.mark.parametrize("family", lc.FAMILIES)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_every_pixel_against_the_float64_reference(shape, family):
    for lam in (0.2, 1.0):
        _check_pixels(_kernel(shape, family, lam)["grad"], shape, family, lam)


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_the_l1_half_is_exact(shape):
    """lambda = 0.  The gradient is bit for bit +-fl(g * fl(1 / N)) by the sign of x - y and 0 where x == y (g = 1 for NULL).

    loss[1], derived from the forward's summation and not measured: a pixel's |x - y| is one float32 rounding; a thread adds up to four
    of them (3 roundings: the first lands on 0), the wave's butterfly adds 6 more, the four waves' sums 3: 13 roundings on a pixel's way
    into its tile's partial, all terms non-negative, so the partial is within (1 + u)^13 - 1 of the exact sum, RELATIVELY.  The
    finishing sum and the division are made in double (2^-53 each: nothing), the result is rounded to float32 once: 14 roundings,
    u = 2^-24.  Bound: |loss[1] - mean64| <= mean64 * 14 u / (1 - 14 u), + 1e-12 for the double part."""
    N = shape[0] * shape[1] * shape[2]
    inv_n = np.float32(1.0 / N)
    for family in ("equal", "range"):
        img, gt = lc.images(shape, family)
        d = img.numpy().astype(np.float64) - gt.numpy().astype(np.float64)
        ref = lc.reference(shape, family, 0.0)["ref"]
        for g in lc.GRAD_LOSSES:
            out = _kernel(shape, family, 0.0, g)
            v = np.float32(1.0 if g is None else g) * inv_n
            want = np.where(d > 0, v, np.where(d < 0, -v, np.float32(0))).astype(np.float32)
            assert np.array_equal(out["grad"], want), (family, g)   # as values: a zero's sign is free
            assert np.array_equal(bits(out["grad"])[d != 0], bits(want)[d != 0]), (family, g)
            rel = abs(float(out["loss"][1]) - ref["l1_mean"]) / ref["l1_mean"]
            print(f"{lc.label(shape, family, 0.0)} g {g}: loss[1] {out['loss'][1]:.9g} float64 {ref['l1_mean']:.12g} rel {rel:.3e}")
            assert rel <= 14 * ULP / (1 - 14 * ULP) + 1e-12, (family, g, rel)
            assert bits(out["loss"])[0] == bits(out["loss"])[1]   # (1 - 0) * l1 + 0 * (1 - ssim), combined in double
        if family == "equal" and shape[2] > 1:
            assert (d[..., : shape[2] // 2] == 0).all() and not _kernel(shape, family, 0.0)["grad"][..., : shape[2] // 2].any()


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_loss_values(shape):
    """loss[0] and loss[2] against float64: within 4 x the largest error of the yardsticks over the family (all shapes, both lambdas)
    plus one float32 rounding of the output; loss[0] is consistent with loss[1] and loss[2] to two float32 roundings (the kernel
    combines the double means and rounds once; the two means it reports are rounded too).  At (1, 1, 1) loss[2] is one pixel's S."""
    for family in lc.FAMILIES:
        yard = lc.family_loss_err(family)
        for lam in (0.2, 1.0):
            ref = lc.reference(shape, family, lam)["ref"]
            out = _kernel(shape, family, lam)["loss"].astype(np.float64)
            name = lc.label(shape, family, lam)
            e0, e2 = abs(out[0] - ref["loss"]), abs(out[2] - ref["ssim_mean"])
            print(f"{name}: loss {out[0]:.9g} err {e0:.3e} (yardsticks, family: {yard['loss']:.3e})  "
                  f"ssim {out[2]:.9g} err {e2:.3e} (yardsticks, family: {yard['ssim_mean']:.3e})")
            assert e0 <= 4 * yard["loss"] + ULP * abs(ref["loss"]), (name, "loss", e0)
            assert e2 <= 4 * yard["ssim_mean"] + ULP * abs(ref["ssim_mean"]), (name, "ssim", e2)
            l = lc.f32(lam)
            combined = (1 - l) * out[1] + l * (1 - out[2])
            assert abs(out[0] - combined) <= ULP * ((1 - l) * abs(out[1]) + l * abs(out[2]) + abs(out[0])) * (1 + 1e-6), (name, out)


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_grad_loss(shape):
    """NULL and a device scalar 1.0 give identical bits; with -2.5 the per-pixel bar holds against the reference scaled by -2.5"""
    for family in ("noise", "flat"):
        null, one = _kernel(shape, family, 0.2), _kernel(shape, family, 0.2, 1.0)
        assert np.array_equal(bits(null["grad"]), bits(one["grad"])) and np.array_equal(bits(null["loss"]), bits(one["loss"]))
        scaled = _kernel(shape, family, 0.2, -2.5)
        assert np.array_equal(bits(null["loss"]), bits(scaled["loss"]))   # (the value does not depend on it)
        _check_pixels(scaled["grad"], shape, family, 0.2, -2.5)


def test_planes_do_not_depend_on_where_their_tiles_run():
    """An image whose C planes are copies of one plane: a plane's tiles land on other workgroups and XCD slots with every C, and
    nothing may depend on that.  Within an image the gradient planes are bit-identical; across C = 1, 3, 8 the means are the same sums
    of the same tile partials, added in double in another order and rounded once: equal to one float32 ulp"""
    img1, gt1 = lc.images((1, 57, 65), "noise")
    outs = {}
    for Cn in (1, 3, 8):
        img, gt = img1.repeat(Cn, 1, 1).contiguous(), gt1.repeat(Cn, 1, 1).contiguous()
        outs[Cn] = out = _run(img, gt, 0.2)
        for c in range(1, Cn):
            assert np.array_equal(bits(out["grad"][c]), bits(out["grad"][0])), (Cn, c)
    _check_pixels(outs[1]["grad"], (1, 57, 65), "noise", 0.2)
    one = outs[1]["grad"][0].astype(np.float64)
    for Cn in (3, 8):
        assert (np.abs(outs[Cn]["loss"] - outs[1]["loss"]) <= np.spacing(outs[1]["loss"])).all(), (outs[Cn]["loss"], outs[1]["loss"])
        # the gradient is fl(g * fl(1 / N)) times what the maps give, and the maps are the same bits: C times a plane of the C-plane
        # image is the one-plane image's gradient to the roundings of the two factors 1 / N and of the two products
        assert (np.abs(outs[Cn]["grad"][0].astype(np.float64) * Cn - one) <= 4 * ULP * np.abs(one)).all(), Cn


@pytest.mark.parametrize("shape,family", [((4, 57, 65), "noise"), ((3, 28, 96), "flat"), ((3, 5, 7), "range")], ids=ids)
def test_two_runs_give_identical_bits(shape, family):
    img, gt = lc.images(shape, family)
    a, b = _kernel(shape, family, 0.2), _run(img, gt, 0.2)
    assert np.array_equal(bits(a["grad"]), bits(b["grad"])) and np.array_equal(bits(a["loss"]), bits(b["loss"]))


@pytest.mark.parametrize("shape", [(3, 5, 7), (1, 7, 43), (4, 57, 65), (3, 65, 43)], ids=ids)
def test_unaligned_operands(shape):
    """img, gt and grad_img one float past a 256-byte boundary: every output bit-equal to the aligned run"""
    for family in ("noise", "impulse"):
        img, gt = lc.images(shape, family)
        a, b = _kernel(shape, family, 0.2), _run(img, gt, 0.2, offset=4)
        assert np.array_equal(bits(a["grad"]), bits(b["grad"])) and np.array_equal(bits(a["loss"]), bits(b["loss"])), family


@pytest.mark.parametrize("shape", [(4, 57, 65), (3, 28, 96), (1, 1, 1)], ids=ids)
def test_loss_value_out_of_the_backward_kernel_at_the_seam_shapes(shape):
    """sgr_l1_ssim_forward(loss_out = NULL) + sgr_l1_ssim_backward_ex(loss_out) where the forward's partial count and the backward's
    tile count differ (36 against 24 at (4, 57, 65)) and the eight leading workgroups shift every tile index: the value equals the
    stand-alone finishing kernel's and the gradient is the same array, bit for bit"""
    for family in ("noise", "flat"):
        img, gt = lc.images(shape, family)
        for g in (None, -2.5):
            a, b = _kernel(shape, family, 0.2, g), _run(img, gt, 0.2, g, from_backward=True)
            assert np.array_equal(bits(a["loss"]), bits(b["loss"])) and a["loss"][0] > 0, (family, g, a["loss"], b["loss"])
            assert np.array_equal(bits(a["grad"]), bits(b["grad"])), (family, g)


def test_the_train_steps_own_call_sequence():
    """NativeTrainer at 128 x 96: its forward carries the rasterizer's post-blend job in the first of eight leading workgroups (every
    tile index shifted), its backward reduces the value.  The step's image, target and lambda through the stand-alone forward + backward
    give the step's `_grad_image` and `loss_out` bit for bit"""
    from sugar_amd import synthetic as syn
    from sugar_amd.train_step import GaussianParams, NativeTrainer
    dev = torch.device(DEV)
    W, H = 128, 96
    scene = syn.make_scene(400, 9, 0.02, 0.15)
    cam = syn.orbit_cameras(W, H)[2]
    cam = cam._replace(viewmatrix=cam.viewmatrix.to(dev), projmatrix=cam.projmatrix.to(dev), campos=cam.campos.to(dev))
    gt = torch.rand(3, H, W, generator=torch.Generator().manual_seed(5))
    nt = NativeTrainer(GaussianParams(scene, dev), torch.zeros(3), W, H)
    gtd = gt.to(dev)
    for _ in range(2):
        nt.step(cam, gtd, cam_key=0)
        nt.synchronize()
    image = nt.image.cpu()
    assert nt.last_num_rendered > 0 and float(image.std()) > 1e-3
    out = _run(image, gt, nt._lambda_dssim)
    assert np.array_equal(bits(out["loss"]), bits(nt.loss_out.cpu().numpy())), (out["loss"], nt.loss_out)
    assert np.array_equal(bits(out["grad"]), bits(nt._grad_image.cpu().numpy()))
    assert (3, H, W) in SHAPES   # (where the stand-alone calls are held to the float64 reference)


@pytest.mark.parametrize("batched", (False, True))
def test_the_drop_in_ssim(batched):
    """fused_loss.make_ssim (lambda = 1 inside) as [3, 29, 33] and [1, 3, 29, 33] with an incoming factor of 2.5: the per-pixel bar
    against -grad_ssim * d(1 - ssim)/dx, the value against the float64 mean"""
    from sugar_amd import fused_loss

    def original(*a, **k):
        raise AssertionError("the call shape is one the kernels cover")
    ssim = fused_loss.make_ssim(original)
    shape = (3, 29, 33)
    for family in ("noise", "flat", "impulse"):
        img, gt = lc.images(shape, family)
        a, b = img.to(DEV), gt.to(DEV)
        if batched:
            a, b = a[None], b[None]
        a.requires_grad_(True)
        value = ssim(a, b)
        (2.5 * value).backward()
        assert a.grad.shape == a.shape
        _check_pixels(a.grad.cpu().numpy().reshape(shape), shape, family, 1.0, -2.5, what="drop-in ssim")
        want = lc.reference(shape, family, 1.0)["ref"]["ssim_mean"]
        assert abs(float(value) - want) <= 4 * lc.family_loss_err(family)["ssim_mean"] + ULP * abs(want), (family, float(value), want)
