"""GPU tests of the refine stage's mesh binding and normal-consistency kernels (csrc/mesh_bind.hip, sugar_amd/mesh_bind.py).

The accuracy bar, everywhere below: a tensor x of the HIP path is compared with a float64 evaluation x64 of the same quantity and with
the float32 evaluation x32 of the reference arithmetic (the fixture's record of the reference class on the CPU, or the torch path on the
same device):

    |x - x64|  <=  2 |x32 - x64|  +  ulp32(max |x64|)            (Euclidean norms over the whole tensor; no element is left out)

Two correctly rounded float32 evaluations in different operation orders can each sit as far from the exact value as the other; a kernel
less accurate than the reference's own arithmetic fails.  `scaling` is held to `torch.exp` on the device WITHIN 1 ULP (the kernel calls
the device libm's expf, as torch does; the test prints how many elements differ at all).  Every test prints the errors it measured.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sugar_binding.npz")
DEV = "cuda"


@pytest.fixture(scope="module")
def fx():
    return np.load(GOLDEN)


@pytest.fixture(scope="module", autouse=True)
def _standins(hip_lib):
    from sugar_amd import shims
    shims.install()


def _norm(a):
    return float(np.linalg.norm(np.asarray(a, dtype=np.float64).ravel()))


def check(name, x, x32, x64):
    """the 2x rule; returns the measured relative errors (hip, reference f32)"""
    x, x32, x64 = (np.asarray(t.detach().cpu().numpy() if torch.is_tensor(t) else t, dtype=np.float64) for t in (x, x32, x64))
    assert x.shape == x64.shape == x32.shape, (name, x.shape, x32.shape, x64.shape)
    assert np.isfinite(x).all(), f"{name}: non-finite values"
    scale = max(_norm(x64), 1e-300)
    e_hip, e_ref = _norm(x - x64), _norm(x32 - x64)
    floor = float(np.spacing(np.float32(np.abs(x64).max())))
    print(f"  {name:34s} hip {e_hip / scale:.3e}   reference f32 {e_ref / scale:.3e}   (floor {floor / scale:.1e})")
    assert e_hip <= 2.0 * e_ref + floor, f"{name}: |hip - f64| = {e_hip:.4e} > 2 x {e_ref:.4e} + {floor:.1e}"
    return e_hip / scale, e_ref / scale


# ------------------------------------------------------------------------------------------------------------ the torch path
def torch_binding(verts, faces, bary, scales, cplx, thickness, n):
    """SuGaR.points / .scaling / .quaternions of a bound model (sugar_model.py:383-479, `not editable`) in plain torch, any dtype and
    device, over the stand-in Meshes / matrix_to_quaternion -- what the HIP path replaces"""
    from pytorch3d.structures import Meshes
    from pytorch3d.transforms import matrix_to_quaternion
    N = torch.nn.functional.normalize
    F_ = faces.shape[0]
    fv = verts[faces]
    points = (fv[:, None] * bary.reshape(n, 3, 1)[None]).sum(dim=-2).reshape(F_ * n, 3)
    scaling = torch.cat([thickness * torch.ones(len(scales), 1, device=scales.device, dtype=scales.dtype), torch.exp(scales)], dim=-1)
    R_0 = N(Meshes(verts=[verts], faces=[faces]).faces_normals_list()[0], dim=-1)
    base_R_1 = N(fv[:, 0] - fv[:, 1], dim=-1)
    base_R_2 = N(torch.cross(R_0, base_R_1, dim=-1))
    c = N(cplx, dim=-1).view(F_, n, 2)
    R_1 = c[..., 0:1] * base_R_1[:, None] + c[..., 1:2] * base_R_2[:, None]
    R_2 = -c[..., 1:2] * base_R_1[:, None] + c[..., 0:1] * base_R_2[:, None]
    R = torch.cat([R_0[:, None, ..., None].expand(-1, n, -1, -1).clone(), R_1[..., None], R_2[..., None]], dim=-1).view(-1, 3, 3)
    return points, scaling, N(matrix_to_quaternion(R), dim=-1)


def hip_binding(verts, faces, bary, scales, cplx, thickness, n):
    from sugar_amd import mesh_bind
    return (mesh_bind.bound_points(verts, faces, bary), mesh_bind.bound_scaling(scales, thickness),
            mesh_bind.bound_quaternions(verts, faces, cplx, n))


def leaves(verts, scales, cplx, dtype=torch.float32):
    return tuple(t.detach().to(dtype).clone().requires_grad_(True) for t in (verts, scales, cplx))


def run_path(fn, verts, faces, bary, scales, cplx, thickness, n, cots, dtype):
    """outputs and the gradients of sum_props (prop * cot) on (verts, scales, cplx)"""
    v, s, z = leaves(verts, scales, cplx, dtype)
    outs = fn(v, faces, bary.to(dtype), s, z, thickness.to(dtype), n)
    loss = sum((o * c.to(dtype)).sum() for o, c in zip(outs, cots))
    loss.backward()
    return [o.detach() for o in outs], [v.grad, s.grad, z.grad]


def ulps_apart(a, b):
    ia, ib = a.contiguous().view(torch.int32).to(torch.int64), b.contiguous().view(torch.int32).to(torch.int64)
    return (ia - ib).abs()


# ------------------------------------------------------------------------------------------------------------ fixture replay
@pytest.mark.parametrize("n", [1, 3, 4, 6])
def test_fixture_replay(fx, n):
    """the reference class's own record (tests/golden/make_sugar_binding.py): every output and every gradient, one backward per property
    and one for the sum of the three"""
    from sugar_amd import mesh_bind
    t = lambda k: torch.as_tensor(fx[f"n{n}_{k}"]).to(DEV)
    faces, bary, thickness = t("faces"), t("bary"), t("thickness")
    cots = {p: t("cot_" + p) for p in ("points", "scaling", "quaternions")}
    r = lambda k: (fx[f"n{n}_{k}"], fx[f"n{n}_{k}_f64"])
    print(f"\nfixture replay, n = {n}:")
    # one backward per property
    v, s, z = leaves(t("_points"), t("_scales"), t("_quaternions"))
    p = mesh_bind.bound_points(v, faces, bary)
    (p * cots["points"]).sum().backward()
    check("points", p, *r("out_points"))
    check("points: d _points", v.grad, *r("grad_points_points"))
    v.grad = None
    sc = mesh_bind.bound_scaling(s, thickness)
    (sc * cots["scaling"]).sum().backward()
    check("scaling", sc, *r("out_scaling"))
    check("scaling: d _scales", s.grad, *r("grad_scaling_scales"))
    want = torch.cat([thickness * torch.ones(len(s), 1, device=DEV), torch.exp(s.detach())], dim=-1)
    apart = ulps_apart(sc.detach(), want)
    print(f"  scaling vs torch.exp on the device: {int((apart > 0).sum())} of {apart.numel()} elements differ, at most {int(apart.max())} ulp")
    assert int(apart.max()) <= 1
    s.grad = None
    q = mesh_bind.bound_quaternions(v, faces, z, n)
    (q * cots["quaternions"]).sum().backward()
    check("quaternions", q, *r("out_quaternions"))
    check("quaternions: d _points", v.grad, *r("grad_quaternions_points"))
    check("quaternions: d _quaternions", z.grad, *r("grad_quaternions_quaternions"))
    # the sum of the three
    _, grads = run_path(hip_binding, t("_points"), faces, bary, t("_scales"), t("_quaternions"), thickness, n,
                        [cots["points"], cots["scaling"], cots["quaternions"]], torch.float32)
    for g, name in zip(grads, ("_points", "_scales", "_quaternions")):
        check("all three: d " + name, g, *r("grad_all" + name))


def torch_normal_consistency(verts, faces):
    from pytorch3d.loss import mesh_normal_consistency
    from pytorch3d.structures import Meshes
    return mesh_normal_consistency(Meshes(verts=[verts], faces=[faces]))


@pytest.mark.parametrize("n", [1, 6])
def test_normal_consistency_fixture(fx, n):
    """against the fixture's float64 value and vertex gradient (the stand-in's definition); the float32 side of the bar is the stand-in's
    torch path on this device"""
    from sugar_amd import mesh_bind
    verts, faces = torch.as_tensor(fx[f"n{n}__points"]).to(DEV), torch.as_tensor(fx[f"n{n}_faces"]).to(DEV)
    v = verts.clone().requires_grad_(True)
    loss = mesh_bind.normal_consistency(v, faces)
    assert loss.dim() == 0
    (loss * 3.0).backward()
    v32 = verts.clone().requires_grad_(True)
    l32 = torch_normal_consistency(v32, faces)
    (l32 * 3.0).backward()
    print(f"\nnormal consistency on the fixture mesh (n = {n}):")
    check("value", loss.reshape(1), l32.reshape(1), fx[f"n{n}_nc_value_f64"])
    check("d verts", v.grad, v32.grad, 3.0 * fx[f"n{n}_nc_grad_f64"])


def test_normal_consistency_closed_forms():
    """the closed forms of tests/test_shims.py through the HIP path: a cube (12 of its 18 edges are right angles), a flat sheet, a bent
    one; and the switch of the stand-in `pytorch3d.loss.mesh_normal_consistency`"""
    from sugar_amd import mesh_bind
    import pytorch3d.loss as p3d_loss
    from pytorch3d.structures import Meshes
    v = torch.tensor([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]], dtype=torch.float32,
                     device=DEV, requires_grad=True)
    f = torch.tensor([[0, 2, 1], [0, 3, 2], [4, 5, 6], [4, 6, 7], [0, 1, 5], [0, 5, 4], [1, 2, 6], [1, 6, 5], [2, 3, 7], [2, 7, 6],
                      [3, 0, 4], [3, 4, 7]], device=DEV)
    nc = mesh_bind.normal_consistency(v, f)
    assert abs(float(nc) - 12 / 18) < 1e-6
    nc.backward()
    assert torch.isfinite(v.grad).all() and float(v.grad.abs().sum()) > 0
    ys, xs = torch.meshgrid(torch.arange(5.0), torch.arange(5.0), indexing="ij")
    gv = torch.stack([xs.reshape(-1), ys.reshape(-1), torch.zeros(25)], dim=1).to(DEV)
    gf = []
    for y in range(4):
        for x in range(4):
            a = y * 5 + x
            gf += [[a, a + 1, a + 6], [a, a + 6, a + 5]]
    gf = torch.tensor(gf, device=DEV)
    assert float(mesh_bind.normal_consistency(gv, gf)) < 1e-6
    bent = gv.clone()
    bent[:, 2] = 0.3 * (bent[:, 0] - 2.0) ** 2
    got = float(mesh_bind.normal_consistency(bent, gf))
    assert got > 1e-3 and abs(got - float(torch_normal_consistency(bent, gf))) < 1e-6
    # the stand-in's switch: off by default, routes a single ROCm mesh when set
    if hasattr(p3d_loss, "USE_HIP_NORMAL_CONSISTENCY"):
        assert p3d_loss.USE_HIP_NORMAL_CONSISTENCY is False
        calls = []
        real = mesh_bind.normal_consistency
        mesh_bind.normal_consistency = lambda *a: calls.append(1) or real(*a)
        try:
            p3d_loss.USE_HIP_NORMAL_CONSISTENCY = True
            routed = p3d_loss.mesh_normal_consistency(Meshes([bent], [gf]))
            p3d_loss.USE_HIP_NORMAL_CONSISTENCY = False
            plain = p3d_loss.mesh_normal_consistency(Meshes([bent], [gf]))
        finally:
            p3d_loss.USE_HIP_NORMAL_CONSISTENCY = False
            mesh_bind.normal_consistency = real
        assert calls == [1] and abs(float(routed) - float(plain)) < 1e-6


# ------------------------------------------------------------------------------------------------------------ trainer scale
@pytest.mark.parametrize("n", [1, 6])
def test_trainer_scale(n):
    """make_bound_scene(1M): forward and backward of the three properties and of the normal consistency against a float64 evaluation
    by the torch path on the same device; every element compared.  The backward is run twice: bit-identical vertex gradients."""
    from sugar_amd import mesh_bind, synthetic as syn
    bs = syn.make_bound_scene(1_000_000, 5, n_per_triangle=n)
    verts, faces = bs.verts.to(DEV), bs.faces.to(DEV)
    scales, cplx = torch.log(bs.plane_scales).to(DEV), bs.complex_rot.to(DEV)
    g = torch.Generator().manual_seed(17)
    cplx = cplx * (0.5 + torch.rand(cplx.shape[0], 1, generator=g).to(DEV))      # not pre-normalised, as in training
    bary = torch.tensor(syn._BARY[n][0], dtype=torch.float32).reshape(n, 3).to(DEV)
    thickness = torch.tensor([bs.thickness], dtype=torch.float32, device=DEV)
    P = faces.shape[0] * n
    cots = [torch.randn(P, k, generator=g).to(DEV) for k in (3, 3, 4)]
    args = (verts, faces, bary, scales, cplx, thickness, n, cots)
    o64, g64 = run_path(torch_binding, *args, torch.float64)
    o32, g32 = run_path(torch_binding, *args, torch.float32)
    oh, gh = run_path(hip_binding, *args, torch.float32)
    print(f"\ntrainer scale, n = {n}: {faces.shape[0]} faces, {verts.shape[0]} vertices, {P} Gaussians")
    for name, a, b, c in zip(("points", "scaling", "quaternions"), oh, o32, o64):
        check(name, a, b, c)
    for name, a, b, c in zip(("d _points", "d _scales", "d _quaternions"), gh, g32, g64):
        check(name, a, b, c)
    _, gh2 = run_path(hip_binding, *args, torch.float32)
    assert torch.equal(gh[0].view(torch.int32), gh2[0].view(torch.int32)), "the vertex gradient is not reproducible bit for bit"
    del o64, g64, o32, g32, oh, gh, gh2
    # the regulariser on the same mesh
    res = {}
    for key, fn, dt in (("f64", torch_normal_consistency, torch.float64), ("f32", torch_normal_consistency, torch.float32),
                        ("hip", mesh_bind.normal_consistency, torch.float32), ("hip2", mesh_bind.normal_consistency, torch.float32)):
        v = verts.to(dt).clone().requires_grad_(True)
        loss = fn(v, faces)
        (loss * 1000.0).backward()
        res[key] = (loss.detach().reshape(1), v.grad)
    check("normal consistency", res["hip"][0], res["f32"][0], res["f64"][0])
    check("normal consistency: d verts", res["hip"][1], res["f32"][1], res["f64"][1])
    assert torch.equal(res["hip"][1].view(torch.int32), res["hip2"][1].view(torch.int32))
    assert torch.equal(res["hip"][0], res["hip2"][0])


# ------------------------------------------------------------------------------------------------------------ degenerate input
EPS32 = float(np.finfo(np.float32).eps)


def close_to_f32(name, x, x32, ulps):
    """directly against the float32 torch path: |x - x32| <= ulps * eps32 * |x32| (Euclidean norms)"""
    x, x32 = x.detach().double().cpu().numpy(), x32.detach().double().cpu().numpy()
    d, scale = _norm(x - x32), _norm(x32)
    print(f"  {name:34s} |hip - torch f32| / |torch f32| = {d / max(scale, 1e-300):.3e}   (bound {ulps * EPS32:.1e})")
    assert d <= ulps * EPS32 * scale, f"{name}: {d:.4e} > {ulps} eps32 x {scale:.4e}"


def _degenerate_case(fx, bad_face=None, bad_z=None):
    n = 3
    t = lambda k: torch.as_tensor(fx[f"n{n}_{k}"]).to(DEV)
    faces, cplx = t("faces").clone(), t("_quaternions").clone()
    if bad_face is not None:
        faces[bad_face, 2] = faces[bad_face, 1]                # (i, j, j): e1 = e2, the cross product is exactly 0 in unfused arithmetic
    if bad_z is not None:
        cplx[bad_z] = 0.0
    cots = [t("cot_points"), t("cot_scaling"), t("cot_quaternions")]
    args = (t("_points"), faces, t("bary"), t("_scales"), cplx, t("thickness"), n, cots)
    runs = [run_path(torch_binding, *args, torch.float64), run_path(torch_binding, *args, torch.float32),
            run_path(hip_binding, *args, torch.float32)]
    for x in runs[2][0] + runs[2][1]:
        assert torch.isfinite(x).all()
    hit_face = bad_face if bad_face is not None else bad_z // n
    rows = torch.tensor([bad_face * n + k for k in range(n)] if bad_face is not None else [bad_z], device=DEV)
    touched = torch.unique(faces[hit_face])
    rest = torch.ones(cplx.shape[0], dtype=torch.bool, device=DEV)
    rest[rows] = False
    vrest = torch.ones(args[0].shape[0], dtype=torch.bool, device=DEV)
    vrest[touched] = False
    return runs, rows, touched, rest, vrest


def test_zero_complex_number(fx):
    """one zero complex number among valid ones: R = [R_0 | 0 | 0], two traces of matrix_to_quaternion tie exactly and the first wins in
    both paths; the gradient on that complex number is the cotangent divided by normalize's eps.  Finite everywhere; by the 2x rule against
    float64 on every element; and on the affected elements EQUAL to the float32 torch path: both evaluate the same float32 operations and
    differ only in the order of the three squares under a norm and in the last place of sqrt and division -- a chain of fewer than ten such
    roundings to an output, some thirty to a gradient -- so 8 eps32 (outputs) and 32 eps32 (gradients), norm-wise, bound their distance."""
    ((o64, g64), (o32, g32), (oh, gh)), rows, touched, rest, vrest = _degenerate_case(fx, bad_z=100)
    print("\nzero complex number:")
    check("quaternions (affected row)", oh[2][rows], o32[2][rows], o64[2][rows])
    check("quaternions (other rows)", oh[2][rest], o32[2][rest], o64[2][rest])
    check("d _quaternions (affected row)", gh[2][rows], g32[2][rows], g64[2][rows])
    check("d _quaternions (other rows)", gh[2][rest], g32[2][rest], g64[2][rest])
    check("d _points", gh[0], g32[0], g64[0])
    check("d _scales", gh[1], g32[1], g64[1])
    close_to_f32("quaternions (affected row)", oh[2][rows], o32[2][rows], 8)
    close_to_f32("d _quaternions (affected row)", gh[2][rows], g32[2][rows], 32)
    close_to_f32("d _points (the face's vertices)", gh[0][touched], g32[0][touched], 32)


def test_zero_area_face(fx):
    """one zero-area face (i, j, j) among valid ones: a finding must not become a fault -- every output and gradient is finite, every
    element NOT on that face meets the 2x rule, and the face's own elements meet the bar the other tests use against float64 and, directly,
    against the float32 torch path (distance to it within twice its own distance to float64, plus the floor).

    That last bar is loose on purpose, and the test prints why: the face's normal is 0 / max(0, 1e-6) normalised again with eps = 1e-12, so
    anything that makes e1 x e1 differ from an exact 0 is amplified by 1e18.  The kernel is built without contraction and gets an exact 0
    (R_0 = 0, as exact arithmetic does).  torch's float32 cross product on the device may contract a1 b2 - a2 b1 into a fused
    multiply-add, which leaves a rounding residue: its R_0 is then a unit vector made of noise, its quaternion and the 1e18-scale vertex
    gradient with it.  Measured on the MI355X (printed below): the float32 torch path is 0.3 (relative) from float64 on those rows, the
    kernel 3e-8."""
    ((o64, g64), (o32, g32), (oh, gh)), rows, touched, rest, vrest = _degenerate_case(fx, bad_face=7)
    print("\nzero-area face:")
    e = torch.as_tensor(fx["n3__points"]).to(DEV)
    e = e[1:] - e[:-1]
    print(f"  torch.cross(e, e) on the device, float32: max |.| = {float(torch.cross(e, e, dim=-1).abs().max()):.3e}"
          f" (0 means the cross product is not contracted)")
    check("points", oh[0], o32[0], o64[0])
    check("quaternions (other rows)", oh[2][rest], o32[2][rest], o64[2][rest])
    check("d _quaternions (other rows)", gh[2][rest], g32[2][rest], g64[2][rest])
    check("d _points (other vertices)", gh[0][vrest], g32[0][vrest], g64[0][vrest])
    check("d _scales", gh[1], g32[1], g64[1])
    check("quaternions (the face's rows)", oh[2][rows], o32[2][rows], o64[2][rows])
    check("d _quaternions (the face's rows)", gh[2][rows], g32[2][rows], g64[2][rows])
    check("d _points (the face's vertices)", gh[0][touched], g32[0][touched], g64[0][touched])
    for name, a, b, c in (("quaternions", oh[2][rows], o32[2][rows], o64[2][rows]), ("d _quaternions", gh[2][rows], g32[2][rows], g64[2][rows]),
                          ("d _points", gh[0][touched], g32[0][touched], g64[0][touched])):
        d_hip, d_ref = _norm((a - b).cpu().numpy()), _norm(b.double().cpu().numpy() - c.cpu().numpy())
        floor = float(np.spacing(np.float32(c.abs().max().item())))
        print(f"  {name + ' (the face) vs torch f32':34s} |hip - f32| / |f32| = {d_hip / max(_norm(b.cpu().numpy()), 1e-300):.3e}")
        assert d_hip <= 2.0 * d_ref + floor, name


# ------------------------------------------------------------------------------------------------------------ through the class
class BoundStandIn:
    """the attributes of a bound reference model that the patched properties read (the pattern of tests/sugar_standin.py), carrying the
    fixture's state; `points` / `scaling` / `quaternions` are the reference's definitions (sugar_model.py:383-479) in torch"""
    binded_to_surface_mesh = True
    editable = False

    def __init__(self, fx, n, dtype=torch.float32):
        t = lambda k: torch.as_tensor(fx[f"n{n}_{k}"]).to(DEV)
        self._points = t("_points").to(dtype).requires_grad_(True)
        self._scales = t("_scales").to(dtype).requires_grad_(True)
        self._quaternions = t("_quaternions").to(dtype).requires_grad_(True)
        # int32, as open3d's triangles are (sugar_model.py:162-164): the stand-in Meshes converts it to a new int64 tensor every call
        self._surface_mesh_faces = torch.nn.Parameter(t("faces").to(torch.int32), requires_grad=False)
        self.surface_triangle_bary_coords = t("bary").to(dtype)[..., None]
        self.surface_mesh_thickness = t("thickness").to(dtype).reshape(())
        self.n_gaussians_per_surface_triangle = n
        self.device = torch.device(DEV)

    def _all(self):
        return torch_binding(self._points, self._surface_mesh_faces, self.surface_triangle_bary_coords, self._scales, self._quaternions,
                             self.surface_mesh_thickness, self.n_gaussians_per_surface_triangle)

    points = property(lambda self: self._all()[0])
    scaling = property(lambda self: self._all()[1])
    quaternions = property(lambda self: self._all()[2])

    @property
    def surface_mesh(self):                                     # sugar_model.py:552-560: a NEW Meshes on every read
        from pytorch3d.structures import Meshes
        return Meshes(verts=[self._points.to(self.device)], faces=[self._surface_mesh_faces.to(self.device)])


BoundStandIn.scale_activation = torch.exp     # (a plain class attribute: `self.scale_activation is torch.exp`, sugar_model.py:20)


def _fresh_standin_class():
    return type("SuGaR", (BoundStandIn,), {"points": BoundStandIn.points, "scaling": BoundStandIn.scaling,
                                           "quaternions": BoundStandIn.quaternions})


def _adam_run(model, steps, weights, guard=None):
    """a fixed seeded loss on the three properties plus the regulariser as refine.py:776-783 calls it,
    `mesh_normal_consistency(model.surface_mesh)`; returns the parameters"""
    from pytorch3d.loss import mesh_normal_consistency
    params = [model._points, model._scales, model._quaternions]
    opt = torch.optim.Adam(params, lr=1e-3, eps=1e-15, foreach=False, capturable=True)
    dtype = model._points.dtype
    w = [x.to(dtype) for x in weights]
    entered = False
    try:
        for it in range(steps):
            if guard is not None and it == 1:
                guard.__enter__()
                entered = True
            opt.zero_grad(set_to_none=True)
            loss = ((model.points * w[0]).sum() + (model.scaling * w[1]).sum() + ((model.quaternions - w[2]) ** 2).sum()
                    + (model.points ** 2).sum() + 0.1 * mesh_normal_consistency(model.surface_mesh))
            loss.backward()
            opt.step()
    finally:
        if entered:
            guard.__exit__(None, None, None)
    return [p.detach().clone() for p in params]


def _sync_debug_mode_works():
    """does torch.cuda.set_sync_debug_mode("error") raise on a synchronising call with this torch on ROCm?"""
    torch.cuda.set_sync_debug_mode("error")
    try:
        torch.ones(1, device=DEV).item()
    except RuntimeError:
        return True
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return False


class _NoSync:
    """steps 2-20 make no host synchronisation.  Where the installed torch honours torch.cuda.set_sync_debug_mode("error") on ROCm, that;
    otherwise `Tensor.item`, `.cpu`, `.tolist` and `torch.cuda.synchronize` are wrapped in counting stand-ins for those steps and the count
    (of calls from anywhere, not only from sugar_amd.mesh_bind) must be zero.  `mode` says which of the two was used."""
    NAMES = ("item", "cpu", "tolist")

    def __init__(self):
        self.mode = "set_sync_debug_mode" if _sync_debug_mode_works() else "counting"
        self.count = 0

    def __enter__(self):
        if self.mode == "set_sync_debug_mode":
            torch.cuda.set_sync_debug_mode("error")
            return self
        self._saved = {k: getattr(torch.Tensor, k) for k in self.NAMES}
        self._saved_sync = torch.cuda.synchronize

        def counting(fn):
            def wrapped(*a, **k):
                self.count += 1
                return fn(*a, **k)
            return wrapped
        for k, fn in self._saved.items():
            setattr(torch.Tensor, k, counting(fn))
        torch.cuda.synchronize = counting(self._saved_sync)
        return self

    def __exit__(self, *a):
        if self.mode == "set_sync_debug_mode":
            torch.cuda.set_sync_debug_mode("default")
            return
        for k, fn in self._saved.items():
            setattr(torch.Tensor, k, fn)
        torch.cuda.synchronize = self._saved_sync


def test_through_the_class_adam_steps(fx):
    """the patched properties on a stand-in object: 20 Adam steps three ways -- HIP path, torch path in float32, torch path in float64;
    the HIP run ends no further from the float64 run than twice the float32 torch run does; steps 2-20 without a host synchronisation.
    The loss includes `mesh_normal_consistency(model.surface_mesh)` with the stand-in's switch on, the faces are an int32 Parameter and
    `surface_mesh` builds a new Meshes every step: ONE topology build serves all 20 steps and all three users."""
    import types
    from sugar_amd import sugar_patch
    n = 6
    g = torch.Generator().manual_seed(23)
    P = fx[f"n{n}__scales"].shape[0]
    weights = [torch.randn(P, 3, generator=g).to(DEV), torch.randn(P, 3, generator=g).to(DEV),
               torch.nn.functional.normalize(torch.randn(P, 4, generator=g), dim=-1).to(DEV)]
    plain = _fresh_standin_class()
    p64 = _adam_run(plain(fx, n, torch.float64), 20, weights)
    p32 = _adam_run(plain(fx, n, torch.float32), 20, weights)
    patched = _fresh_standin_class()
    module = types.SimpleNamespace(SuGaR=patched, use_old_method=False)
    sugar_patch.install_binding(module)
    model = patched(fx, n, torch.float32)
    from sugar_amd import mesh_bind
    import pytorch3d.loss as p3d_loss
    calls, built, regulariser = [], [], []
    real, real_init, real_nc = mesh_bind._backward, mesh_bind.MeshTopology.__init__, mesh_bind._NormalConsistency.backward
    mesh_bind._backward = lambda *a, **k: calls.append(1) or real(*a, **k)

    def counting_init(self, *a, **k):
        built.append(1)
        real_init(self, *a, **k)
    mesh_bind.MeshTopology.__init__ = counting_init
    mesh_bind._NormalConsistency.backward = staticmethod(lambda ctx, grad: regulariser.append(1) or real_nc(ctx, grad))
    mesh_bind.MeshTopology.clear()
    guard = _NoSync()
    try:
        p3d_loss.USE_HIP_NORMAL_CONSISTENCY = True       # what shims.install(patch_binding=...) sets
        ph = _adam_run(model, 20, weights, guard=guard)
    finally:
        p3d_loss.USE_HIP_NORMAL_CONSISTENCY = False
        mesh_bind._backward, mesh_bind.MeshTopology.__init__, mesh_bind._NormalConsistency.backward = real, real_init, real_nc
        torch.cuda.set_sync_debug_mode("default")
        sugar_patch.uninstall_binding(module)
    assert len(calls) == 60, "the HIP path did not serve points (read twice) and quaternions on every step"
    assert len(regulariser) == 20, "the regulariser did not go through the HIP path on every step"
    assert len(built) == 1, f"the topology of the int32 faces Parameter was built {len(built)} times in 20 steps"
    assert guard.count == 0, f"{guard.count} synchronising calls in steps 2-20"
    print(f"\n20 Adam steps through the patched class (no-synchronisation check: {guard.mode}):")
    for name, a, b, c in zip(("_points", "_scales", "_quaternions"), ph, p32, p64):
        assert torch.isfinite(a).all()
        check(name, a, b, c)
