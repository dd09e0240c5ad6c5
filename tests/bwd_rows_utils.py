"""The scene, the injected sums and the float32 yardstick of the row-by-row tests of the backward preprocess
(tests/test_preprocess_bwd_reference.py on the CPU, tests/test_gpu_preprocess_bwd_rows.py on the GPU).

The scene is the smallest one that reaches every branch of k_preprocess_bwd: 800 Gaussians of syn.make_scene and 210 constructed
ones (centres beyond 1.3 tanfov in x, in y, in both; the eight combinations of colour-clamp bits; needles and discs; sub-pixel
Gaussians; depths next to the 0.2 cull; zero quaternions and opacity logits of +-12 in raw mode), at 128 x 96 pixels.  The nine
sums of a row are injected, not computed by a blend backward: without its float atomics every output can be compared row by row."""
from __future__ import annotations

import ctypes as C
import functools
from typing import NamedTuple

import numpy as np
import torch

from oracle import cpu_oracle as orc
from oracle import torch_cpu_rasterizer as tcr
from sugar_amd import synthetic as syn

W, H = 128, 96
N_BASE = 800
GROUPS = (("clamp_x", 24), ("clamp_y", 24), ("clamp_xy", 16), ("colour", 80), ("needle", 24), ("subpixel", 24), ("near", 12),
          ("zero_quat", 6))
P_FULL = N_BASE + sum(n for _, n in GROUPS)  # 1010: 15 waves and 50 rows, 3 workgroups and 242 rows
N_ONE_SLOT, N_NEG_ZERO, ZERO_SHARE = 6, 12, 0.30
GRADS = ("mean3D", "scale", "rot", "sh", "cov3D")


class RowScene(NamedTuple):
    means3D: np.ndarray     # [P,3] float32
    raw_scales: np.ndarray  # [P,3] log scales
    raw_rot: np.ndarray     # [P,4] quaternions of norm 1e-3 .. 1e3 (zero_quat: exactly zero)
    raw_opac: np.ndarray    # [P] logits (opac12: +-12)
    scales: np.ndarray      # exp(raw_scales) in float32
    rot_given: np.ndarray   # non-raw mode: quaternions of norm 0.9 .. 1.1, used as given
    rot_unit: np.ndarray    # torch.nn.functional.normalize(raw_rot) in float32 (zero stays zero): what raw mode renders with
    opac: np.ndarray        # sigmoid(raw_opac) in float32
    shs: np.ndarray         # [P,16,3]
    groups: dict            # name -> row indices (in the scene's final order)
    sums: np.ndarray        # [P,9] float32, the default injection


def camera(i=0):
    return syn.orbit_cameras(W, H)[i]


def _world(cam, txtz, tytz, z):
    """view-space (t.x / t.z, t.y / t.z, t.z) -> world positions"""
    V = cam.viewmatrix.double().numpy()
    pv = np.stack([txtz * z, tytz * z, z], axis=1)
    return (pv - V[3, :3]) @ V[:3, :3].T


@functools.lru_cache(maxsize=None)
def scene(shuffled=True) -> RowScene:
    cam = camera(0)
    rng = np.random.default_rng(20)
    base = syn.make_scene(N_BASE, 5, 0.01, 0.08)
    n_c = P_FULL - N_BASE
    means = np.zeros((n_c, 3)); scales = np.zeros((n_c, 3))
    shs = np.concatenate([(rng.random((n_c, 1, 3)) - 0.5) / tcr.SH_C0, rng.standard_normal((n_c, 15, 3)) * 0.1], axis=1)
    tfx, tfy = cam.tanfovx, cam.tanfovy
    u = lambda lo, hi, *s: rng.random(s) * (hi - lo) + lo
    sign = lambda n: np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    names = np.concatenate([np.full(n, k) for k, (_, n) in enumerate(GROUPS)])
    o = 0
    for name, n in GROUPS:
        sl = slice(o, o + n); o += n
        if name in ("clamp_x", "clamp_y", "clamp_xy"):
            # beyond 1.3 tanfov by 8 .. 50 %, and so large (sigma = 0.2 .. 0.35 of the depth, ~30 pixels) that they reach the screen
            z = u(1.5, 3.0, n)
            out_x = sign(n) * 1.3 * tfx * u(1.08, 1.5, n); in_x = u(-0.7, 0.7, n) * tfx
            out_y = np.where((np.arange(n) // 2) % 2 == 0, 1.0, -1.0) * 1.3 * tfy * u(1.08, 1.5, n); in_y = u(-0.7, 0.7, n) * tfy
            means[sl] = _world(cam, in_x if name == "clamp_y" else out_x, in_y if name == "clamp_x" else out_y, z)
            scales[sl] = z[:, None] * u(0.2, 0.35, n, 3)
        elif name == "near":
            means[sl] = _world(cam, u(-0.5, 0.5, n) * tfx, u(-0.5, 0.5, n) * tfy, u(0.21, 0.39, n))
            scales[sl] = u(0.003, 0.01, n, 3)
        else:
            means[sl] = u(-0.6, 0.6, n, 3)
            scales[sl] = u(0.02, 0.06, n, 3)
            if name == "needle":  # scale ratios of 1e3: needles (one long axis) and discs (two)
                s = u(0.05, 0.15, n)
                scales[sl] = s[:, None] * np.where(np.arange(3)[None] <= (np.arange(n) % 2)[:, None], 1.0, 1e-3)
            if name == "subpixel":
                scales[sl] = u(1e-4, 1e-3, n, 3)
    means = np.concatenate([base.means3D.numpy().astype(np.float64), means]).astype(np.float32)
    scales = np.concatenate([base.scales.numpy().astype(np.float64), scales])
    shs = np.concatenate([base.shs.numpy().astype(np.float64), shs])
    group_id = np.concatenate([np.full(N_BASE, -1), names])
    # the eight combinations of clamp bits: every channel's value before the clamp is +-(0.05 .. 0.5), the sign set by its bit
    col = np.flatnonzero(group_id == [k for k, _ in GROUPS].index("colour"))
    shs[col, 1:] = rng.standard_normal((len(col), 15, 3)) * 0.003
    shs[col, 0] = 0.0
    d = torch.as_tensor(means[col].astype(np.float64)) - cam.campos.double()[None]
    rest = tcr.eval_sh_unclamped(3, torch.as_tensor(shs[col]), d / d.norm(dim=1, keepdim=True)).numpy()  # (0.5 + the rest)
    bits = (np.arange(len(col)) % 8)[:, None] >> np.arange(3)[None] & 1
    target = np.where(bits == 1, -1.0, 1.0) * u(0.05, 0.5, len(col), 3)
    shs[col, 0] = (target - rest) / tcr.SH_C0
    P = P_FULL
    q = rng.standard_normal((P, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
    raw_rot = q * 10.0 ** u(-3.0, 3.0, P, 1)
    raw_rot[group_id == [k for k, _ in GROUPS].index("zero_quat")] = 0.0
    raw_opac = np.concatenate([torch.logit(base.opacities.double().reshape(-1)).numpy(), rng.standard_normal(n_c) * 2.0])
    opac12 = np.arange(0, N_BASE, 50)  # 16 rows of the base scene
    raw_opac[opac12] = np.where(np.arange(len(opac12)) % 2 == 0, 12.0, -12.0)
    rot_given = q * u(0.9, 1.1, P, 1)

    perm = np.random.default_rng(21).permutation(P) if shuffled else np.arange(P)
    f = lambda a: np.ascontiguousarray(np.asarray(a)[perm].astype(np.float32))
    group_id = group_id[perm]
    groups = {name: np.flatnonzero(group_id == k) for k, (name, _) in enumerate(GROUPS)}
    groups["base"] = np.flatnonzero(group_id == -1)
    groups["opac12"] = np.flatnonzero(np.isin(perm, opac12))
    # the activated parameters, as a float32 caller of the reference forms them (torch, float32)
    raw_rot32, raw_scales, raw_opac32 = f(raw_rot), f(np.log(scales)), f(raw_opac)
    t = torch.as_tensor
    sc = RowScene(f(means), raw_scales, raw_rot32, raw_opac32, torch.exp(t(raw_scales)).numpy(), f(rot_given),
                  torch.nn.functional.normalize(t(raw_rot32), dim=1, eps=1e-12).numpy(), torch.sigmoid(t(raw_opac32)).numpy(), f(shs),
                  groups, None)
    return sc._replace(sums=default_sums(sc))


def default_sums(sc):
    """standard normal in all nine slots, except (rows of the base scene only, so that every constructed row is a touched one):
    N_ONE_SLOT rows per slot with that slot alone non-zero, N_NEG_ZERO rows of nine -0.0, and ZERO_SHARE of all rows all zero"""
    rng = np.random.default_rng(22)
    P = sc.means3D.shape[0]
    sums = rng.standard_normal((P, 9)).astype(np.float32)
    pick = rng.permutation(sc.groups["base"])
    o = 0
    for slot in range(9):
        rows = pick[o:o + N_ONE_SLOT]; o += N_ONE_SLOT
        v = sums[rows, slot].copy()
        sums[rows] = 0.0
        sums[rows, slot] = v
    sums[pick[o:o + N_NEG_ZERO]] = -0.0; o += N_NEG_ZERO
    sums[pick[o:o + int(ZERO_SHARE * P)]] = 0.0
    # ... and one of Sxx, Sxy, Syy at a time, of those that reach the clamped axis: see conic_only_rows
    for group, slots in (("clamp_x", (6, 7)), ("clamp_y", (8, 7)), ("clamp_xy", (6, 7, 8))):
        rows = sc.groups[group][1::2]
        keep = np.array(slots)[np.arange(len(rows)) % len(slots)]
        v = sums[rows, keep].copy()
        sums[rows] = 0.0
        sums[rows, keep] = v
    return sums


def conic_only_rows(sc):
    """Every second row of the three clamp groups carries ONE of Sxx, Sxy, Syy alone (in turn; not Syy where only x is clamped, nor
    Sxx where only y is: their share of that axis is cov2D's off-diagonal squared).  The frustum clamp acts on the path
    from the conic's cotangent through J to the mean; with all nine sums of the same size that path is 1e-4 .. 5e-3 of the row's
    dL_dmean3D (the mean2D path carries a factor 0.5 W), on these rows it is the whole row.  One slot, not three: a centre clamped
    in x and y moves along the view axis only, the three slots' terms are then multiples of one vector, and three random multiples
    of 1e-5 were seen (in float64) to leave 7e-8 -- a residue whose relative error says nothing about an implementation."""
    return np.concatenate([sc.groups[k][1::2] for k in ("clamp_x", "clamp_y", "clamp_xy")])


def special_rows(sc):
    """-> (one_slot: list of nine index arrays, neg_zero rows): recovered from the default sums"""
    s = sc.sums
    nz = s != 0
    one = [np.flatnonzero(nz[:, k] & (nz.sum(1) == 1)) for k in range(9)]
    neg = np.flatnonzero((~nz).all(1) & np.signbit(s).all(1))
    return one, neg


def inputs(sc, cam, *, raw=False, P=None, mode="sh", D=3, M=16, cov=False, scale_modifier=1.0):
    """keyword arguments of the float64 reference for one case: the parameters as the KERNEL is given them (raw or activated)
    mode: "sh" or "colors" (colors_precomp); cov: cov3D_precomp instead of scales and rotations (non-raw only)"""
    P = P or sc.means3D.shape[0]
    kw = dict(means3D=sc.means3D[:P], viewmatrix=cam.viewmatrix.numpy(), projmatrix=cam.projmatrix.numpy(), campos=cam.campos.numpy(),
              W=W, H=H, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, sh_degree=D, scale_modifier=scale_modifier)
    if mode == "sh":
        kw["shs"] = np.ascontiguousarray(sc.shs[:P, :M])
    else:
        kw["colors_precomp"] = np.random.default_rng(23).random((P_FULL, 3)).astype(np.float32)[:P]
    if cov:
        kw["cov3D_precomp"] = cov6(sc, scale_modifier)[:P]
    elif raw:
        kw["scales"], kw["rotations"] = sc.raw_scales[:P], sc.raw_rot[:P]
    else:
        kw["scales"], kw["rotations"] = sc.scales[:P], sc.rot_given[:P]
    return kw


def cov6(sc, mod):
    S = tcr.cov3d_from_scale_rot(torch.as_tensor(sc.scales).double(), mod, torch.as_tensor(sc.rot_given).double())
    return torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], dim=1).float().contiguous().numpy()


def activated(sc, kw, raw):
    """the same case as the float32 oracle takes it: activated parameters"""
    kw = dict(kw)
    if raw:
        P = kw["means3D"].shape[0]
        kw["scales"], kw["rotations"] = sc.scales[:P], sc.rot_unit[:P]
    return kw


def oracle_forward(sc, kw, raw):
    """oracle.cpu_oracle.forward of a case -> (state, record in the reference's terms)"""
    P = kw["means3D"].shape[0]
    a = activated(sc, kw, raw)
    st = orc.forward(a.pop("means3D"), sc.opac[:P], bg=np.zeros(3, np.float32), **a)
    rec = dict(opacity=st["conic_opacity"][:, 3].copy(), conic=st["conic_opacity"][:, :3].copy(),
               clamped=st["clamped"].astype(bool), radii=st["radii"].copy())
    return st, rec


def oracle_rows(sc, kw, raw, st, rec, sums):
    """The float32 yardstick: the finishing step in float32, then orc_preprocess_backward (oracle/cpu_rasterizer.c) over the injected
    cotangents, then -- in raw mode -- the chain rule of the three activations in float32 (torch).  `st`: the oracle's forward state (its
    float32 cov3D); `rec`: the record whose opacity, conic, clamp bits and radii are used (the oracle's own, or the kernel's).
    -> dict like preprocess_backward_ref's, float32"""
    f32 = np.float32
    a = activated(sc, kw, raw)
    P = a["means3D"].shape[0]
    S = np.asarray(sums, f32).reshape(P, 9)
    op, cn = np.asarray(rec["opacity"], f32).reshape(-1), np.asarray(rec["conic"], f32)
    vis = np.asarray(rec["radii"]) > 0
    dm2 = np.zeros((P, 3), f32)
    dm2[:, 0] = -(op * f32(0.5 * W)) * (cn[:, 0] * S[:, 4] + cn[:, 1] * S[:, 5])
    dm2[:, 1] = -(op * f32(0.5 * H)) * (cn[:, 2] * S[:, 5] + cn[:, 1] * S[:, 4])
    dcn = np.zeros((P, 4), f32)
    dcn[:, [0, 1, 3]] = f32(-0.5) * op[:, None] * S[:, 6:9]
    dcol = np.ascontiguousarray(S[:, 0:3])
    dm2[~vis] = 0; dcn[~vis] = 0; dcol[~vis] = 0
    shs, colors, cov = a.get("shs"), a.get("colors_precomp"), a.get("cov3D_precomp")
    M = 0 if shs is None else shs.shape[1]
    g = dict(mean3D=np.zeros((P, 3), f32), cov3D=np.zeros((P, 6), f32), sh=np.zeros((P, max(M, 1), 3), f32),
             scale=np.zeros((P, 3), f32), rot=np.zeros((P, 4), f32))
    p = orc._p
    c = lambda x: None if x is None else np.ascontiguousarray(x, dtype=f32)
    radii = np.ascontiguousarray(rec["radii"], dtype=np.int32)
    clamped = np.ascontiguousarray(np.asarray(rec["clamped"]).astype(np.uint8))
    cov_ptr = c(cov) if cov is not None else st["cov3D"]
    scl, rot = (None, None) if cov is not None else (c(a["scales"]), c(a["rotations"]))
    orc.lib().orc_preprocess_backward(
        C.c_int(P), C.c_int(a["sh_degree"]), C.c_int(M), p(c(a["means3D"])), p(radii), p(c(shs)), p(clamped), p(scl), p(rot),
        C.c_float(a["scale_modifier"]), p(cov_ptr), p(c(a["viewmatrix"])), p(c(a["projmatrix"])), C.c_int(W), C.c_int(H),
        C.c_float(a["tanfovx"]), C.c_float(a["tanfovy"]), p(c(a["campos"])), p(dm2), p(dcn), p(g["mean3D"]), p(dcol), p(g["cov3D"]),
        p(g["sh"]), p(g["scale"]), p(g["rot"]))
    g["opacity"] = np.where(vis, S[:, 3], f32(0))
    if raw:  # the chain rule of the three activations as float32 autograd applies it
        t = torch.as_tensor
        rs, rq = t(np.asarray(kw["scales"], f32)).requires_grad_(True), t(np.asarray(kw["rotations"], f32)).requires_grad_(True)
        torch.exp(rs).backward(t(g["scale"]))
        torch.nn.functional.normalize(rq, dim=1, eps=1e-12).backward(t(g["rot"]))
        g["scale"], g["rot"] = rs.grad.numpy(), rq.grad.numpy()
        g["opacity"] = g["opacity"] * op * (f32(1) - op)
    if cov is not None:
        del g["scale"], g["rot"]
    else:
        del g["cov3D"]
    if shs is None:
        del g["sh"]
    return g


def row_err(got, ref, rows):
    """err(row) = max|got - ref| / max|ref row| over `rows` whose reference row is not all zero; the others must be zero exactly.
    -> (err [n], the rows it belongs to)"""
    got = np.asarray(got, np.float64).reshape(len(ref), -1)[rows]
    ref = np.asarray(ref, np.float64).reshape(len(ref), -1)[rows]
    top = np.abs(ref).max(axis=1)
    live = top > 0
    assert not got[~live].any(), "rows whose reference is exactly zero must be exactly zero"
    return np.abs(got[live] - ref[live]).max(axis=1) / top[live], np.asarray(rows)[live]


def touched(sums):
    return (np.asarray(sums).reshape(-1, 9) != 0).any(axis=1)


def describe(name, err):
    if not len(err):
        return f"{name}: no rows"
    return f"{name}: rows {len(err)} max {err.max():.3e} median {np.median(err):.3e} p99 {np.quantile(err, 0.99):.3e}"
