"""Helpers shared by the parity tests: run the CPU oracle and the HIP path on the same seeded inputs."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from oracle import cpu_oracle as orc


def scene_kwargs(scene, cam, bg, *, use_sh=True, use_cov=False, sh_degree=3, scale_modifier=1.0):
    """numpy kwargs for oracle.cpu_oracle.forward"""
    kw = dict(viewmatrix=cam.viewmatrix.numpy(), projmatrix=cam.projmatrix.numpy(), campos=cam.campos.numpy(),
              bg=bg.numpy(), W=cam.image_width, H=cam.image_height, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy,
              sh_degree=sh_degree, scale_modifier=scale_modifier)
    if use_sh:
        kw["shs"] = scene.shs.numpy()
    else:
        kw["colors_precomp"] = precomputed_colors(scene).numpy()
    if use_cov:
        kw["cov3D_precomp"] = precomputed_cov(scene, scale_modifier).numpy()
    else:
        kw["scales"] = scene.scales.numpy()
        kw["rotations"] = scene.rotations.numpy()
    return kw


def precomputed_colors(scene):
    g = torch.Generator().manual_seed(99)
    return torch.rand(scene.means3D.shape[0], 3, generator=g)


def precomputed_cov(scene, mod=1.0):
    """Sigma = R S^2 R^T packed as (00,01,02,11,12,22) -- sugar_scene/sugar_model.py:2222-2239"""
    from oracle.torch_cpu_rasterizer import cov3d_from_scale_rot
    S = cov3d_from_scale_rot(scene.scales.double(), mod, scene.rotations.double())
    return torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], dim=1).float().contiguous()


def run_oracle(scene, cam, bg, **opts):
    kw = scene_kwargs(scene, cam, bg, **opts)
    return orc.forward(scene.means3D.numpy(), scene.opacities.numpy(), **kw)


def run_hip(scene, cam, bg, *, use_sh=True, use_cov=False, sh_degree=3, scale_modifier=1.0, grad_out=None,
            device="cuda:0", debug=False):
    """Runs the product path through the reference-shaped Python API. Returns dict of numpy arrays."""
    from sugar_amd.diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    from sugar_amd import _lib
    dev = torch.device(device)
    settings = GaussianRasterizationSettings(
        image_height=cam.image_height, image_width=cam.image_width, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy,
        bg=bg.to(dev), scale_modifier=scale_modifier, viewmatrix=cam.viewmatrix.to(dev),
        projmatrix=cam.projmatrix.to(dev), sh_degree=sh_degree, campos=cam.campos.to(dev), prefiltered=False,
        debug=debug)
    rast = GaussianRasterizer(settings)
    P = scene.means3D.shape[0]
    means3D = scene.means3D.to(dev).requires_grad_(True)
    means2D = torch.zeros(P, 3, device=dev, requires_grad=True)
    opac = scene.opacities.to(dev).requires_grad_(True)
    kw = {}
    leaves = dict(means3D=means3D, means2D=means2D, opacities=opac)
    if use_sh:
        leaves["shs"] = kw["shs"] = scene.shs.to(dev).requires_grad_(True)
    else:
        leaves["colors_precomp"] = kw["colors_precomp"] = precomputed_colors(scene).to(dev).requires_grad_(True)
    if use_cov:
        leaves["cov3D_precomp"] = kw["cov3D_precomp"] = precomputed_cov(scene, scale_modifier).to(dev).requires_grad_(True)
    else:
        leaves["scales"] = kw["scales"] = scene.scales.to(dev).requires_grad_(True)
        leaves["rotations"] = kw["rotations"] = scene.rotations.to(dev).requires_grad_(True)
    color, radii = rast(means3D=means3D, means2D=means2D, opacities=opac, **kw)
    out = dict(color=color.detach().cpu().numpy(), radii=radii.cpu().numpy())
    # private scratch, through the introspection ABI
    fn = color.grad_fn
    saved = fn.saved_tensors
    geom, binning, img = saved[7], saved[8], saved[9]
    lib = _lib.load()
    W, H = cam.image_width, cam.image_height
    R = fn.num_rendered
    out["num_rendered"] = R
    rec = geom.cpu().numpy()[: P * 48].view(np.float32).reshape(P, 12)
    out["rec"] = rec  # columns: REC_* below (GeomRec, sugar_amd/csrc/sgr_common.h)
    imgb = img.cpu().numpy()
    T = ((W + 15) // 16) * ((H + 15) // 16)
    o = lib.sgr_img_final_T_offset(W, H); out["final_T"] = imgb[o:o + W * H * 4].view(np.float32)
    o = lib.sgr_img_n_contrib_offset(W, H); out["n_contrib"] = imgb[o:o + W * H * 4].view(np.uint32)
    o = lib.sgr_img_tile_start_offset(W, H); out["tile_start"] = imgb[o:o + (T + 1) * 4].view(np.uint32)
    o = lib.sgr_img_tile_maxc_offset(W, H); out["tile_maxc"] = imgb[o:o + T * 4].view(np.uint32)
    o = lib.sgr_binning_point_list_offset(R); out["point_list"] = binning.cpu().numpy()[o:o + R * 4].view(np.uint32)
    if grad_out is not None:
        color.backward(torch.as_tensor(grad_out).to(dev))
        out["grads"] = {k: (v.grad.detach().cpu().numpy() if v.grad is not None else None) for k, v in leaves.items()}
    return out


class _PatternScratch:
    """diff_gaussian_rasterization._Scratch with every byte of the three buffers set to 0xFF (a NaN as a float, 2^32 - 1 as a count: whatever
    a test reads back was written by a kernel) and the P reach flags, which a forward only ever SETS, cleared -- both on the current
    stream, ahead of the forward's kernels"""

    def __init__(self, device, reach_offset, P):
        self.device, self.tensors, self._cbs, self.reach = device, {}, {}, (int(reach_offset), int(P))

    def cb(self, name):
        from sugar_amd import _lib

        def alloc(_user, nbytes):
            t = self.tensors[name] = torch.full((int(nbytes),), 0xFF, dtype=torch.uint8, device=self.device)
            if name == "geom":
                o, P = self.reach
                assert o + P <= int(nbytes)
                t[o:o + P] = 0
            return t.data_ptr()

        self._cbs[name] = _lib.ALLOC_FN(alloc)
        return self._cbs[name]

    def release(self):
        t, self.tensors = self.tensors, {}
        self._cbs.clear()
        return t


# float columns of the private 48-byte geometry record (GeomRec, sugar_amd/csrc/sgr_common.h)
REC_XY, REC_CONIC, REC_OPACITY, REC_DEPTH, REC_RADIUS, REC_RGB, REC_CLAMPED = slice(0, 2), [2, 3, 4], 5, 6, 7, slice(8, 11), 11


def rel_stats(a, b, floor_frac=1e-3):
    """Per-element relative error with a floor of floor_frac * max|b| (so exact zeros do not blow up)."""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    scale = np.abs(b).max() if b.size else 0.0
    floor = max(scale * floor_frac, 1e-30)
    rel = np.abs(a - b) / (np.abs(b) + floor)
    nrm = np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)
    return dict(max_rel=float(rel.max()) if rel.size else 0.0, frac_gt_1e4=float((rel > 1e-4).mean()) if rel.size else 0.0,
                norm_rel=float(nrm), max_abs=float(np.abs(a - b).max()) if a.size else 0.0, scale=float(scale))


def grad_image(W, H):
    return np.random.default_rng(0).standard_normal((3, H, W)).astype(np.float32)


MODE_RAW, MODE_SH_DIR_ELSEWHERE = 4, 8   # SGR_MODE_RAW_PARAMS, SGR_MODE_SH_DIR_ELSEWHERE


class Run:
    """One forward through the C ABI, and backwards over its scratch (sgr_backward_ex with flags).

    raw: the raw 3DGS parameters (log scale, un-normalised quaternion, opacity logit), derived from the activated scene -- or, with
    raw_given, the scene's fields hold them already.  colors / cov: colors_precomp [P,3] / cov3D_precomp [P,6] instead of the SH
    coefficients / of scales and rotations.  The image size is the camera's.
    flags: further SGR_FLAG_* bits of the forward; tile_need / tile_need_out: the walk hint going in / coming out (device uint32 per tile);
    header_host: the forward's two header copies land in self.header (pinned, 16 words; read it after a synchronize).  With
    SGR_FLAG_REACH the scratch starts as 0xFF bytes with the reach flags cleared (the forward only ever SETS them): see _PatternScratch."""

    def __init__(self, scene, cam, bg, raw, *, raw_given=False, D=3, M=16, colors=None, cov=None, scale_modifier=1.0, device="cuda:0",
                 flags=0, tile_need=None, tile_need_out=None, header_host=False):
        from sugar_amd import _lib
        from sugar_amd.diff_gaussian_rasterization import _Scratch
        self.L, self.lib = _lib, _lib.load()
        self.dev = dev = torch.device(device)
        self.P = P = scene.means3D.shape[0]
        self.W, self.H = W, H = cam.image_width, cam.image_height
        self.raw, self.D, self.M, self.mod = bool(raw), int(D), int(M), float(scale_modifier)
        f = lambda t: None if t is None else torch.as_tensor(t).to(dev).float().contiguous()
        self.means, self.shs = f(scene.means3D), (f(scene.shs[:, :M]) if colors is None else None)
        self.colors, self.cov = f(colors), f(cov)
        if raw and not raw_given:  # the raw 3DGS parameters: log scale, un-normalised quaternion, opacity logit
            self.scales, self.rots = f(scene.scales.log()), f(scene.rotations * 2.5)
            self.opac = f(torch.logit(scene.opacities))
        else:
            self.scales, self.rots, self.opac = f(scene.scales), f(scene.rotations), f(scene.opacities)
        if cov is not None:
            self.scales = self.rots = None
        self.bg, self.vm, self.pm, self.cp = f(bg), f(cam.viewmatrix), f(cam.projmatrix), f(cam.campos)
        self.tx, self.ty = float(cam.tanfovx), float(cam.tanfovy)
        self.color = torch.empty(3, H, W, device=dev)
        self.radii = torch.empty(P, dtype=torch.int32, device=dev)
        self.dpix = torch.as_tensor(grad_image(W, H)).to(dev)
        sc = _PatternScratch(dev, self.lib.sgr_geom_reach_offset_bytes(P), P) if flags & _lib.SGR_FLAG_REACH else _Scratch(dev)
        self.header = torch.zeros(16, dtype=torch.int32).pin_memory() if header_host else None
        self.tile_need, self.tile_need_out = tile_need, tile_need_out  # (kept alive)
        p = self.ptr
        opts = _lib.ForwardOpts(0, (_lib.SGR_FLAG_RAW_PARAMS if raw else 0) | int(flags), p(self.header), None, p(tile_need), p(tile_need_out),
                                0.0, 0, None, None, None)
        self.stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        self.R = self.lib.sgr_forward_ex(sc.cb("geom"), None, sc.cb("binning"), None, sc.cb("img"), None, P, self.D, self.M, p(self.bg),
                                         W, H, p(self.means), p(self.shs), p(self.colors), p(self.opac), p(self.scales), self.mod,
                                         p(self.rots), p(self.cov), p(self.vm), p(self.pm), p(self.cp), self.tx, self.ty, 0,
                                         p(self.color), p(self.radii), 0, self.stream, C.byref(opts))
        assert self.R >= 0, _lib.last_error()
        self.scratch = sc.release()

    @staticmethod
    def ptr(t):
        return None if t is None else C.c_void_p(t.data_ptr())

    def acc(self):
        """the accumulator table float[P][16] inside the geometry scratch (a view: writable)"""
        o = self.lib.sgr_geom_acc_offset_bytes(self.P)
        return self.scratch["geom"][o:o + self.P * 64].view(torch.float32).view(self.P, 16)

    def _img(self, offset_fn, n, dtype):
        torch.cuda.synchronize()
        o = offset_fn(self.W, self.H)
        return self.scratch["img"][o:o + 4 * n].cpu().numpy().view(dtype)

    @property
    def tiles(self):
        return ((self.W + 15) // 16) * ((self.H + 15) // 16)

    def final_T(self):
        return self._img(self.lib.sgr_img_final_T_offset, self.W * self.H, np.float32)

    def n_contrib(self):
        return self._img(self.lib.sgr_img_n_contrib_offset, self.W * self.H, np.uint32)

    def tile_start(self):
        return self._img(self.lib.sgr_img_tile_start_offset, self.tiles + 1, np.uint32)

    def tile_maxc(self):
        return self._img(self.lib.sgr_img_tile_maxc_offset, self.tiles, np.uint32)

    def tile_walked(self):
        """uint32[T]: the furthest list position any pixel of the tile examined"""
        return self._img(self.lib.sgr_img_tile_walked_offset, self.tiles, np.uint32)

    def point_list(self):
        """the first tile_start[T] entries of the instance list: Gaussian ids, tile-major, depth order"""
        n = int(self.tile_start()[-1])
        o = self.lib.sgr_binning_point_list_offset(self.R)
        return self.scratch["binning"][o:o + 4 * n].cpu().numpy().view(np.uint32)

    def reach(self):
        """the reach table, one byte per Gaussian (SGR_FLAG_REACH), on the host"""
        torch.cuda.synchronize()
        o = self.lib.sgr_geom_reach_offset_bytes(self.P)
        return self.scratch["geom"][o:o + self.P].cpu().numpy()

    def record(self):
        """the forward's 48-byte record of every Gaussian, as float32 [P,12] on the host (columns: REC_* above)"""
        torch.cuda.synchronize()
        return self.scratch["geom"][: self.P * 48].cpu().numpy().view(np.float32).reshape(self.P, 12)

    def backward(self, phase, store_sh, flags=0, stats=True, *, mode=0, dpix=None, dens0=None, intermediates=True, sh_offset=0):
        """-> dict of device tensors: every output of the call, and the three densification statistics (going in: dens0 =
        (max_radii, accum, denom), or zeros with max_radii at 2).  mode: further SGR_MODE_* bits; intermediates=False passes NULL
        for dL_dmean2D and dL_dconic; sh_offset: dL_dsh starts that many floats past a 256-byte boundary."""
        dev, P = self.dev, self.P
        nan = lambda *s: torch.full(s, float("nan"), device=dev)
        out = dict(opacity=nan(P), color=nan(P, 3), mean3D=nan(P, 3))
        if intermediates:
            out.update(mean2D=nan(P, 3), conic=nan(P, 4))
        if self.cov is None:
            out.update(scale=nan(P, 3), rot=nan(P, 4))
        else:
            out["cov3D"] = nan(P, 6)
        if store_sh:
            self._sh_buf = nan(P * self.M * 3 + sh_offset)
            out["sh"] = self._sh_buf[sh_offset:].view(P, self.M, 3)
        p = self.ptr
        if dens0 is None:
            dens = [torch.zeros(P, device=dev) for _ in range(3)]
            dens[0].fill_(2.0)  # max_radii2D starts above the smallest radii: the maximum must keep it
        else:
            dens = [torch.as_tensor(t).to(dev).float().clone() for t in dens0]
        bo = self.L.BackwardOpts(*([t.data_ptr() for t in dens] if stats else [None] * 3), None, int(flags))
        g, b, i = (self.scratch[k] for k in ("geom", "binning", "img"))
        dpix = self.dpix if dpix is None else dpix
        rc = self.lib.sgr_backward_ex(phase | mode | (MODE_RAW if self.raw else 0), P, self.D, self.M, self.R, p(self.bg), self.W, self.H,
                                      p(self.means), p(self.shs), p(self.colors), p(self.scales), self.mod, p(self.rots), p(self.cov),
                                      p(self.vm), p(self.pm), p(self.cp), self.tx, self.ty, p(self.radii), p(g), p(b), p(i), p(dpix),
                                      p(out.get("mean2D")), p(out.get("conic")), p(out["opacity"]), p(out["color"]), p(out["mean3D"]),
                                      p(out.get("cov3D")), p(out.get("sh")), p(out.get("scale")), p(out.get("rot")), 0, self.stream,
                                      C.byref(bo))
        assert rc >= 0, self.L.last_error()
        torch.cuda.synchronize()
        if phase == 2:
            del out["color"]  # (written by phase 1)
        out.update(max_radii=dens[0], accum=dens[1], denom=dens[2])
        return out
