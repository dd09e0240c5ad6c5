#!/usr/bin/env python
"""Golden fixture from the reference's OWN methods for the kernels of csrc/sdf_regulariser.hip: sugar_scene/sugar_model.py is
imported from /root/reference, untouched (with the test-only substitutions of make_sugar_callsite.py), the model of
make_sugar_field.py (`build_model`: P = 2 500, 120 x 88, K = 16) is built on the CPU and these methods of the reference are called:

  SuGaR.sample_points_in_gaussians     :885-928    N = 6 000, mask on, proportional to volume, factor 1.5 (the call and the seeds of
                                                   make_sugar_field.py); `torch.randn_like` is wrapped for the duration of the call so
                                                   that the noise it drew is recorded next to the indices and the samples
  SuGaR.get_smallest_axis(return_idx)  :930-944    and get_normals() (:946-968)
  SuGaR.get_points_depth_in_depth_map  :1318-1333  over a seeded smooth-plus-noise depth map that requires grad, passed as the
                                                   stride-3 slice `image[..., 0]` of an [H,W,3] tensor, and camera-space points made
                                                   from the samples plus a band pushed outside the frustum

with their autograd gradients under random weight tensors.  For every recorded output or gradient `name`, `yard_<name>` is the
norm-wise distance between the reference method's float32 result and the float64 restatement of
tests/sdf_regulariser_restatement.py: what a float32 evaluation of these formulas is off by, the yardstick of the GPU test.
The model state is that of tests/golden/sugar_field.npz (asserted).  The field tail needs no fixture of its own: sugar_field.npz
holds `field_out_*`, `field_hi_*` and `field_grad_*` with weights on `sdf` and `beta`.

    python tests/golden/make_sdf_regulariser.py      -> tests/golden/sdf_regulariser.npz
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import make_sugar_callsite as mk  # noqa: E402
from make_sugar_field import N_SAMPLES, P, build_model  # noqa: E402
from tests import sdf_regulariser_restatement as rs  # noqa: E402

CAM_IDX = 3
SCALE_FACTOR = 1.5


def depth_map(H, W, seed=21):
    """smooth plus noise, around the distance of the orbit cameras to the blob"""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
    return 3.0 + 0.6 * torch.sin(5 * xx) * torch.cos(4 * yy) + 0.05 * torch.randn(H, W, generator=g)


def conditions(out, field_fx):
    """what the tests rely on (asserted here and again by tests/test_sdf_regulariser_cpu.py)"""
    frac = float(out["depth_outside"].mean())
    assert 0.05 <= frac <= 0.30, frac
    counts = np.bincount(out["sample_idx"], minlength=P)
    assert counts.min() == 0 and counts.max() >= 32, (counts.min(), counts.max())
    s = np.sort(np.exp(field_fx["state_scales"].astype(np.float64)), axis=1)
    assert (s[:, 0] < s[:, 1]).all()                   # no scaling row with two equal minima
    assert float(field_fx["field_out_density"].max()) < 0.98


def run():
    sm = mk._import_reference_model()
    real_cuda, real_randn_like = torch.Tensor.cuda, torch.randn_like
    torch.Tensor.cuda = lambda self, *a, **k: self
    sm.knn_points = mk._scipy_knn_points
    from tests.oracle_rasterizer import GaussianRasterizer as OracleRasterizer
    sm.GaussianRasterizer = OracleRasterizer
    try:
        model, cams = build_model(sm)
        field_fx = np.load(os.path.join(HERE, "sugar_field.npz"))
        for name in ("_points", "_scales", "_quaternions"):
            assert np.array_equal(getattr(model, name).detach().numpy(), field_fx["state" + name]), name
        H, W = model.image_height, model.image_width
        out = {}
        g = torch.Generator().manual_seed(5)
        wgen = torch.Generator().manual_seed(31)
        params = (model._points, model._scales, model._quaternions)
        # the float64 twin of the model's properties (sugar_model.py:383-479 for a model that is not mesh-bound)
        p64 = [t.detach().double().requires_grad_(True) for t in params]

        def props64():
            return p64[0], torch.exp(p64[1]), torch.nn.functional.normalize(p64[2], dim=-1)

        def record(name, ref32, ref64):
            out[name] = ref32.detach().numpy().copy()
            out["yard_" + name] = np.float64(rs.distance(ref32, ref64))

        def grads64(value, weights):
            for t in p64:
                t.grad = None
            (value * weights.double()).sum().backward()
            return [t.grad if t.grad is not None else torch.zeros_like(t) for t in p64]

        # ---- sample_points_in_gaussians (:885-928)
        torch.manual_seed(11)
        mask = torch.rand(P, generator=g) < 0.8
        drawn = []

        def recording_randn_like(*a, **k):
            drawn.append(real_randn_like(*a, **k))
            return drawn[-1]
        torch.randn_like = recording_randn_like
        try:
            model.zero_grad(set_to_none=True)
            samples, sample_idx = model.sample_points_in_gaussians(N_SAMPLES, sampling_scale_factor=SCALE_FACTOR, mask=mask,
                                                                   probabilities_proportional_to_volume=True)
        finally:
            torch.randn_like = real_randn_like
        assert len(drawn) == 1 and np.array_equal(samples.detach().numpy(), field_fx["field_x"])
        noise = drawn[0]
        w = torch.randn(N_SAMPLES, 3, generator=wgen)
        (samples * w).sum().backward()
        out["sample_mask"] = mask.numpy(); out["sample_idx"] = sample_idx.numpy().copy(); out["sample_noise"] = noise.numpy().copy()
        out["sample_factor"] = np.float64(SCALE_FACTOR); out["sample_w"] = w.numpy()
        pts64, sc64, q64 = props64()
        s64 = rs.sample_transform(pts64, q64, sc64, sample_idx, noise.double(), SCALE_FACTOR)
        record("sample_out", samples, s64)
        for name, t, g64 in zip(("_points", "_scales", "_quaternions"), params, grads64(s64, w)):
            record("sample_grad" + name, t.grad, g64)

        # ---- get_smallest_axis(return_idx=True) (:930-944) and get_normals() (:946-968)
        model.zero_grad(set_to_none=True)
        axis, axis_idx = model.get_smallest_axis(return_idx=True)
        normals = model.get_normals()
        assert torch.equal(normals, axis)
        w = torch.randn(P, 3, generator=wgen)
        (axis * w).sum().backward()
        out["axis_idx"] = axis_idx.numpy().copy(); out["axis_w"] = w.numpy()
        pts64, sc64, q64 = props64()
        a64, j64 = rs.smallest_axis(q64, sc64)
        assert torch.equal(j64, axis_idx)
        record("axis_out", axis, a64)
        record("normals_out", normals, a64)
        record("axis_grad_quaternions", model._quaternions.grad, grads64(a64, w)[2])
        assert model._scales.grad is None or not model._scales.grad.abs().any()

        # ---- get_points_depth_in_depth_map (:1318-1333)
        fov_camera = model.nerfmodel.training_cameras.p3d_cameras[CAM_IDX]
        image = depth_map(H, W)[..., None].repeat(1, 1, 3).contiguous().requires_grad_(True)     # an [H,W,3] render
        depth = image[..., 0]                                                                    # stride 3
        assert depth.stride() == (3 * W, 3)
        with torch.no_grad():
            cam_pts = fov_camera.get_world_to_view_transform().transform_points(samples.detach())
            cam_pts = cam_pts[cam_pts[..., 2] > float(fov_camera.znear)]
            band = cam_pts[::6].clone()                                                          # a band pushed outside the frustum
            band[:, :2] *= torch.tensor([8.0, 9.0]) * torch.sign(torch.randn(len(band), 2, generator=wgen))
            cam_pts = torch.cat((cam_pts, band)).contiguous()
        pts = cam_pts.clone().requires_grad_(True)
        map_z = model.get_points_depth_in_depth_map(fov_camera, depth, pts)
        w = torch.randn(len(pts), generator=wgen)
        (map_z * w).sum().backward()
        Pm = fov_camera.get_projection_transform().get_matrix().detach()
        out["depth_cam_idx"] = np.int32(CAM_IDX); out["depth_projection"] = Pm.numpy().copy()
        out["depth_map"] = depth.detach().numpy().copy(); out["depth_pts"] = cam_pts.numpy().copy(); out["depth_w"] = w.numpy()
        d64 = depth.detach().double().requires_grad_(True)
        x64 = cam_pts.double().requires_grad_(True)
        z64 = rs.depth_lookup(Pm.double(), d64, x64)
        (z64 * w.double()).sum().backward()
        out["depth_outside"] = rs.lookup_pixels(Pm.double(), cam_pts.double(), H, W)[2].numpy()
        record("depth_out", map_z, z64)
        record("depth_grad_pts", pts.grad, x64.grad)
        record("depth_grad_map", image.grad[..., 0], d64.grad)
        assert not image.grad[..., 1:].abs().any()
        conditions(out, field_fx)
        return out
    finally:
        torch.Tensor.cuda = real_cuda
        torch.randn_like = real_randn_like


def main():
    out = run()
    path = os.path.join(HERE, "sdf_regulariser.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", len(out), "arrays")
    for k in sorted(out):
        a = np.asarray(out[k])
        print(f"  {k:34s} {str(a.shape):16s} {a.dtype}  mean {float(a.astype(np.float64).mean()):.5g}")


if __name__ == "__main__":
    sys.exit(main())
