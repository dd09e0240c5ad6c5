#!/usr/bin/env python
"""Golden fixture for the refined mesh's UV texture, written by the reference's OWN function on the CPU:

  extract_texture_image_and_uv_from_gaussians(rc, square_size=10, n_sh=1)     sugar_scene/sugar_model.py:2464-2677

(the call of sugar_extractors/refined_mesh.py:191-193) on the mesh-bound SuGaR of make_sugar_callsite.py (`run_bound`, on a
coarser bumpy sphere: 324 triangles), once with n = 1 and once with n = 6 Gaussians per triangle.  Test-only substitutions as in
make_sugar_callsite.py (identity `.cuda()`, the CPU-oracle Gaussian rasterizer); the function's pytorch3d imports resolve to
the stand-ins of sugar_amd.shims (AmbientLights, MeshRenderer, SoftPhongShader, BlendParams; MeshRasterizer on the CPU ORACLE
z-buffer, tests/mesh_backend.py).  Six cameras at 128 x 96: four orbit views, a close-up in which many pixels map to one texel,
and one whose far plane (zfar = 2.75) cuts through the mesh so that covered pixels lie beyond it or blend towards the background.

Recorded once (the same mesh and cameras serve both models): verts, faces, per view the NDC face verts the rasterizer received,
znear / zfar and the camera (R, T, K), the outputs verts_uv / faces_uv, and the visit counters (the function's local
`texture_counter`, read back through a recording `torch.zeros`).  Per model: the other inputs of the texture kernels (Gaussian
centres, M = get_covariance(return_full_matrix, return_sqrt, inverse_scales), DC features), the Gaussian render the function
baked, the init-only texture of a second call in which every view misses the mesh, and the final texture at the visited texels
(`texture_visited`, 0 elsewhere: an unvisited texel keeps its init value).  To keep the file small, the render handed to the
function is quantised to multiples of 1/256 and zeroed where the mesh does not cover the pixel (the function reads covered pixels
only); the function bakes exactly what is recorded.

The GPU test (tests/test_gpu_texture.py) replays this file through the HIP kernels; it never imports the reference.

    python tests/golden/make_sugar_texture.py      -> tests/golden/sugar_texture.npz
"""
import contextlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import make_sugar_callsite as mk  # noqa: E402
import make_sugar_field as mf  # noqa: E402

W, H = 128, 96
SQUARE = 10
ZFAR_CUT = (5, 2.75)     # camera 5 gets this far plane
SHARED = ("verts", "faces", "R", "T", "K", "znear", "zfar", "face_verts_ndc", "verts_uv", "faces_uv", "counter")


def full_texture(d, pre):
    """the reference's final texture of model `pre` ("n1_" / "n6_"): the visited texels, the init value everywhere else"""
    return np.where(d["counter"][..., None] > 0, d[pre + "texture_visited"], d[pre + "texture_init"])


def cameras():
    from sugar_amd import synthetic as syn
    cams = syn.orbit_cameras(W, H, n=4, radius=3.0, elev_deg=20.0)
    cams.append(syn.look_at_camera((1.05, 0.25, 0.3), (0.0, 0.0, 0.0), W, H))          # close-up: triangles span many pixels
    cams.append(syn.look_at_camera((-2.4, 1.4, -1.0), (0.0, 0.0, 0.0), W, H))          # far plane through the mesh
    return cams


class Cameras(mf.Cameras):
    """CamerasWrapper's length: the number of training cameras (sugar_model.py:2648)"""
    def __len__(self):
        return len(self.camera_to_worlds)


def build_model(sm, n_per_triangle, seed):
    cams = cameras()
    tc = Cameras(cams)
    tc.p3d_cameras.zfar[ZFAR_CUT[0]] = ZFAR_CUT[1]
    nerf = types.SimpleNamespace(device=torch.device("cpu"), training_cameras=tc)
    mesh = mk._bumpy_sphere(n_lat=10, n_lon=18)
    g = torch.Generator().manual_seed(seed)
    model = sm.SuGaR(nerfmodel=nerf, points=None, colors=None, initialize=False, sh_levels=4, keep_track_of_knn=False,
                     surface_mesh_to_bind=mesh, n_gaussians_per_surface_triangle=n_per_triangle, learn_surface_mesh_positions=True,
                     learn_surface_mesh_opacity=True, learn_surface_mesh_scales=True)
    P = model._n_points
    with torch.no_grad():   # a mid-refinement state with well-separated colours
        model._scales += 0.3 * torch.randn(P, 2, generator=g) + 0.5
        model._quaternions += 0.7 * torch.randn(P, 2, generator=g)
        model.all_densities += 2.0 * torch.randn(P, 1, generator=g) + 2.5
        model._sh_coordinates_dc[...] = (torch.rand(P, 1, 3, generator=g) - 0.5) / 0.28209479177387814
        model._sh_coordinates_rest += 0.15 * torch.randn(P, 15, 3, generator=g)
    return model


def _empty_backend(face_verts, image_size, K, perspective_correct, cull_backfaces):
    Hh, Ww = image_size
    return (torch.full((Hh, Ww, K), -1, dtype=torch.int64), torch.full((Hh, Ww, K), -1.0), torch.full((Hh, Ww, K, 3), -1.0),
            torch.full((Hh, Ww, K), -1.0))


@contextlib.contextmanager
def _backend(fn):
    import sugar_amd.mesh_raster as mr
    old = mr._backend
    mr._backend = fn
    try:
        yield
    finally:
        mr._backend = old


class _ZerosRecorder(types.ModuleType):
    """`torch` as seen by sugar_model's globals, with `zeros` recording what it returns: the function's local `texture_counter`
    (a zeros tensor of shape (S, S, 1), updated in place by its index_put_ rounds) is read back after the call"""
    def __init__(self):
        super().__init__("torch")
        self.made = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def zeros(self, *a, **k):
        t = torch.zeros(*a, **k)
        self.made.append(t)
        return t


@contextlib.contextmanager
def _record_zeros(sm):
    rec = _ZerosRecorder()
    old = sm.torch
    sm.torch = rec
    try:
        yield rec
    finally:
        sm.torch = old


def run_model(sm, n_per_triangle, seed):
    from tests.mesh_backend import oracle_backend
    from pytorch3d.renderer import MeshRasterizer, RasterizationSettings
    model = build_model(sm, n_per_triangle, seed)
    out = {}
    p3d = model.nerfmodel.training_cameras.p3d_cameras
    verts = model.surface_mesh.verts_list()[0].detach()
    faces = model.surface_mesh.faces_list()[0]
    out["verts"] = verts.numpy().copy()
    out["faces"] = faces.numpy().astype(np.int64)
    out["points"] = model.points.detach().numpy().copy()
    out["M"] = model.get_covariance(return_full_matrix=True, return_sqrt=True, inverse_scales=True).detach().numpy().copy()
    out["features_dc"] = model.sh_coordinates[:, 0].detach().numpy().copy()
    out["R"], out["T"], out["K"] = p3d.R.numpy().copy(), p3d.T.numpy().copy(), p3d.K.numpy().copy()
    out["znear"], out["zfar"] = p3d.znear.numpy().astype(np.float32), p3d.zfar.numpy().astype(np.float32)
    fvs = []
    for c in range(len(p3d)):
        mesh_proj = MeshRasterizer(cameras=p3d[c]).transform(model.surface_mesh)
        fvs.append(mesh_proj.verts_list()[0][faces].detach().numpy())
    out["face_verts_ndc"] = np.stack(fvs)
    renders = []
    real_render = model.render_image_gaussian_rasterizer

    def recording_render(**k):
        img = real_render(**k).detach().clamp(min=0, max=1)
        fr = MeshRasterizer(cameras=p3d[k["camera_indices"]], raster_settings=RasterizationSettings(
            image_size=(model.image_height, model.image_width), blur_radius=0.0, faces_per_pixel=1))(model.surface_mesh)
        img = torch.round(img * 256.0) / 256.0 * (fr.zbuf[0, ..., 0] > 0)[..., None]
        renders.append(img.numpy().copy())
        return img
    with torch.no_grad(), _backend(oracle_backend):
        model.render_image_gaussian_rasterizer = recording_render
        with _record_zeros(sm) as rec:
            verts_uv, faces_uv, tex = sm.extract_texture_image_and_uv_from_gaussians(model, square_size=SQUARE, n_sh=1)
        model.render_image_gaussian_rasterizer = real_render
        S = tex.shape[0]
        counter = [t for t in rec.made if tuple(t.shape) == (S, S, 1)]
        assert len(counter) == 1, [tuple(t.shape) for t in rec.made]
        out["rgb"] = np.stack(renders)
        out["verts_uv"], out["faces_uv"] = verts_uv.numpy(), faces_uv.numpy()
        out["counter"] = counter[0][..., 0].numpy().copy()
        out["texture_visited"] = np.where(out["counter"][..., None] > 0, tex.numpy(), np.float32(0))
    with torch.no_grad(), _backend(_empty_backend):
        _, _, init = sm.extract_texture_image_and_uv_from_gaussians(model, square_size=SQUARE, n_sh=1)
        out["texture_init"] = init.numpy()
    return out


def run():
    """(single-threaded: the reference's `index_put_` without accumulate splits more than 32768 elements across threads, and
    several pixels of one view that map to the same texel then race; run serially it keeps the last of them in row-major order,
    the rule the HIP kernels implement)"""
    sm = mk._import_reference_model()
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    real_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    sm.knn_points = mk._scipy_knn_points
    from tests.oracle_rasterizer import GaussianRasterizer as OracleRasterizer
    sm.GaussianRasterizer = OracleRasterizer
    try:
        out = {"W": np.int32(W), "H": np.int32(H), "square_size": np.int32(SQUARE)}
        for n, seed in ((1, 91), (6, 92)):
            for k, v in run_model(sm, n, seed).items():
                if k in SHARED:
                    assert k not in out or np.array_equal(out[k], v), k
                    out[k] = v
                else:
                    out[f"n{n}_{k}"] = v
        return out
    finally:
        torch.Tensor.cuda = real_cuda
        torch.set_num_threads(threads)


def main():
    out = run()
    path = os.path.join(HERE, "sugar_texture.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", len(out), "arrays")
    for k in sorted(out):
        a = np.asarray(out[k])
        print(f"  {k:24s} {str(a.shape):20s} {a.dtype}  mean {float(a.astype(np.float64).mean()):.5g}")


if __name__ == "__main__":
    sys.exit(main())
