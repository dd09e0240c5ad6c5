#!/usr/bin/env python
"""Golden fixture for the density grid of the marching-cubes extraction (sugar_extractors/coarse_mesh.py:623-660), from the
reference's OWN methods.  With make_sugar_field.py's substitutions (the reference's sugar_scene/sugar_model.py imported untouched,
identity `.cuda()`, scipy k-NN, the CPU-oracle-backed rasterizer) the same small mid-training SuGaR model is built on the CPU and the
extractor's own sequence is run:

  sugar.reset_neighbors(knn_to_track=16)                      coarse_mesh.py:627
  X = Y = Z = torch.linspace(-1, 1, R) * extent               :635-637  (R = 40 here, 512 there)
  pts = meshgrid(X, Y, Z) flattened                           :639-640
  densities = sugar.compute_density(pts).reshape(R, R, R)     :653-655  (sugar_model.py:1345-1368)

The file holds the inputs (`points`, `inv_scaled_rot` = get_covariance(return_full_matrix, return_sqrt, inverse_scales), `strengths`,
`sh_dc`), the grid axes, the model's neighbour table after reset_neighbors(16) (the exact 16 nearest neighbours of every Gaussian, the
choice any exact k-NN makes) and the density volume.  tests/test_marching_cubes_cpu.py re-runs `run()` against the committed file where
the reference tree is present; tests/test_gpu_marching_cubes.py replays it through sugar_amd.extract.density_grid.

    python tests/golden/make_sugar_mcgrid.py      -> tests/golden/sugar_mcgrid.npz
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
import make_sugar_field as mf  # noqa: E402

R = 40
EXTENT = 0.9   # the model's points lie within ~0.7 of the origin


def run():
    sm = mk._import_reference_model()
    real_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    old_knn = sm.knn_points
    sm.knn_points = mk._scipy_knn_points
    try:
        model, _ = mf.build_model(sm)
        with torch.no_grad():
            model.reset_neighbors(knn_to_track=16)
            X = torch.linspace(-1, 1, R) * EXTENT
            xx, yy, zz = torch.meshgrid(X, X, X, indexing="ij")
            pts = torch.cat([xx.reshape(-1, 1), yy.reshape(-1, 1), zz.reshape(-1, 1)], dim=-1)
            densities = model.compute_density(pts).reshape(R, R, R)
            B = model.get_covariance(return_full_matrix=True, return_sqrt=True, inverse_scales=True)
            out = {
                "points": model.points.detach().numpy().astype(np.float32).copy(),
                "inv_scaled_rot": B.detach().numpy().astype(np.float32).copy(),
                "strengths": model.strengths.detach().numpy().astype(np.float32).reshape(-1).copy(),
                "sh_dc": model._sh_coordinates_dc.detach().numpy().astype(np.float32).reshape(-1, 3).copy(),
                "knn_idx": model.knn_idx.numpy().astype(np.int32).copy(),
                "X": X.numpy().copy(), "Y": X.numpy().copy(), "Z": X.numpy().copy(),
                "density": densities.numpy().astype(np.float32).copy(),
            }
        return out
    finally:
        torch.Tensor.cuda = real_cuda
        sm.knn_points = old_knn


def main():
    out = run()
    path = os.path.join(HERE, "sugar_mcgrid.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", len(out), "arrays")
    for k in sorted(out):
        a = np.asarray(out[k])
        print(f"  {k:16s} {str(a.shape):16s} {a.dtype}  mean {float(a.astype(np.float64).mean()):.5g}  max {float(a.max()):.5g}")


if __name__ == "__main__":
    sys.exit(main())
