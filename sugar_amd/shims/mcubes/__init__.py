"""Stand-in for PyMCubes (`import mcubes`, sugar_extractors/coarse_mesh.py:625), which is not in the ROCm image: the one function the
reference calls, over the HIP kernels of sugar_amd.marching_cubes.

    vertices, triangles = mcubes.marching_cubes(densities.cpu().numpy(), density_th)        # coarse_mesh.py:660, :703

takes a 3-D numpy array and an isovalue and returns numpy arrays, vertices[V,3] float64 in index coordinates and triangles[T,3] int64
-- with this module on the path the reference's `use_marching_cubes` branch runs unmodified up to its open3d calls.  The volume goes
to the current ROCm device and the mesh comes back; there is no CPU implementation here (no ROCm device: RuntimeError)."""
import numpy as np

__all__ = ["marching_cubes"]


def marching_cubes(volume, isovalue):
    vol = np.asarray(volume)
    if vol.ndim != 3:
        raise ValueError("mcubes.marching_cubes: volume must be a 3-D array")
    if vol.dtype.kind not in "fiub":
        raise TypeError("mcubes.marching_cubes: volume must be a numeric array")
    isovalue = float(isovalue)
    if not np.isfinite(isovalue):
        raise ValueError("mcubes.marching_cubes: isovalue must be finite")
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("mcubes.marching_cubes (sugar_amd stand-in): needs a ROCm device; there is no CPU fallback")
    from sugar_amd.marching_cubes import marching_cubes as hip_marching_cubes
    dev = torch.device("cuda", torch.cuda.current_device())
    verts, faces = hip_marching_cubes(torch.from_numpy(np.ascontiguousarray(vol, dtype=np.float32)).to(dev), isovalue)
    return verts.cpu().numpy().astype(np.float64), faces.cpu().numpy()
