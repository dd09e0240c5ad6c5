"""Marching cubes on the HIP kernels of csrc/marching_cubes.hip (C ABI: sgr_marching_cubes_*, sgr_mesh_vertex_normals in
include/sugar_raster.h): what `mcubes.marching_cubes` does for the `use_marching_cubes` branch of sugar_extractors/coarse_mesh.py
(:660, :703), without leaving the device.

  marching_cubes(volume[nx,ny,nz], level) -> (verts[V,3] float32 in INDEX coordinates, faces[F,3] int64)
  vertex_normals(verts, faces)            -> normals[V,3], unit length or zero

Rules (the kernel file states them in full): a corner is inside iff its value is finite and >= level -- NaN and +-inf count as outside;
a crossed grid edge carries one vertex at t = (level - a) / (b - a) from its outside end, t = 0.5 when the outside end (or t: inf / inf) is not
finite, so no vertex is ever NaN; faces are wound with their normals towards lower values.  Vertices are welded by edge ownership and
numbered by a scan in grid order: the result is bit-identical between runs.

`marching_cubes` makes ONE device-to-host read -- the pair (V, F), which sizes the outputs (`mc_count` returns it still on the
device; `mc_emit` takes the two integers).  Nothing else in this module waits on the device.  There is no CPU path: CPU tensors raise."""
from __future__ import annotations

import torch

from . import _lib
from ._call import call, csr, need_gpu, ptr

MAX_POINTS = 2 ** 31  # nx * ny * nz must stay below this


def _volume(volume, level):
    need_gpu("marching_cubes", volume=volume)
    if volume.dim() != 3 or volume.dtype != torch.float32:
        raise ValueError("marching_cubes: volume must be a float32 tensor of shape [nx, ny, nz]")
    nx, ny, nz = (int(s) for s in volume.shape)
    if min(nx, ny, nz) < 1 or nx * ny * nz >= MAX_POINTS:
        raise ValueError(f"marching_cubes: a grid of {nx} x {ny} x {nz} points is refused: nx * ny * nz must be in [1, 2^31)")
    level = float(level)
    if level != level or level in (float("inf"), float("-inf")):
        raise ValueError("marching_cubes: level must be finite")
    return volume.detach().contiguous(), level, (nx, ny, nz)


def mc_count(volume: torch.Tensor, level: float):
    """the classify and scan passes: returns (state, counts) with counts = int64[2] = (V, F) ON THE DEVICE; no host synchronisation"""
    lib = _lib.load()
    vol, level, (nx, ny, nz) = _volume(volume, level)
    dev = vol.device
    scratch = torch.empty(lib.sgr_marching_cubes_scratch_bytes(nx, ny, nz), dtype=torch.uint8, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    call("sgr_marching_cubes_count", dev, nx, ny, nz, ptr(vol), level, ptr(scratch), ptr(counts))
    return (vol, level, scratch), counts


def mc_emit(state, n_verts: int, n_faces: int):
    """the emit passes for the (V, F) read from `mc_count`'s counts: (verts[V,3] float32, faces[F,3] int64); no host synchronisation"""
    vol, level, scratch = state
    nx, ny, nz = (int(s) for s in vol.shape)
    n_verts, n_faces = int(n_verts), int(n_faces)
    if n_verts >= MAX_POINTS or n_faces >= MAX_POINTS:
        raise ValueError(f"marching_cubes: {n_verts} vertices / {n_faces} faces do not fit 31-bit ids")
    dev = vol.device
    verts = torch.empty(n_verts, 3, dtype=torch.float32, device=dev)
    faces = torch.empty(n_faces, 3, dtype=torch.int64, device=dev)
    if n_verts or n_faces:
        call("sgr_marching_cubes_emit", dev, nx, ny, nz, ptr(vol), level, ptr(scratch), n_verts, n_faces, ptr(verts), ptr(faces))
    return verts, faces


def marching_cubes(volume: torch.Tensor, level: float):
    """(verts[V,3] float32, faces[F,3] int64) of the level set `volume == level`; vertices in index coordinates (vertex (i + t, j, k)
    lies on the grid edge from point (i, j, k) to (i + 1, j, k)).  volume: float32 [nx, ny, nz] on a ROCm device, nx * ny * nz < 2^31."""
    state, counts = mc_count(volume, level)
    n_verts, n_faces = counts.tolist()          # the one device-to-host read: it sizes the outputs
    return mc_emit(state, n_verts, n_faces)


def vertex_normals(verts: torch.Tensor, faces: torch.Tensor) -> torch.Tensor:
    """normals[V,3]: per vertex the sum of the area-weighted normals (b - a) x (c - a) of its faces, added in ascending (face, corner)
    order, normalised; zero where a vertex has no face or no area around it.  No host synchronisation."""
    need_gpu("vertex_normals", verts=verts, faces=faces)
    if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError("vertex_normals: verts must be [V,3] and faces [F,3]")
    v = verts.detach().to(torch.float32).contiguous()
    f = faces.detach().to(torch.int64).contiguous()
    V, F_ = int(v.shape[0]), int(f.shape[0])
    normals = torch.empty(V, 3, dtype=torch.float32, device=v.device)
    if V == 0:
        return normals
    if 3 * F_ >= MAX_POINTS:
        raise ValueError("vertex_normals: 3 F must stay below 2^31")
    # the vertex -> (face, corner) list (a face naming a vertex outside [0, V) is skipped by the kernel)
    offsets, items = csr(f.clamp(0, V - 1), V)
    call("sgr_mesh_vertex_normals", v.device, V, F_, ptr(v), ptr(f), ptr(offsets), ptr(items), ptr(normals))
    return normals
