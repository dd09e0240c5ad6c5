"""A serial restatement of csrc/marching_cubes.hip in numpy float32 (test infrastructure): the same rules, the same generated table
(parsed from sugar_amd/csrc/mc_table.h), no GPU.

  * corner inside  <=>  finite and >= iso;
  * the grid point with linear index p = (x ny + y) nz + z owns its +x, +y, +z edges; vertex ids = exclusive scan of the crossed owned
    edges in linear point order, then axis order;
  * vertex on a crossed edge: t = (iso - a) / (b - a) from the OUTSIDE end (a outside, b inside; three float32 operations),
    t = 0.5 when a or t is not finite (b - a alone overflowing gives t = 0, on the outside grid point); coordinate i + t when the lower end is outside, (i + 1) - t otherwise;
  * faces in linear cell order, then table order.

`marching_cubes(volume, iso)` returns (verts[V,3] float32, faces[F,3] int64, aux) with aux = dict(owner[V] linear point index,
axis[V], t[V] float32) for the checks that need the edge a vertex lies on."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE_PATH = os.path.join(ROOT, "sugar_amd", "csrc", "mc_table.h")


def load_table(path=TABLE_PATH):
    """(max_tris, edge_owner[12], ntri[256], tri[256, 3 * max_tris]) parsed from the generated header"""
    src = open(path).read()
    src = re.sub(r"//[^\n]*", "", src)
    max_tris = int(re.search(r"#define\s+MC_MAX_TRIS\s+(\d+)", src).group(1))

    def ints(name):
        body = re.search(name + r"(?:\[[^\]]*\])+\s*=\s*\{(.*?)\};", src, flags=re.S).group(1)
        return np.array([int(v) for v in re.findall(r"-?\d+", body)], dtype=np.int64)
    owner = ints("MC_EDGE_OWNER")
    ntri = ints("MC_NTRI")
    tri = ints("MC_TRI").reshape(256, 3 * max_tris)
    assert owner.shape == (12,) and ntri.shape == (256,)
    return max_tris, owner, ntri, tri


def inside_mask(vol, iso):
    with np.errstate(invalid="ignore"):
        return np.isfinite(vol) & (vol >= np.float32(iso))


def marching_cubes(volume, iso):
    vol = np.ascontiguousarray(volume, dtype=np.float32)
    assert vol.ndim == 3
    nx, ny, nz = vol.shape
    iso = np.float32(iso)
    _, owner_corner, ntri, tri = load_table()
    ins = inside_mask(vol, iso)
    N = nx * ny * nz
    strides = (ny * nz, nz, 1)

    # ---- owned crossed edges
    crossed = np.zeros((3, nx, ny, nz), dtype=bool)
    crossed[0, :-1] = ins[:-1] != ins[1:]
    crossed[1, :, :-1] = ins[:, :-1] != ins[:, 1:]
    crossed[2, :, :, :-1] = ins[:, :, :-1] != ins[:, :, 1:]
    c = crossed.reshape(3, N)
    per_point = c.sum(axis=0).astype(np.int64)
    base = np.cumsum(per_point) - per_point                       # exclusive scan in linear point order
    vid = np.stack([base, base + c[0], base + c[0] + c[1]])       # id of the +axis vertex of every point (where crossed)
    V = int(per_point.sum())

    # ---- vertices
    verts = np.zeros((V, 3), dtype=np.float32)
    owner = np.zeros(V, dtype=np.int64)
    axis_of = np.zeros(V, dtype=np.int64)
    t_of = np.zeros(V, dtype=np.float32)
    flat = vol.reshape(N)
    fins = ins.reshape(N)
    for a in range(3):
        p = np.nonzero(c[a])[0]
        q = p + strides[a]
        lo_in = fins[p]
        va, vb = flat[p], flat[q]
        out_v = np.where(lo_in, vb, va)
        in_v = np.where(lo_in, va, vb)
        with np.errstate(all="ignore"):
            t = ((iso - out_v) / (in_v - out_v)).astype(np.float32)
        t = np.where(np.isfinite(out_v) & np.isfinite(t), t, np.float32(0.5)).astype(np.float32)
        coords = np.stack([p // (ny * nz), (p // nz) % ny, p % nz], axis=1).astype(np.float32)
        i = coords[:, a]
        coords[:, a] = np.where(lo_in, (i + np.float32(1.0)) - t, i + t).astype(np.float32)
        ids = vid[a][p]
        verts[ids] = coords
        owner[ids], axis_of[ids], t_of[ids] = p, a, t

    # ---- faces
    faces = np.zeros((0, 3), dtype=np.int64)
    if nx > 1 and ny > 1 and nz > 1:
        case = np.zeros((nx - 1, ny - 1, nz - 1), dtype=np.int64)
        for corner in range(8):
            dx, dy, dz = corner & 1, (corner >> 1) & 1, (corner >> 2) & 1
            case |= ins[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz].astype(np.int64) << corner
        full = np.zeros((nx, ny, nz), dtype=np.int64)
        full[:-1, :-1, :-1] = case
        full = full.reshape(N)
        cells = np.nonzero(ntri[full] > 0)[0]                     # linear cell order
        if cells.size:
            rows = tri[full[cells]]                               # [n_cells, 3 * max_tris], -1 padded
            cell_of = np.repeat(cells, rows.shape[1]).reshape(rows.shape)
            keep = rows >= 0
            e = rows[keep]
            pcell = cell_of[keep]
            oc = owner_corner[e]
            q = pcell + (oc & 1) * strides[0] + ((oc >> 1) & 1) * strides[1] + ((oc >> 2) & 1) * strides[2]
            ax = e // 4
            assert c[ax, q].all(), "the table uses an edge that is not crossed"
            faces = vid[ax, q].reshape(-1, 3).astype(np.int64)
    return verts, faces, dict(owner=owner, axis=axis_of, t=t_of)


# ---- mesh checks shared by the CPU and GPU tests
def directed_edges(faces):
    f = np.asarray(faces, dtype=np.int64)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])


def edge_report(faces, n_verts):
    """(closed, boundary): closed = every undirected edge is used by exactly two faces, once in each direction;
    boundary = the directed edges [n,2] whose reverse is absent"""
    e = directed_edges(faces)
    key = e[:, 0] * n_verts + e[:, 1]
    rkey = e[:, 1] * n_verts + e[:, 0]
    uniq, counts = np.unique(key, return_counts=True)
    no_repeat = bool((counts == 1).all())
    has_reverse = np.isin(rkey, uniq)
    return no_repeat and bool(has_reverse.all()), e[~has_reverse], no_repeat


def euler_characteristic(faces, n_verts):
    e = directed_edges(faces)
    und = np.unique(np.minimum(e[:, 0], e[:, 1]) * n_verts + np.maximum(e[:, 0], e[:, 1]))
    used = np.unique(np.asarray(faces).reshape(-1))
    return int(used.size) - int(und.size) + int(np.asarray(faces).shape[0])


def signed_volume_and_area(verts, faces):
    v = np.asarray(verts, dtype=np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    vol = float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)
    area = float(np.linalg.norm(np.cross(b - a, c - a), axis=1).sum() / 2.0)
    return vol, area
