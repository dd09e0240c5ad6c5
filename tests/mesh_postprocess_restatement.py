"""A numpy restatement of the refined-mesh postprocess (sugar_extractors/refined_mesh.py:125-187), kept apart from the product
(sugar_amd/mesh_postprocess.py, csrc/mesh_postprocess.hip) and written without reading it: the serial peel with slot counting, the
re-add in float64 over a brute-force 16-NN, the row compaction; and the case meshes the tests share.

The peel rule: face (a, b, c) has three slots carrying the unordered pairs {a,b}, {b,c}, {c,a}; the live count of a pair is the number
of slots of live faces that carry it; in one iteration a live face stays live iff each of its three pairs has live count >= 2, all
counts taken before any face of the iteration is removed."""
from collections import Counter

import numpy as np


# ---------------------------------------------------------------- the peel
def face_pairs(face):
    a, b, c = (int(x) for x in face)
    return [(min(a, b), max(a, b)), (min(b, c), max(b, c)), (min(c, a), max(c, a))]


def peel(faces, iterations, mask=None):
    """bool[F] after `iterations` steps, serial"""
    faces = np.asarray(faces)
    live = np.ones(len(faces), bool) if mask is None else np.array(mask, bool)
    pairs = [face_pairs(f) for f in faces]
    for _ in range(int(iterations)):
        count = Counter()
        for f in range(len(faces)):
            if live[f]:
                for p in pairs[f]:
                    count[p] += 1                       # one per SLOT: (i, j, j) adds 2 to {i,j}
        nxt = live.copy()
        for f in range(len(faces)):
            if live[f]:
                nxt[f] = all(count[p] >= 2 for p in pairs[f])
        live = nxt
    return live


def peel_steps(faces, iterations, mask=None, serial=True):
    """[mask after 0, 1, ..., iterations steps].  serial=False counts with numpy instead of the Python loop -- the same rule (a bincount
    of the live slots' pair ids), for the 150 600-face case; tests/test_mesh_postprocess_cpu.py holds the two against each other."""
    faces = np.asarray(faces)
    live = np.ones(len(faces), bool) if mask is None else np.array(mask, bool)
    out = [live]
    if not serial:
        e = np.stack([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]], axis=1).reshape(-1, 2)
        uniq, pair_id = np.unique(e.min(1) * (int(faces.max()) + 1) + e.max(1), return_inverse=True)
        pair_id = pair_id.reshape(-1)
    for _ in range(int(iterations)):
        if serial:
            live = peel(faces, 1, live)
        else:
            count = np.bincount(pair_id[np.repeat(live, 3)], minlength=len(uniq))
            live = live & (count[pair_id] >= 2).reshape(-1, 3).all(1)
        out.append(live)
    return out


def peel_reference_criterion(faces, iterations, mask=None):
    """the reference's own statement (:133-147), brute force: the float32 tensor of the live faces' sorted pairs, the full matrix of
    squared distances, a slot is 'inside' iff its second-smallest distance is < 0.01, a face stays iff its three slots are"""
    faces = np.asarray(faces)
    e = np.sort(np.stack([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]], axis=1), axis=-1).astype(np.float32)   # [F,3,2]
    live = np.ones(len(faces), bool) if mask is None else np.array(mask, bool)
    for _ in range(int(iterations)):
        p = e[live].reshape(-1, 2)
        if len(p) == 0:
            break
        d = ((p[:, None, :] - p[None, :, :]) ** 2).sum(-1)
        d.sort(axis=1)
        inside = (d[:, 1].reshape(-1, 3) < np.float32(0.01)).all(-1)
        live[np.nonzero(live)[0]] = inside
    return live


# ---------------------------------------------------------------- the re-add
def quaternion_to_matrix(q):
    q = np.asarray(q, np.float64)
    r, i, j, k = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    two_s = 2.0 / (q * q).sum(-1)
    m = np.stack([1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
                  two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r),
                  two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j)], axis=-1)
    return m.reshape(-1, 3, 3)


def face_density(verts, faces, points, scaling, quaternions, strengths, n_closest=16):
    """float64 density (sugar_model.py:1345-1368, density_factor 1) at the centre of EVERY face, over its n_closest nearest Gaussians"""
    verts, points = np.asarray(verts, np.float64), np.asarray(points, np.float64)
    centres = verts[np.asarray(faces)].mean(-2)
    d2 = ((centres[:, None, :] - points[None, :, :]) ** 2).sum(-1)
    nearest = np.argsort(d2, axis=1, kind="stable")[:, :n_closest]
    inv_s = 1.0 / np.maximum(np.asarray(scaling, np.float64), 1e-8)
    B = quaternion_to_matrix(quaternions) * inv_s[:, None, :]                # R * (1 / s)[:, None]: column j scaled by 1 / s_j
    shift = centres[:, None, :] - points[nearest]                            # [F,K,3]
    warped = np.einsum("fkij,fki->fkj", B[nearest], shift)                   # B^T shift
    q = np.clip((warped * warped).sum(-1), 0.0, 1e8)
    st = np.asarray(strengths, np.float64).reshape(-1)
    return (st[nearest] * np.exp(-0.5 * q)).sum(-1)


def readd(mask, density, threshold):
    """dead faces of density > threshold (strictly) come back"""
    out = np.array(mask, bool)
    out[~out] = density[~out] > threshold
    return out


def margin_ok(mask, density, threshold, rel=1e-3):
    """the condition on the inputs: every DEAD face's float64 density lies outside threshold (1 +- rel)"""
    d = density[~np.asarray(mask, bool)]
    return bool(np.all((d < threshold * (1 - rel)) | (d > threshold * (1 + rel))))


# ---------------------------------------------------------------- the compaction
def compact_rows(t, mask, n):
    """rows f n .. f n + n - 1 of every kept face f, in order"""
    t = np.asarray(t)
    keep = [f * n + k for f in range(len(mask)) if mask[f] for k in range(n)]
    return t[np.asarray(keep, np.int64)] if keep else t[:0]


# ---------------------------------------------------------------- the cases
def sheet(nx, ny):
    """2 nx ny faces over (nx + 1)(ny + 1) vertices, vertex (i, j) = j (nx + 1) + i, cell (i, j) split along its diagonal"""
    f = []
    for j in range(ny):
        for i in range(nx):
            a, b, c, d = j * (nx + 1) + i, j * (nx + 1) + i + 1, (j + 1) * (nx + 1) + i + 1, (j + 1) * (nx + 1) + i
            f += [(a, b, c), (a, c, d)]
    return np.array(f, np.int64)


def sheet_fast(nx, ny):
    """`sheet` without the Python loop (the 150 600-face case)"""
    i, j = np.meshgrid(np.arange(nx), np.arange(ny))
    a = (j * (nx + 1) + i).reshape(-1)
    b, c, d = a + 1, a + nx + 2, a + nx + 1
    return np.stack([np.stack([a, b, c], -1), np.stack([a, c, d], -1)], axis=1).reshape(-1, 3).astype(np.int64)


def with_extras(faces):
    """+ a degenerate face (0, 1, 1), a face on sheet vertices 3, 4, 5 twice, an isolated face on three new vertices"""
    v = int(faces.max()) + 1
    return np.concatenate([faces, np.array([[0, 1, 1], [3, 4, 5], [3, 4, 5], [v, v + 1, v + 2]], np.int64)])


def sheet_verts(nx, ny, n_verts, seed, jitter=0.25, z=0.0):
    """vertex (i, j) at (i, j, 0) plus a seeded jitter in the plane (and `z` times a jitter off it); vertices beyond the sheet (the
    isolated face's) sit beside it"""
    g = np.random.default_rng(seed)
    v = np.zeros((n_verts, 3))
    k = np.arange(n_verts)
    v[:, 0], v[:, 1] = k % (nx + 1), k // (nx + 1)
    v[:, :2] += g.uniform(-jitter, jitter, (n_verts, 2))
    v[:, 2] = z * g.uniform(-1, 1, n_verts)
    return v.astype(np.float32)


def octahedron(subdivisions=2):
    """a closed surface: every edge has exactly two faces; 8 * 4^subdivisions faces"""
    verts = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    faces = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    for _ in range(subdivisions):
        mid, nxt = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                mid[key] = len(verts)
                verts.append(tuple((np.array(verts[a]) + np.array(verts[b])) / 2))
            return mid[key]
        for a, b, c in faces:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nxt += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
        faces = nxt
    return np.array(verts, np.float32), np.array(faces, np.int64)


def initial_mask(n_faces, seed=5):
    """a non-trivial initial mask: about a tenth of the faces dead, seeded"""
    return np.random.default_rng(seed).uniform(size=n_faces) > 0.1


def readd_case(seed=11):
    """The re-add case: the 7 x 5 sheet with the extras, vertices jittered in all three directions, peeled 2 iterations; 300 generic
    random Gaussians around it (centres, anisotropic scales, rotations, strengths all random: no two distances tie).  Returns a dict."""
    nx, ny = 7, 5
    faces = with_extras(sheet(nx, ny))
    verts = sheet_verts(nx, ny, int(faces.max()) + 1, seed, z=0.3)
    g = np.random.default_rng(seed + 1)
    P = 300
    points = np.stack([g.uniform(-1, nx + 4, P), g.uniform(-1, ny + 2, P), g.uniform(-0.6, 0.6, P)], -1).astype(np.float32)
    scaling = np.exp(g.uniform(np.log(0.25), np.log(0.9), (P, 3))).astype(np.float32)
    q = g.standard_normal((P, 4))
    quaternions = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    strengths = g.uniform(0.02, 1.0, P).astype(np.float32)
    return dict(verts=verts, faces=faces, points=points, scaling=scaling, quaternions=quaternions, strengths=strengths,
                mask=peel(faces, 2), threshold=0.5)


def bound_case(nx, ny, n, seed):
    """a synthetic refine checkpoint's tensors for an nx x ny sheet (no extras) with n Gaussians per triangle, in the reference's layout:
    jittered planar vertices, a thickness of 0.02 (so that float32 rounding off the plane stays far below the re-add margin), in-plane
    scales of 0.15, random in-plane rotations, densities that are high (logit 3) on the left half of the sheet and low (logit -7) on
    the right, DC colours random"""
    faces = sheet(nx, ny)
    F = len(faces)
    verts = sheet_verts(nx, ny, (nx + 1) * (ny + 1), seed)
    g = np.random.default_rng(seed + 1)
    centre_x = verts[faces].mean(1)[:, 0]
    logit = np.where(centre_x < nx / 2, 3.0, -7.0)
    return {"_points": verts, "_surface_mesh_faces": faces, "surface_mesh_thickness": np.array(0.02, np.float32),
            "_scales": np.full((F * n, 2), np.log(0.15), np.float32) + g.uniform(-0.1, 0.1, (F * n, 2)).astype(np.float32),
            "_quaternions": g.standard_normal((F * n, 2)).astype(np.float32),
            "all_densities": np.repeat(logit, n).reshape(F * n, 1).astype(np.float32),
            "_sh_coordinates_dc": g.uniform(-1.5, 1.5, (F * n, 1, 3)).astype(np.float32),
            "_sh_coordinates_rest": (0.1 * g.standard_normal((F * n, 15, 3))).astype(np.float32)}
