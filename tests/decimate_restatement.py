"""A serial restatement of csrc/mesh_decimate.hip and sugar_amd/decimate.py in numpy float64 (test infrastructure, no GPU): the same
rules in the same operation order, every product and sum written out so that each is rounded on its own (no dot / einsum / sum).  The
rules are stated at the top of the kernel file; the function names here follow its sections.

  decimate(verts, faces, target, boundary_weight=1.0) -> (verts float32, faces int64, info)
  clean(verts, faces, degenerate=True, duplicated_triangles=True, duplicated_vertices=True, non_manifold_edges=True)
      -> (verts float32, faces int64, vertex_map int64)"""
import numpy as np

KEY_INVALID = np.int64(2 ** 63 - 1)
DET_REL = 1e-12
CAND_DIV = 4
PASSES = 4


def round_limit(n_faces, target):
    t, k = max(int(target), 1), 0
    while (t << k) < int(n_faces):
        k += 1
    return 8 * k + 32


# ---------------------------------------------------------------------------------------------------------------------- small algebra
def _cross(u, w):
    return np.stack([u[..., 1] * w[..., 2] - u[..., 2] * w[..., 1], u[..., 2] * w[..., 0] - u[..., 0] * w[..., 2],
                     u[..., 0] * w[..., 1] - u[..., 1] * w[..., 0]], axis=-1)


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _plane_quadric(w, a, b, c, d):
    wa, wb, wc, wd = w * a, w * b, w * c, w * d
    return np.stack([wa * a, wa * b, wa * c, wa * d, wb * b, wb * c, wb * d, wc * c, wc * d, wd * d], axis=-1)


def _cost(q, x, y, z):
    return (x * (q[..., 0] * x + q[..., 1] * y + q[..., 2] * z + q[..., 3]) + y * (q[..., 1] * x + q[..., 4] * y + q[..., 5] * z + q[..., 6]) +
            z * (q[..., 2] * x + q[..., 5] * y + q[..., 7] * z + q[..., 8]) + (q[..., 3] * x + q[..., 6] * y + q[..., 8] * z + q[..., 9]))


# ---------------------------------------------------------------------------------------------------------------------- topology
def sorted_incidences(faces, V):
    f = np.asarray(faces, dtype=np.int64)
    e0 = np.stack([f[:, 1], f[:, 2], f[:, 0]], axis=1).reshape(-1)
    e1 = np.stack([f[:, 2], f[:, 0], f[:, 1]], axis=1).reshape(-1)
    key = np.minimum(e0, e1) * V + np.maximum(e0, e1)
    order = np.argsort(key, kind="stable")
    return key[order], order


class Edges:
    def __init__(self, faces, V):
        skey, order = sorted_incidences(faces, V)
        n = len(skey)
        new = np.ones(n, dtype=bool)
        new[1:] = skey[1:] != skey[:-1]
        first = np.nonzero(new)[0]
        count = np.diff(np.append(first, n))
        self.keys = skey[first]                                  # sorted, distinct
        self.lo, self.hi = self.keys // V, self.keys % V
        self.nf = np.minimum(count, 3)
        self.count = count
        self.f0 = order[first] // 3
        second = np.minimum(first + 1, n - 1)
        self.f1 = np.where(count >= 2, order[second] // 3, -1)
        self.bflag = np.zeros(n, dtype=bool)
        self.bflag[order[first[count == 1]]] = True
        self.vbnd = np.zeros(V, dtype=bool)
        self.vbnd[self.lo[count == 1]] = True
        self.vbnd[self.hi[count == 1]] = True
        self.V = V

    def adjacent(self, a, b):
        """whether the vertices a and b share a face (elementwise)"""
        k = np.minimum(a, b) * self.V + np.maximum(a, b)
        pos = np.minimum(np.searchsorted(self.keys, k), len(self.keys) - 1)
        return self.keys[pos] == k


def vertex_csr(faces, V):
    flat = np.asarray(faces, dtype=np.int64).reshape(-1)
    items = np.argsort(flat, kind="stable")
    offsets = np.searchsorted(flat[items], np.arange(V + 1))
    return offsets, items


def _padded_items(offsets, items, verts_of):
    """items of the vertices `verts_of` as [n, D] with a validity mask"""
    start, cnt = offsets[verts_of], offsets[verts_of + 1] - offsets[verts_of]
    D = int(cnt.max()) if len(cnt) else 0
    col = np.arange(D)[None, :]
    mask = col < cnt[:, None]
    idx = np.where(mask, start[:, None] + col, 0)
    return items[idx], mask


# ---------------------------------------------------------------------------------------------------------------------- quadrics
def vertex_quadrics(P, faces, bflag, bw):
    F_ = len(faces)
    p = [P[faces[:, k]] for k in range(3)]
    n = _cross(p[1] - p[0], p[2] - p[0])
    ln = np.sqrt(_dot(n, n))
    ok = ln > 0.0
    with np.errstate(all="ignore"):
        nn = n / ln[:, None]
        d = -(nn[:, 0] * p[0][:, 0] + nn[:, 1] * p[0][:, 1] + nn[:, 2] * p[0][:, 2])
        w = 0.5 * ln
        K = _plane_quadric(w, nn[:, 0], nn[:, 1], nn[:, 2], d)
        B, okb = [], []
        for k in range(3):
            ps, pe = p[(k + 1) % 3], p[(k + 2) % 3]
            m = _cross(pe - ps, nn)
            ml = np.sqrt(_dot(m, m))
            a, b, c = m[:, 0] / ml, m[:, 1] / ml, m[:, 2] / ml
            dd = -(a * ps[:, 0] + b * ps[:, 1] + c * ps[:, 2])
            B.append(_plane_quadric(bw * w, a, b, c, dd))
            okb.append(ok & (ml > 0.0) & bflag.reshape(F_, 3)[:, k])
    # the terms of item (f, c) in order: K(f), then B(f, k) for the k != c, ascending
    contrib = np.zeros((F_, 3, 3, 10))
    mask = np.zeros((F_, 3, 3), dtype=bool)
    for c in range(3):
        contrib[:, c, 0], mask[:, c, 0] = K, ok
        for slot, k in enumerate([k for k in range(3) if k != c], start=1):
            contrib[:, c, slot], mask[:, c, slot] = B[k], okb[k]
    target = np.repeat(np.asarray(faces, dtype=np.int64)[:, :, None], 3, axis=2)
    Q = np.zeros((len(P), 10))
    np.add.at(Q, target[mask], contrib[mask])                   # unbuffered, in index order: ascending (face, corner, term)
    return Q


# ---------------------------------------------------------------------------------------------------------------------- edge evaluation
def _opposite(faces, f, lo, hi):
    fv = faces[np.maximum(f, 0)]
    out = np.full(len(f), -1, dtype=np.int64)
    for k in (2, 1, 0):
        v = fv[:, k]
        out = np.where((v != lo) & (v != hi), v, out)
    return np.where(f >= 0, out, -1)


def _check_end(s, t, oa, ob, nb, P, faces, offsets, items, ed):
    """(ok, has) per edge for the end s"""
    it, valid = _padded_items(offsets, items, s)
    f, c = it // 3, it % 3
    fv = faces[f]
    dying = (fv == t[:, None, None]).any(axis=2)
    surv = valid & ~dying
    w1 = np.take_along_axis(fv, ((c + 1) % 3)[..., None], axis=2)[..., 0]
    w2 = np.take_along_axis(fv, ((c + 2) % 3)[..., None], axis=2)[..., 0]
    A, B = oa[:, None], ob[:, None]
    has = (surv & (B >= 0) & (((w1 == A) & (w2 == B)) | ((w1 == B) & (w2 == A)))).any(axis=1)
    bad = np.zeros(len(s), dtype=bool)
    for w in (w1, w2):
        bad |= (surv & (w != A) & (w != B) & ed.adjacent(w, np.broadcast_to(t[:, None], w.shape))).any(axis=1)
    ps = P[s][:, None, :]
    p1, p2 = P[w1], P[w2]
    n_old = _cross(p1 - ps, p2 - ps)
    n_new = _cross(p1 - nb[:, None, :], p2 - nb[:, None, :])
    with np.errstate(invalid="ignore"):
        bad |= (surv & ~(_dot(n_old, n_new) > 0.0)).any(axis=1)
    return ~bad, has


def edge_eval(P, Q, faces, offsets, items, ed, chunk=100000):
    """(key int64[E], pos[E,3])"""
    E = len(ed.lo)
    key = np.full(E, KEY_INVALID, dtype=np.int64)
    pos = np.zeros((E, 3))
    lo, hi, nf = ed.lo, ed.hi, ed.nf
    oa = _opposite(faces, ed.f0, lo, hi)
    ob = np.where(nf == 2, _opposite(faces, ed.f1, lo, hi), -1)
    pre = (nf <= 2) & (lo != hi) & (oa >= 0) & ~((nf == 2) & ((ob < 0) | (oa == ob))) & ~((nf == 2) & ed.vbnd[lo] & ed.vbnd[hi])
    idx = np.nonzero(pre)[0]
    for i0 in range(0, len(idx), chunk):
        e = idx[i0:i0 + chunk]
        l, h = lo[e], hi[e]
        q = Q[l] + Q[h]
        pl, ph = P[l], P[h]
        mid = 0.5 * (pl + ph)
        q0, q1, q2, q3, q4, q5, q6, q7, q8 = (q[:, k] for k in range(9))
        c00, c01, c02 = q4 * q7 - q5 * q5, q2 * q5 - q1 * q7, q1 * q5 - q2 * q4
        c11, c12, c22 = q0 * q7 - q2 * q2, q1 * q2 - q0 * q5, q0 * q4 - q1 * q1
        det = q0 * c00 + q1 * c01 + q2 * c02
        tr = q0 + q4 + q7
        with np.errstate(all="ignore"):
            big = np.abs(det) > DET_REL * tr * tr * tr
            sol = np.stack([-((c00 * q3 + c01 * q6 + c02 * q8) / det), -((c01 * q3 + c11 * q6 + c12 * q8) / det),
                            -((c02 * q3 + c12 * q6 + c22 * q8) / det)], axis=1)
            dm, de = sol - mid, ph - pl
            solved = big & (_dot(dm, dm) <= _dot(de, de))
            cost_s = _cost(q, sol[:, 0], sol[:, 1], sol[:, 2])
            nb, cost = pl.copy(), _cost(q, pl[:, 0], pl[:, 1], pl[:, 2])
            for cand in (ph, mid):
                cc = _cost(q, cand[:, 0], cand[:, 1], cand[:, 2])
                better = cc < cost
                cost = np.where(better, cc, cost)
                nb = np.where(better[:, None], cand, nb)
            nb = np.where(solved[:, None], sol, nb)
            cost = np.where(solved, cost_s, cost)
        ok = np.isfinite(cost)
        nb = np.where(ok[:, None], nb, 0.0)
        ok_lo, has_lo = _check_end(l, h, oa[e], ob[e], nb, P, faces, offsets, items, ed)
        ok_hi, has_hi = _check_end(h, l, oa[e], ob[e], nb, P, faces, offsets, items, ed)
        ok &= ok_lo & ok_hi & ~(has_lo & has_hi)
        bits = cost.view(np.int64).copy()
        bits = np.where(bits < 0, bits ^ np.int64(0x7FFFFFFFFFFFFFFF), bits)
        key[e] = np.where(ok, bits, KEY_INVALID)
        pos[e] = nb
    return key, pos


# ---------------------------------------------------------------------------------------------------------------------- one round
def _claimed_vertices(cand, ed, faces, offsets, items):
    """[n, W] the vertices of every face at lo and at hi of the candidate edges, with a mask"""
    parts, masks = [], []
    for s in (ed.lo[cand], ed.hi[cand]):
        it, valid = _padded_items(offsets, items, s)
        fv = faces[it // 3]
        parts.append(fv.reshape(len(cand), -1))
        masks.append(np.repeat(valid, 3, axis=1))
    return np.concatenate(parts, axis=1), np.concatenate(masks, axis=1)


def one_round(P, Q, faces, target):
    V, F_ = len(P), len(faces)
    ed = Edges(faces, V)
    offsets, items = vertex_csr(faces, V)
    key, pos = edge_eval(P, Q, faces, offsets, items, ed)
    order = np.argsort(key, kind="stable")
    n_valid = int((key != KEY_INVALID).sum())
    n_cand = (n_valid + CAND_DIV - 1) // CAND_DIV
    if n_cand == 0:
        return P, Q, faces, 0
    cand = order[:n_cand]
    W, mask = _claimed_vertices(cand, ed, faces, offsets, items)
    rank = np.broadcast_to(np.arange(n_cand, dtype=np.int64)[:, None], W.shape)
    win = np.zeros(n_cand, dtype=np.int64)
    dead = np.zeros(n_cand, dtype=bool)
    lock = np.zeros(V, dtype=bool)
    for _ in range(PASSES):
        live = (win == 0) & ~dead
        dead |= live & (lock[W] & mask).any(axis=1)             # a vertex of it belongs to an earlier pass's winner
        live &= ~dead
        claim = np.full(V, KEY_INVALID, dtype=np.int64)
        m = mask & live[:, None]
        np.minimum.at(claim, W[m], rank[m])
        holds = live & ((claim[W] == rank) | ~mask).all(axis=1)
        win = np.where(holds, ed.nf[cand], win)
        lock[W[mask & holds[:, None]]] = True
    before = np.cumsum(win) - win
    keep = (win > 0) & ((F_ - before) > target)
    e = cand[keep]
    u, v = ed.lo[e], ed.hi[e]
    P, Q = P.copy(), Q.copy()
    P[u] = pos[e]
    Q[u] = Q[u] + Q[v]
    rename = np.arange(V, dtype=np.int64)
    rename[v] = u
    vkeep = np.ones(V, dtype=bool)
    vkeep[v] = False
    faces = rename[faces]
    fkeep = (faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 0] != faces[:, 2])
    vpos = np.cumsum(vkeep) - 1
    return P[vkeep], Q[vkeep], vpos[faces[fkeep]], int(keep.sum())


def decimate(verts, faces, target, boundary_weight=1.0):
    v32 = np.ascontiguousarray(verts, dtype=np.float32)
    f = np.ascontiguousarray(faces, dtype=np.int64)
    target = int(target)
    V, F_ = len(v32), len(f)
    limit = round_limit(F_, target)
    info = dict(rounds=0, faces=F_, target=target, target_met=F_ <= target, round_limit=limit)
    if F_ <= target or F_ == 0 or V == 0:
        return v32, f, info
    centre = 0.5 * (v32.min(axis=0).astype(np.float64) + v32.max(axis=0).astype(np.float64))
    P = v32.astype(np.float64) - centre
    Q = vertex_quadrics(P, f, Edges(f, V).bflag, float(boundary_weight))
    rounds = 0
    while len(f) > target and rounds < limit:
        P, Q, f, n = one_round(P, Q, f, target)
        rounds += 1
        if n == 0 or len(f) == 0:
            break
    info.update(rounds=rounds, faces=len(f), target_met=len(f) <= target)
    return (P + centre).astype(np.float32), f, info


# ---------------------------------------------------------------------------------------------------------------------- cleaning
def clean(verts, faces, degenerate=True, duplicated_triangles=True, duplicated_vertices=True, non_manifold_edges=True):
    v = np.ascontiguousarray(verts, dtype=np.float32)
    f = np.ascontiguousarray(faces, dtype=np.int64).reshape(-1, 3)
    V = len(v)
    vmap = np.arange(V, dtype=np.int64)
    if degenerate and len(f):
        f = f[(f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])]
    if duplicated_triangles and len(f):
        seen, keep = set(), np.ones(len(f), dtype=bool)
        for i, t in enumerate(map(tuple, np.sort(f, axis=1))):
            keep[i] = t not in seen                             # the lowest face id of a vertex set survives
            seen.add(t)
        f = f[keep]
    if duplicated_vertices and V:
        first = {}
        for i, b in enumerate(map(bytes, v)):                   # bit-equal coordinates: the lowest id survives
            vmap[i] = first.setdefault(b, i)
        f = vmap[f]
    while non_manifold_edges and len(f) and V:
        skey, order = sorted_incidences(f, V)
        new = np.ones(len(skey), dtype=bool)
        new[1:] = skey[1:] != skey[:-1]
        first = np.nonzero(new)[0]
        count = np.diff(np.append(first, len(skey)))
        p = v.astype(np.float64)
        n = _cross(p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]])
        a2 = _dot(n, n)
        remove = np.zeros(len(f), dtype=bool)
        for i, c in zip(first[count > 2], count[count > 2]):    # every edge with more than two faces removes its smallest face
            fs = order[i:i + c] // 3
            best = min(fs, key=lambda g: (a2[g], -g))           # ties: the highest face id
            remove[best] = True
        if not remove.any():
            break
        f = f[~remove]
    if V == 0 or len(f) == 0:
        return v[:0], np.zeros((0, 3), np.int64), np.full(V, -1, dtype=np.int64)
    ref = np.zeros(V, dtype=bool)
    ref[f.reshape(-1)] = True
    new_id = np.where(ref, np.cumsum(ref) - 1, -1)
    return v[ref], new_id[f], new_id[vmap]
