#!/usr/bin/env python
"""Generate sugar_amd/csrc/mc_table.h: the 256-case triangle table of csrc/marching_cubes.hip.

Nothing here is typed in from a published table; the cases are constructed:

  corners  c = dx + 2 dy + 4 dz (bit a of c = the corner's offset along axis a; x = axis 0), bit c of the case = corner c is inside;
  edges    e = 4 axis + j: the cell edge along `axis` whose lower corner has the two other offsets (u, v), j = u + 2 v, with (u, v)
           the offsets along the two remaining axes in ascending axis order.  The lower corner is the grid point that owns the edge.

  1. On each of the six cell faces the boundary segments follow from that face's four corner signs ALONE: two crossed edges give one
     segment; four crossed edges (inside corners on one diagonal, the ambiguous face) give two segments, each cutting off ONE INSIDE
     corner -- the fixed ambiguity rule: inside corners are never joined across an ambiguous face.  Two cells sharing a face see the
     same four signs, hence the same segments: the surface is closed.
  2. A segment A -> B on a face with outward normal n is directed along N x n, N pointing from the inside corners it cuts off to the
     outside: with that direction every loop runs counter-clockwise seen from the outside (lower values).
  3. Every crossed edge ends one segment and starts another; following them closes the loops.
  4. Each loop is fan-triangulated.  The apex is the first loop position for which the fewest fan diagonals lie in a cell face (a
     diagonal between two edges of one face would lie on an ambiguous face and could coincide with the neighbour cell's).

    python scripts/gen_mc_table.py            # rewrites sugar_amd/csrc/mc_table.h
    python scripts/gen_mc_table.py --check    # exit 1 if the committed header differs
"""
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "sugar_amd", "csrc", "mc_table.h")


def corner_offset(c):
    return (c & 1, (c >> 1) & 1, (c >> 2) & 1)


def corner_id(off):
    return off[0] + 2 * off[1] + 4 * off[2]


def edge_corners(e):
    """(lower corner, upper corner) of cell edge e"""
    axis, j = divmod(e, 4)
    others = [a for a in range(3) if a != axis]
    off = [0, 0, 0]
    off[others[0]] = j & 1
    off[others[1]] = j >> 1
    lo = corner_id(off)
    off[axis] = 1
    return lo, corner_id(off)


EDGE_OF = {frozenset(edge_corners(e)): e for e in range(12)}


def faces():
    """the six faces: (outward normal, the four corners in cyclic order)"""
    out = []
    for axis in range(3):
        u, v = [a for a in range(3) if a != axis]
        for side in (0, 1):
            cyc = []
            for (a, b) in ((0, 0), (1, 0), (1, 1), (0, 1)):
                off = [0, 0, 0]
                off[axis] = side
                off[u], off[v] = a, b
                cyc.append(corner_id(off))
            n = [0, 0, 0]
            n[axis] = 1 if side else -1
            out.append((tuple(n), cyc))
    return out


FACES = faces()


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def dot(a, b):
    return sum(x * y for x, y in zip(a, b))


def midpoint(e):
    lo, hi = edge_corners(e)
    a, b = corner_offset(lo), corner_offset(hi)
    return tuple((x + y) / 2 for x, y in zip(a, b))


def face_segments(case, normal, cyc):
    """directed segments (edge_from, edge_to) on one face; depends on the signs of the face's four corners only"""
    inside = [(case >> c) & 1 for c in cyc]
    crossed = [k for k in range(4) if inside[k] != inside[(k + 1) % 4]]       # side k joins cyc[k] and cyc[k+1]
    if not crossed:
        return []
    side_edge = lambda k: EDGE_OF[frozenset((cyc[k], cyc[(k + 1) % 4]))]
    if len(crossed) == 2:
        pairs = [(crossed[0], crossed[1])]
    else:
        # ambiguous: cut off every inside corner on its own (sides k-1 and k meet at corner cyc[k])
        pairs = [((k - 1) % 4, k) for k in range(4) if inside[k]]
    out = []
    for ka, kb in pairs:
        ea, eb = side_edge(ka), side_edge(kb)
        ins = []
        for k in (ka, kb):
            ins.append(corner_offset(cyc[k] if inside[k] else cyc[(k + 1) % 4]))
        centre_in = tuple((x + y) / 2 for x, y in zip(*ins))
        A, B = midpoint(ea), midpoint(eb)
        mid = tuple((x + y) / 2 for x, y in zip(A, B))
        N = tuple(m - c for m, c in zip(mid, centre_in))
        d = cross(N, normal)
        s = dot(tuple(b - a for a, b in zip(A, B)), d)
        assert s != 0
        out.append((ea, eb) if s > 0 else (eb, ea))
    return out


def share_face(e1, e2):
    c = set(edge_corners(e1)) | set(edge_corners(e2))
    return any(c <= set(cyc) for _, cyc in FACES)


def case_triangles(case):
    nxt = {}
    for normal, cyc in FACES:
        for a, b in face_segments(case, normal, cyc):
            assert a not in nxt, "an edge starts two segments"
            nxt[a] = b
    assert sorted(nxt) == sorted(set(nxt.values()))
    loops, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop, e = [], start
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = nxt[e]
        assert e == start
        loops.append(loop)
    tris, in_face = [], 0
    for loop in loops:
        n = len(loop)
        best = None
        for r in range(n):
            rot = loop[r:] + loop[:r]
            bad = sum(share_face(rot[0], rot[i]) for i in range(2, n - 1))
            if best is None or bad < best[0]:
                best = (bad, rot)
        in_face += best[0]
        rot = best[1]
        for i in range(1, n - 1):
            tris.append((rot[0], rot[i], rot[i + 1]))
    return tris, in_face


def generate():
    table = [case_triangles(c) for c in range(256)]
    max_tris = max(len(t) for t, _ in table)
    in_face = sum(b for _, b in table)
    lines = [
        "// mc_table.h -- GENERATED by scripts/gen_mc_table.py; do not edit (tests/test_marching_cubes_cpu.py checks it against the generator).",
        "// Corner c = dx + 2 dy + 4 dz, case bit c = corner c inside; cell edge e = 4 axis + j, owned by the cell corner with the offsets",
        "// MC_EDGE_OWNER[e] (a corner id).  MC_TRI[case]: MC_NTRI[case] triangles of three cell edges each, -1 padded, wound",
        "// counter-clockwise seen from the outside (lower values).  Ambiguous faces never join inside corners.",
        f"// Fan diagonals lying in a cell face, over all cases: {in_face}.",
        "#pragma once",
        "#ifndef MC_TABLE_QUAL  /* csrc/marching_cubes.hip places the tables in device memory */",
        "#define MC_TABLE_QUAL static const",
        "#endif",
        f"#define MC_MAX_TRIS {max_tris}",
        "MC_TABLE_QUAL unsigned char MC_EDGE_OWNER[12] = {" + ", ".join(str(edge_corners(e)[0]) for e in range(12)) + "};",
        "MC_TABLE_QUAL unsigned char MC_NTRI[256] = {",
    ]
    for r in range(0, 256, 32):
        lines.append("    " + ", ".join(str(len(table[c][0])) for c in range(r, r + 32)) + ",")
    lines.append("};")
    lines.append("MC_TABLE_QUAL signed char MC_TRI[256][3 * MC_MAX_TRIS] = {")
    for c in range(256):
        flat = list(itertools.chain.from_iterable(table[c][0]))
        flat += [-1] * (3 * max_tris - len(flat))
        lines.append("    {" + ", ".join("%2d" % v for v in flat) + "},")
    lines.append("};")
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    text = generate()
    if "--check" in sys.argv:
        sys.exit(0 if open(OUT).read() == text else 1)
    with open(OUT, "w") as f:
        f.write(text)
    print("wrote", OUT)
