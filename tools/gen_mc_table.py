"""Generate esr_nerf_amd/csrc/mc_table.h, the marching-cubes case table of esr_nerf_amd/csrc/mesh.hip.

    python tools/gen_mc_table.py            write the header
    python tools/gen_mc_table.py --check    exit 1 if the committed header differs from what this script writes

No table is typed in: every one of the 256 cases is derived from a rule on the cube's six faces.

Cube conventions (shared with mesh.hip and tests/mesh_ref.py):
  corner (dx, dy, dz) is bit dx | dy << 1 | dz << 2 of the case index; a set bit is an INSIDE corner (u > threshold).
  edge id = 4 * axis + (b0 | b1 << 1): the edge along `axis` whose two other coordinates, in increasing axis order, are
  b0 and b1.  Its owner corner (the one with coordinate 0 along `axis`) owns the edge's vertex in the lattice numbering.

Face rule.  A face with one, two adjacent or three inside corners gets the single segment that joins its two crossed
edges.  A face with two diagonal inside corners (the ambiguous face) gets two segments, each cutting off one inside
corner, so the inside corners stay separated.  The decision reads only the face's own four corner flags, so two cells
that share a face produce the same segments.  A segment p -> q on a face with outward normal N is directed so that the
inside corners on its side satisfy ((q - p) x (c - p)) . N < 0; the neighbouring cell sees the face with the opposite
normal and so traverses the segment q -> p.  Every crossed edge lies on exactly two faces, so the segments chain into
closed loops.  Each loop is fan-triangulated from a start vertex chosen so that no fan diagonal joins two vertices of
one face (such a diagonal could coincide with the neighbouring cell's).  With this direction each triangle (a, b, c)
has (b - a) x (c - a) pointing from the inside to the outside, i.e. towards decreasing u.
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "esr_nerf_amd", "csrc", "mc_table.h")


def corner_bit(c):
    return c[0] | c[1] << 1 | c[2] << 2


def edge_id(axis, c):
    """id of the edge along `axis` through corner c (c[axis] is ignored)."""
    o = [c[b] for b in range(3) if b != axis]
    return 4 * axis + (o[0] | o[1] << 1)


def edge_corners(e):
    """(owner corner, other corner) of edge e."""
    axis, b0, b1 = e >> 2, e & 1, (e >> 1) & 1
    c = [0, 0, 0]
    others = [b for b in range(3) if b != axis]
    c[others[0]], c[others[1]] = b0, b1
    c1 = list(c)
    c1[axis] = 1
    return tuple(c), tuple(c1)


def edge_mid(e):
    a, b = edge_corners(e)
    return (np.array(a, float) + np.array(b, float)) / 2


def faces():
    """(axis, side, outward normal, corners in cyclic order) of the six faces."""
    out = []
    for axis in range(3):
        u, v = [b for b in range(3) if b != axis]
        for side in (0, 1):
            cyc = []
            for pu, pv in ((0, 0), (1, 0), (1, 1), (0, 1)):
                c = [0, 0, 0]
                c[axis], c[u], c[v] = side, pu, pv
                cyc.append(tuple(c))
            n = np.zeros(3)
            n[axis] = 1.0 if side else -1.0
            out.append((axis, side, n, cyc))
    return out


FACES = faces()


def edge_between(c0, c1):
    axis = [a for a in range(3) if c0[a] != c1[a]]
    assert len(axis) == 1
    return edge_id(axis[0], c0)


def face_edges(e):
    """indices into FACES of the two faces that contain edge e."""
    a, b = edge_corners(e)
    return [f for f, (_, _, _, cyc) in enumerate(FACES) if a in cyc and b in cyc]


def orient(p, q, c, n):
    """(p, q) directed so that corner c (on the segment's inside side) satisfies ((q - p) x (c - p)) . n < 0."""
    P, Q = edge_mid(p), edge_mid(q)
    s = float(np.dot(np.cross(Q - P, np.array(c, float) - P), n))
    assert s != 0.0
    return (p, q) if s < 0 else (q, p)


def face_segments(case, f):
    """Directed segments (edge id pairs) the face rule gives face f under `case`."""
    _, _, n, cyc = FACES[f]
    ins = [bool(case >> corner_bit(c) & 1) for c in cyc]
    k = sum(ins)
    if k in (0, 4):
        return []
    crossed = [i for i in range(4) if ins[i] != ins[(i + 1) % 4]]           # cyclic edge i joins corners i, i+1
    eids = [edge_between(cyc[i], cyc[(i + 1) % 4]) for i in crossed]
    if len(crossed) == 2:
        c = cyc[ins.index(True)]
        return [orient(eids[0], eids[1], c, n)]
    # ambiguous face: two diagonal inside corners, each cut off by its own segment
    segs = []
    for i in range(4):
        if ins[i]:
            e_prev = edge_between(cyc[(i - 1) % 4], cyc[i])
            e_next = edge_between(cyc[i], cyc[(i + 1) % 4])
            segs.append(orient(e_prev, e_next, cyc[i], n))
    return segs


def case_segments(case):
    return [s for f in range(6) for s in face_segments(case, f)]


def crossed_edges(case):
    out = []
    for e in range(12):
        a, b = edge_corners(e)
        if (case >> corner_bit(a) & 1) != (case >> corner_bit(b) & 1):
            out.append(e)
    return out


def loops(case):
    nxt = {}
    for p, q in case_segments(case):
        assert p not in nxt, (case, p)                                      # out-degree 1
        nxt[p] = q
    assert sorted(nxt.values()) == sorted(nxt) == crossed_edges(case), case  # in-degree 1, every crossed edge
    out, seen = [], set()
    for e in sorted(nxt):
        if e in seen:
            continue
        loop = [e]
        seen.add(e)
        while nxt[loop[-1]] != e:
            loop.append(nxt[loop[-1]])
            seen.add(loop[-1])
        out.append(loop)
    return out


def share_face(a, b):
    return bool(set(face_edges(a)) & set(face_edges(b)))


def fan(loop):
    """Fan triangles of one loop, started at the first vertex whose diagonals join no two vertices of one face."""
    k = len(loop)
    for s in range(k):
        rot = loop[s:] + loop[:s]
        if not any(share_face(rot[0], rot[i]) for i in range(2, k - 1)):
            return [(rot[0], rot[i], rot[i + 1]) for i in range(1, k - 1)]
    raise AssertionError(f"no clean fan start for loop {loop}")


def case_triangles(case):
    tris = [t for lp in loops(case) for t in fan(lp)]
    for a, b, c in tris:                    # orientation: from the inside to the outside (edge midpoints)
        nrm = np.cross(edge_mid(b) - edge_mid(a), edge_mid(c) - edge_mid(a))
        out = 0.0
        for e in (a, b, c):
            c0, c1 = edge_corners(e)
            d = np.array(c1, float) - np.array(c0, float)
            out += float(np.dot(nrm, d if case >> corner_bit(c0) & 1 else -d))
        assert out > 0, (case, (a, b, c))
    return tris


def table():
    return [case_triangles(c) for c in range(256)]


MAX_TRIS = 5     # asserted below: the largest triangle count of a case under this face rule


def render() -> str:
    tab = table()
    mt = max(len(t) for t in tab)
    assert mt == MAX_TRIS, mt
    row = 3 * MAX_TRIS + 1
    lines = [
        "// Generated by tools/gen_mc_table.py -- do not edit; rerun the generator.",
        "// Marching-cubes case table of mesh.hip.  Case bit (dx | dy << 1 | dz << 2) = corner (dx, dy, dz) is inside (u > thr).",
        "// Edge id = 4 * axis + (b0 | b1 << 1), b0 / b1 = the edge's other two coordinates in increasing axis order.",
        "// ESR_MC_TRI[case]: edge ids, three per triangle, -1 terminated; (b - a) x (c - a) points from inside to outside.",
        "#pragma once",
        "#include <stdint.h>",
        "",
        "#if defined(__HIPCC__)",
        "#define ESR_MC_STORAGE static __constant__",
        "#else",
        "#define ESR_MC_STORAGE static const",
        "#endif",
        "",
        f"#define ESR_MC_MAX_TRIS {MAX_TRIS}",
        f"#define ESR_MC_ROW {row}",
        "",
        "ESR_MC_STORAGE int8_t ESR_MC_NTRI[256] = {",
    ]
    for i in range(0, 256, 32):
        lines.append("    " + ", ".join(str(len(t)) for t in tab[i:i + 32]) + ",")
    lines += ["};", "", "ESR_MC_STORAGE int8_t ESR_MC_TRI[256][ESR_MC_ROW] = {"]
    for c, tris in enumerate(tab):
        ids = [e for t in tris for e in t]
        ids += [-1] * (row - len(ids))
        lines.append("    {" + ", ".join(f"{v:2d}" for v in ids) + "},  // " + str(c))
    lines += ["};", ""]
    return "\n".join(lines)


def main(argv):
    text = render()
    if "--check" in argv:
        with open(OUT) as f:
            same = f.read() == text
        print("mc_table.h up to date" if same else "mc_table.h differs from the generator's output")
        return 0 if same else 1
    with open(OUT, "w") as f:
        f.write(text)
    print("wrote", OUT)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
