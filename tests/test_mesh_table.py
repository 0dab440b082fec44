"""The marching-cubes case table (esr_nerf_amd/csrc/mc_table.h): it is what tools/gen_mc_table.py writes, and every case
obeys the face rule restated here independently of the generator.  CPU only."""
import importlib.util
import os

import numpy as np
import pytest

import mesh_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _generator():
    spec = importlib.util.spec_from_file_location("gen_mc_table", os.path.join(ROOT, "tools", "gen_mc_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


NTRI, TRI = mesh_ref.load_table()


def corners_of_edge(e):
    dx, dy, dz, ax = (int(v) for v in mesh_ref.edge_owner(e))
    c0 = (dx, dy, dz)
    c1 = list(c0)
    c1[ax] = 1
    return c0, tuple(c1)


def bit(c):
    return c[0] | c[1] << 1 | c[2] << 2


def mid(e):
    a, b = corners_of_edge(e)
    return (np.array(a, float) + np.array(b, float)) / 2


EDGE_OF = {frozenset(corners_of_edge(e)): e for e in range(12)}


def case_tris(case):
    row = TRI[case]
    n = int(NTRI[case])
    assert (row[3 * n:] == -1).all() and (row[:3 * n] >= 0).all()
    return [tuple(int(v) for v in row[3 * t:3 * t + 3]) for t in range(n)]


def crossed(case):
    return {e for e in range(12) if (case >> bit(corners_of_edge(e)[0]) & 1) != (case >> bit(corners_of_edge(e)[1]) & 1)}


def face_rule(case):
    """Directed face segments: one per face with 1, 2 adjacent or 3 inside corners; two cutting off the inside corners
    of an ambiguous face; p -> q with ((q - p) x (c - p)) . N < 0 for an inside corner c on the segment's side."""
    segs = set()
    for axis in range(3):
        u, v = [b for b in range(3) if b != axis]
        for side in (0, 1):
            cyc = []
            for pu, pv in ((0, 0), (1, 0), (1, 1), (0, 1)):
                c = [0, 0, 0]
                c[axis], c[u], c[v] = side, pu, pv
                cyc.append(tuple(c))
            N = np.zeros(3)
            N[axis] = 1.0 if side else -1.0
            ins = [bool(case >> bit(c) & 1) for c in cyc]
            edges = [EDGE_OF[frozenset((cyc[i], cyc[(i + 1) % 4]))] for i in range(4)]   # cyclic edge i: corners i, i+1
            pairs = []
            if sum(ins) in (1, 2, 3) and not (ins[0] == ins[2] and ins[1] == ins[3]):
                cut = [edges[i] for i in range(4) if ins[i] != ins[(i + 1) % 4]]
                pairs.append((cut[0], cut[1], cyc[ins.index(True)]))
            elif sum(ins) == 2:                                                        # ambiguous: separate the insides
                for i in range(4):
                    if ins[i]:
                        pairs.append((edges[(i - 1) % 4], edges[i], cyc[i]))
            for p, q, c in pairs:
                s = np.dot(np.cross(mid(q) - mid(p), np.array(c, float) - mid(p)), N)
                segs.add((p, q) if s < 0 else (q, p))
    return segs


def test_generator_reproduces_the_header():
    gen = _generator()
    with open(os.path.join(ROOT, "esr_nerf_amd", "csrc", "mc_table.h")) as f:
        assert gen.render() == f.read()


def test_empty_cases():
    assert NTRI[0] == 0 and NTRI[255] == 0 and (TRI[0] == -1).all() and (TRI[255] == -1).all()


@pytest.mark.parametrize("case", range(256))
def test_case_obeys_the_face_rule(case):
    tris = case_tris(case)
    used = {e for t in tris for e in t}
    assert used <= crossed(case)                              # only crossed edges
    assert used == crossed(case)                              # every crossed edge
    # boundary of the triangle set (directed edges whose reverse is absent) == the face segments
    directed = {}
    for a, b, c in tris:
        assert len({a, b, c}) == 3
        for p, q in ((a, b), (b, c), (c, a)):
            directed[(p, q)] = directed.get((p, q), 0) + 1
    assert all(n == 1 for n in directed.values())
    boundary = {d for d in directed if (d[1], d[0]) not in directed}
    assert boundary == face_rule(case)
    # orientation: (b - a) x (c - a) points from the inside corners of the triangle's edges to the outside ones
    for a, b, c in tris:
        nrm = np.cross(mid(b) - mid(a), mid(c) - mid(a))
        out = 0.0
        for e in (a, b, c):
            c0, c1 = corners_of_edge(e)
            d = np.array(c1, float) - np.array(c0, float)
            out += float(np.dot(nrm, d if case >> bit(c0) & 1 else -d))
        assert out > 0, (case, (a, b, c))


def _edge_census(tris):
    fwd = tris.reshape(-1, 3)
    e = np.concatenate([fwd[:, [0, 1]], fwd[:, [1, 2]], fwd[:, [2, 0]]])
    und = np.sort(e, 1)
    key, inv, cnt = np.unique(und, axis=0, return_inverse=True, return_counts=True)
    sign = np.where(e[:, 0] < e[:, 1], 1, -1)
    bal = np.zeros(len(key), np.int64)
    np.add.at(bal, inv.reshape(-1), sign)
    return key, cnt, bal


def test_random_sign_lattice_is_closed_and_oriented():
    """A random-sign field (many ambiguous faces): every edge of the mesh away from the lattice boundary lies in exactly two
    triangles, traversed in opposite directions."""
    rng = np.random.default_rng(7)
    u = rng.standard_normal((14, 11, 9)).astype(np.float32)
    v, f = mesh_ref.marching_cubes(u, 0.0)
    assert len(f) > 500
    assert (f[:, 0] != f[:, 1]).all() and (f[:, 1] != f[:, 2]).all() and (f[:, 0] != f[:, 2]).all()
    key, cnt, bal = _edge_census(f)
    dims = np.array(u.shape) - 1.0

    def on_face(p):
        return (p == 0) | (p == dims)

    open_ = (cnt != 2) | (bal != 0)
    assert open_.any()                                        # the box cuts the surface
    for a, b in key[open_]:
        assert (on_face(v[a]) & on_face(v[b])).any(), (v[a], v[b])   # both ends on one lattice face
    assert ((cnt == 2) & (bal == 0)).sum() > 0.8 * len(key)


def test_reference_sphere_is_a_closed_sphere():
    R, r = 40, 13.3
    g = np.arange(R, dtype=np.float64) - (R - 1) / 2
    u = (r - np.sqrt(g[:, None, None] ** 2 + g[None, :, None] ** 2 + g[None, None, :] ** 2)).astype(np.float32)
    v, f = mesh_ref.marching_cubes(u, 0.0)
    key, cnt, bal = _edge_census(f)
    assert (cnt == 2).all() and (bal == 0).all()
    assert len(v) - len(key) + len(f) == 2
    vol = np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6
    assert abs(vol / (4 / 3 * np.pi * r ** 3) - 1) < 0.01
