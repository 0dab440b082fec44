"""numpy restatement of esr_nerf_amd/csrc/mesh.hip's marching cubes (the contract of esr_mesh_count / esr_mesh_emit).

- A node is inside iff u > thr (thr rounded to binary32, as the kernel receives it); u == thr is outside.
- Every edge between lattice neighbours n, n + e_a whose inside flags differ holds one vertex at n + t e_a (index space),
  t = ((double)thr - (double)u[n]) / ((double)u[n + e_a] - (double)u[n]).
- Vertices are numbered by the owner node's linear index (i * R1 + j) * R2 + k, then by axis x < y < z.
- Triangles are listed by the cell's linear index over (R0-1) x (R1-1) x (R2-1), then in the order of the case table
  (esr_nerf_amd/csrc/mc_table.h, parsed here).

Vectorised: R = 256 runs in seconds.
"""
from __future__ import annotations

import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE_H = os.path.join(ROOT, "esr_nerf_amd", "csrc", "mc_table.h")


def load_table(path=TABLE_H):
    """(ntri [256] int64, tri [256, ROW] int64 edge ids, -1 padded) from the header."""
    text = open(path).read()
    row = int(re.search(r"#define ESR_MC_ROW (\d+)", text).group(1))
    ntri_body = text.split("ESR_MC_NTRI[256] = {", 1)[1].split("};", 1)[0]
    ntri = np.array([int(v) for v in re.findall(r"-?\d+", ntri_body)], np.int64)
    tri_body = text.split("ESR_MC_TRI[256][ESR_MC_ROW] = {", 1)[1].split("};", 1)[0]
    rows = re.findall(r"\{([^}]*)\}", tri_body)
    tri = np.array([[int(v) for v in r.split(",")] for r in rows], np.int64)
    assert ntri.shape == (256,) and tri.shape == (256, row)
    return ntri, tri


def edge_owner(e):
    """(owner corner offset (dx, dy, dz), axis) of cube edge id e (arrays allowed)."""
    e = np.asarray(e)
    axis, b0, b1 = e >> 2, e & 1, (e >> 1) & 1
    dx = np.where(axis == 0, 0, b0)
    dy = np.where(axis == 0, b0, np.where(axis == 1, 0, b1))
    dz = np.where(axis == 2, 0, b1)
    return dx, dy, dz, axis


def marching_cubes(u: np.ndarray, thr: float, table=None):
    """-> (vertices float64 [V, 3] in index space, triangles int64 [F, 3])"""
    ntri, tri = table if table is not None else load_table()
    u = np.ascontiguousarray(u, np.float32)
    R0, R1, R2 = u.shape
    thr32 = np.float32(thr)
    ins = u > thr32
    cross = np.zeros((R0, R1, R2, 3), bool)
    cross[:-1, :, :, 0] = ins[:-1] != ins[1:]
    cross[:, :-1, :, 1] = ins[:, :-1] != ins[:, 1:]
    cross[:, :, :-1, 2] = ins[:, :, :-1] != ins[:, :, 1:]
    flat = cross.reshape(-1)
    vid = np.cumsum(flat, dtype=np.int64) - 1
    vid[~flat] = -1
    vid = vid.reshape(R0, R1, R2, 3)
    n, a = np.nonzero(cross.reshape(-1, 3))                  # owner node (linear), axis: already in vertex order
    i, j, k = np.unravel_index(n, (R0, R1, R2))
    u0 = u.reshape(-1)[n].astype(np.float64)
    step = np.array([R1 * R2, R2, 1], np.int64)[a]
    u1 = u.reshape(-1)[n + step].astype(np.float64)
    t = (np.float64(thr32) - u0) / (u1 - u0)
    verts = np.stack([i, j, k], -1).astype(np.float64)
    verts[np.arange(len(n)), a] += t
    # cells
    b = ins.astype(np.int64)                                 # corner (dx, dy, dz) -> bit dx | dy << 1 | dz << 2
    case = (b[:-1, :-1, :-1] | b[1:, :-1, :-1] << 1 | b[:-1, 1:, :-1] << 2 | b[1:, 1:, :-1] << 3 |
            b[:-1, :-1, 1:] << 4 | b[1:, :-1, 1:] << 5 | b[:-1, 1:, 1:] << 6 | b[1:, 1:, 1:] << 7)
    case = case.reshape(-1)
    nt = ntri[case]
    cells = np.repeat(np.arange(case.size, dtype=np.int64), nt)
    if cells.size == 0:
        return verts.reshape(-1, 3), np.zeros((0, 3), np.int64)
    first = np.cumsum(nt) - nt
    local = np.arange(cells.size, dtype=np.int64) - np.repeat(first, nt)
    ci, cj, ck = np.unravel_index(cells, (R0 - 1, R1 - 1, R2 - 1))
    tris = np.empty((cells.size, 3), np.int64)
    for v in range(3):
        e = tri[case[cells], 3 * local + v]
        assert (e >= 0).all()
        dx, dy, dz, ax = edge_owner(e)
        tris[:, v] = vid[ci + dx, cj + dy, ck + dz, ax]
    assert (tris >= 0).all()
    return verts, tris


def counts(u: np.ndarray, thr: float, table=None):
    """(V, F) of marching_cubes(u, thr) without building the mesh (cheap at R = 512)."""
    ntri = (table if table is not None else load_table())[0]
    ins = np.ascontiguousarray(u, np.float32) > np.float32(thr)
    n_v = int(np.count_nonzero(ins[:-1] != ins[1:]) + np.count_nonzero(ins[:, :-1] != ins[:, 1:]) +
              np.count_nonzero(ins[:, :, :-1] != ins[:, :, 1:]))
    b = ins.view(np.uint8)
    case = np.zeros(tuple(s - 1 for s in ins.shape), np.uint8)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                case |= b[dx:dx + case.shape[0], dy:dy + case.shape[1], dz:dz + case.shape[2]] << (dx | dy << 1 | dz << 2)
    return n_v, int(np.bincount(case.reshape(-1), minlength=256) @ ntri)
