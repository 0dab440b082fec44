"""The DTU Chamfer metric on the device: the reference's ``utils2.metric.DTU_CD`` (utils2/metric.py:113-256) over
libesr_hip.so's esr_cd_* kernels (esr_nerf_amd/csrc/chamfer.hip), plus the file reading the trainer did with trimesh.

``sample_mesh_points``  the referenced vertices, then points sampled on every triangle (count -> cumsum -> fill)
``radius_downsample``   the keep mask of the reference's greedy radius loop, in a given order (rounds on the device)
``nn_distance``         exact nearest-neighbour distances, +inf at or beyond max_dist
``dtu_chamfer``         (mean_d2s, mean_s2d, overall) with a seeded device permutation for the reference's unseeded shuffle
``DTU_CD``              the drop-in with the reference's signature
``read_ply`` / ``write_ply`` / ``load_dtu_pcd``  replace trimesh.load of the stl cloud, mesh.export and DTU.pcd's reads

Plumbing in torch: the unreferenced-vertex compaction, the scans, ``torch.sort`` of the cell keys, the bound / ObsMask /
ground-plane filters (exact f64 elementwise ops in numpy's order) and the two means.  Memory of an index over n points:
n x (24 B sorted copy + 8 B key + 8 B sort index + 4 B id) + up to n x (8 B start) + a hash table of 12 B per slot at
2-4 slots per occupied cell -- about 90 B per point, under 2 GB for the 20 M points of a DTU-scale mesh sample.
"""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np
import torch

from . import _lib

_MAX_CELLS = (1 << 21) - 2           # cells per axis of a key (21 bits)
_COARSE = 8                          # nearest neighbour: coarse cell = 8^3 fine cells
_NN_MIN_CELLS = 128                  # nearest neighbour: fine cells at least max_dist / 128 wide, so no search walks
                                     # more than ~17 coarse rings (max_dist / (8 h) + 1) whatever the target set's extent
_ROUNDS_PER_READ = 4                 # downsample rounds launched between two read-backs of the "changed" flags


def _dev(device=None):
    return torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())


def _as_points(x, device) -> torch.Tensor:
    t = torch.as_tensor(np.asarray(x, dtype=np.float64) if not isinstance(x, torch.Tensor) else x)
    t = t.to(device=device, dtype=torch.float64).reshape(-1, 3).contiguous()
    return t


def _pow2(n: int) -> int:
    return 1 << max(1, int(n - 1).bit_length())


class CellIndex:
    """The cell index of esr_cd_index_t over ``points`` (device f64 [n, 3], n >= 1): cell size ``h``, the points sorted by
    cell key, the hash table of the occupied cells and, when ``coarse``, the occupancy table of the coarse cells."""

    def __init__(self, points: torch.Tensor, h: float, coarse: int = 0):
        L, dev = _lib.lib(), points.device
        if points.shape[0] >= 2 ** 31:
            raise ValueError(f"CellIndex: {points.shape[0]} points exceed the kernels' 31-bit point ids")
        lo, hi = points.min(0).values, points.max(0).values
        lo_h, hi_h = lo.cpu().numpy(), hi.cpu().numpy()
        ext = float((hi_h - lo_h).max())
        mag = float(np.abs(np.concatenate([lo_h, hi_h])).max())
        # a cell size the 21-bit keys can hold, and one far above the rounding of (p - origin) at this magnitude
        h = max(float(h), ext / _MAX_CELLS, mag * 2.0 ** -30, 1e-300)
        dims = [int(math.floor((hi_h[a] - lo_h[a]) / h)) + 1 for a in range(3)]
        if max(dims) > _MAX_CELLS:
            h *= max(dims) / _MAX_CELLS * (1 + 1e-9)
            dims = [int(math.floor((hi_h[a] - lo_h[a]) / h)) + 1 for a in range(3)]
        self.h, self.dims, self.coarse = h, dims, coarse
        ix = _lib.EsrCdIndex()
        ix.origin[:] = [float(v) for v in lo_h]
        ix.h, ix.coarse = h, coarse
        ix.dims[:] = dims
        n = points.shape[0]
        with torch.cuda.device(dev):
            s = _lib.stream_ptr(dev)
            keys = torch.empty(n, dtype=torch.int64, device=dev)
            _lib.check(L.esr_cd_cell_keys(C.byref(ix), _lib.ptr(points), n, _lib.ptr(keys), s), "esr_cd_cell_keys")
            skeys, order = torch.sort(keys, stable=True)
            ukeys, counts = torch.unique_consecutive(skeys, return_counts=True)
            self.start = torch.cat([counts.new_zeros(1), torch.cumsum(counts, 0)])
            self.pts = points[order].contiguous()
            self.ids = order.to(torch.int32)
            self.n_cells = int(ukeys.numel())
            self.tkeys, self.tcells = self._table(ukeys, True)
            ix.cap = self.tkeys.numel()
            ix.keys, ix.cells = _lib.ptr(self.tkeys), _lib.ptr(self.tcells)
            ix.start, ix.pts, ix.ids = _lib.ptr(self.start), _lib.ptr(self.pts), _lib.ptr(self.ids)
            if coarse:
                m = (1 << 21) - 1
                cx, cy, cz = ukeys >> 42, (ukeys >> 21) & m, ukeys & m
                ck = torch.unique((cx // coarse) << 42 | (cy // coarse) << 21 | (cz // coarse))
                self.ckeys, _ = self._table(ck, False)
                ix.ccap, ix.ckeys = self.ckeys.numel(), _lib.ptr(self.ckeys)
        self.ix = ix

    @staticmethod
    def _table(ukeys: torch.Tensor, with_vals: bool):
        cap = _pow2(2 * ukeys.numel() + 1)
        tk = torch.full((cap,), -1, dtype=torch.int64, device=ukeys.device)
        tv = torch.empty(cap, dtype=torch.int32, device=ukeys.device) if with_vals else None
        _lib.check(_lib.lib().esr_cd_hash_insert(_lib.ptr(ukeys.contiguous()), ukeys.numel(), cap, _lib.ptr(tk),
                                                 _lib.ptr(tv), _lib.stream_ptr(ukeys.device)), "esr_cd_hash_insert")
        return tk, tv


# ----------------------------------------------------------------------------------------------------------------------
# the three device stages


@torch.no_grad()
def remove_unreferenced(vertices: torch.Tensor, triangles: torch.Tensor):
    """trimesh.Trimesh.remove_unreferenced_vertices: the referenced vertices in their order, the triangles renumbered"""
    used = torch.zeros(vertices.shape[0], dtype=torch.bool, device=vertices.device)
    used[triangles.reshape(-1)] = True
    remap = torch.cumsum(used.to(torch.int64), 0) - 1
    return vertices[used].contiguous(), remap[triangles].contiguous()


@torch.no_grad()
def sample_mesh_points(vertices, triangles, thresh: float = 0.2, device=None) -> torch.Tensor:
    """The reference's data_pcd (metric.py:119-164): the referenced vertices, then the samples of every triangle with
    area2 > 0 in triangle order.  -> device f64 [P, 3]."""
    L, dev = _lib.lib(), _dev(device if device is not None else
                              (vertices.device if isinstance(vertices, torch.Tensor) and vertices.is_cuda else None))
    v = _as_points(vertices, dev)
    f = torch.as_tensor(np.asarray(triangles) if not isinstance(triangles, torch.Tensor) else triangles)
    f = f.to(device=dev, dtype=torch.int64).reshape(-1, 3).contiguous()
    if f.numel() and (int(f.min()) < 0 or int(f.max()) >= v.shape[0]):
        raise ValueError("sample_mesh_points: a triangle names a vertex that does not exist")
    v, f = remove_unreferenced(v, f)
    n_tri = f.shape[0]
    with torch.cuda.device(dev):
        s = _lib.stream_ptr(dev)
        counts = torch.empty(n_tri, dtype=torch.int64, device=dev)
        _lib.check(L.esr_cd_sample_count(_lib.ptr(v), _lib.ptr(f), n_tri, thresh, _lib.ptr(counts), s),
                   "esr_cd_sample_count")
        incl = torch.cumsum(counts, 0)
        total = int(incl[-1]) if n_tri else 0
        out = torch.empty(v.shape[0] + total, 3, dtype=torch.float64, device=dev)
        out[:v.shape[0]] = v
        if total:
            _lib.check(L.esr_cd_sample_fill(_lib.ptr(v), _lib.ptr(f), n_tri, thresh, _lib.ptr(incl - counts),
                                            _lib.ptr(out[v.shape[0]:]), s), "esr_cd_sample_fill")
    return out


@torch.no_grad()
def radius_downsample(points, thresh: float, order=None, return_rounds: bool = False):
    """Keep mask [n] (device bool) over ``points[order]``: position k is kept exactly when no kept earlier position lies
    within ``thresh`` (((dx*dx + dy*dy) + dz*dz) <= thresh*thresh) -- the loop of metric.py:176-186.  ``order``: a
    permutation (default: the identity).  ``return_rounds``: also the number of rounds that changed a state."""
    L = _lib.lib()
    p = points if isinstance(points, torch.Tensor) and points.is_cuda else _as_points(points, _dev())
    p = p.to(torch.float64).reshape(-1, 3)
    dev = p.device
    if order is not None:
        p = p[torch.as_tensor(order, device=dev, dtype=torch.int64)]
    p = p.contiguous()
    n = p.shape[0]
    state = torch.zeros(n, dtype=torch.int8, device=dev)
    rounds = 0
    if n:
        # cells at least thresh wide (and a margin over it), so every pair within thresh lies in neighbouring cells
        index = CellIndex(p, thresh * (1.0 + 2.0 ** -20))
        flags = torch.zeros(_ROUNDS_PER_READ, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            s = _lib.stream_ptr(dev)
            while True:
                flags.zero_()
                for r in range(_ROUNDS_PER_READ):
                    _lib.check(L.esr_cd_downsample_round(C.byref(index.ix), _lib.ptr(p), n, thresh,
                                                         _lib.ptr(state), _lib.ptr(flags[r:r + 1]), s),
                               "esr_cd_downsample_round")
                f = flags.cpu().tolist()
                if 0 in f:
                    rounds += f.index(0)
                    break
                rounds += _ROUNDS_PER_READ
    keep = state == 1
    return (keep, rounds) if return_rounds else keep


def _nn_cell(t: torch.Tensor) -> float:
    """A fine cell size for nearest-neighbour search over a surface-like cloud: about 8 points per occupied cell on
    the central 90 % of the cloud (the cell size only moves the speed; the distances are exact whatever it is)."""
    n = t.shape[0]
    sub = t[:: max(1, n // 1_000_000)]
    q = torch.quantile(sub, torch.tensor([0.05, 0.95], dtype=torch.float64, device=t.device), dim=0)
    ext = float((q[1] - q[0]).max()) / 0.9
    return max(ext * math.sqrt(8.0 / n), 1e-12)


@torch.no_grad()
def nn_distance(queries, targets, max_dist: float = 20.0, cell: float | None = None) -> torch.Tensor:
    """Distance from every query to its nearest target: sqrt of the smallest ((dx*dx + dy*dy) + dz*dz), +inf when that
    distance is not < max_dist (or there is no target).  -> device f64 [nq].  ``cell``: the fine cell size (default:
    from the target density); it is raised to max_dist / 128 at least, which bounds the work of every query even for a
    target set of one point or of coincident points.  The distances do not depend on it."""
    L = _lib.lib()
    dev = _dev(queries.device if isinstance(queries, torch.Tensor) and queries.is_cuda else None)
    q, t = _as_points(queries, dev), _as_points(targets, dev)
    out = torch.full((q.shape[0],), math.inf, dtype=torch.float64, device=dev)
    if not q.shape[0] or not t.shape[0]:
        return out
    if not max_dist > 0:
        raise ValueError(f"nn_distance: max_dist must be > 0, got {max_dist}")
    h = max(cell if cell is not None else _nn_cell(t), max_dist / _NN_MIN_CELLS)
    index = CellIndex(t, h, coarse=_COARSE)
    with torch.cuda.device(dev):
        _lib.check(L.esr_cd_nn(C.byref(index.ix), _lib.ptr(q), q.shape[0], max_dist, _lib.ptr(out),
                               _lib.stream_ptr(dev)), "esr_cd_nn")
    return out


# ----------------------------------------------------------------------------------------------------------------------
# the metric


def _mean_below(d: torch.Tensor, max_dist: float) -> float:
    sel = d[d < max_dist]
    return float(sel.sum()) / sel.numel() if sel.numel() else math.nan


@torch.no_grad()
def dtu_filters(data_down: torch.Tensor, obs_mask, bb, res, patch=60):
    """metric.py:189-207: (data_in, data_in_obs).  BB is cast to float32 first, as the reference does; the ObsMask index
    is np.around (half to even) of (p - f32(BB0)) / Res."""
    dev = data_down.device
    bb32 = np.asarray(bb, dtype=np.float32).reshape(2, 3)
    lo = torch.as_tensor((bb32[0] - np.float32(patch)).astype(np.float64), device=dev)
    hi = torch.as_tensor((bb32[1] + np.float32(patch * 2)).astype(np.float64), device=dev)
    inb = ((data_down >= lo) & (data_down < hi)).all(1)
    data_in = data_down[inb]
    res_t = torch.as_tensor(np.asarray(res, dtype=np.float64).reshape(-1), device=dev)
    g = torch.round((data_in - torch.as_tensor(bb32[0].astype(np.float64), device=dev)) / res_t).to(torch.int64)
    obs = np.asarray(obs_mask)
    shape = torch.as_tensor(obs.shape, dtype=torch.int64, device=dev)
    ginb = ((g >= 0) & (g < shape)).all(1)
    gi = g[ginb]
    om = torch.as_tensor(obs.astype(np.bool_), device=dev)
    in_obs = om[gi[:, 0], gi[:, 1], gi[:, 2]]
    return data_in, data_in[ginb][in_obs]


def above_plane(stl: torch.Tensor, ground_plane) -> torch.Tensor:
    """metric.py:221-222: ((P0*x + P1*y) + P2*z) + P3 > 0, each product and sum rounded separately"""
    P = [float(v) for v in np.asarray(ground_plane, dtype=np.float64).reshape(4)]
    s = stl[:, 0] * P[0]
    s = s + stl[:, 1] * P[1]
    s = s + stl[:, 2] * P[2]
    return (s + P[3]) > 0


@torch.no_grad()
def dtu_chamfer(vertices, triangles, obs_mask, bb, res, stl, ground_plane, max_dist=20.0, patch=60, thresh=0.2, *,
                seed=0, order=None, device=None, stats=None):
    """(mean_d2s, mean_s2d, overall) as floats.  The data cloud is shuffled by ``order`` (a permutation of the sampled
    points) or else by a device permutation seeded with ``seed`` -- the reference's unseeded default_rng shuffle.  A mean
    over an empty selection is nan.  ``stats``: a dict that receives the point counts and the downsample's rounds."""
    dev = _dev(device)
    pts = sample_mesh_points(vertices, triangles, thresh, device=dev)
    n = pts.shape[0]
    if order is None:
        g = torch.Generator(device=dev)
        g.manual_seed(int(seed))
        order = torch.randperm(n, generator=g, device=dev)
    else:
        order = torch.as_tensor(order, dtype=torch.int64, device=dev)
        if order.numel() != n:
            raise ValueError(f"dtu_chamfer: order has {order.numel()} entries for {n} sampled points")
    data = pts[order].contiguous()
    keep, rounds = radius_downsample(data, thresh, return_rounds=True)
    data_down = data[keep]
    data_in, data_in_obs = dtu_filters(data_down, obs_mask, bb, res, patch)
    stl_t = _as_points(stl.vertices if hasattr(stl, "vertices") else stl, dev)
    d2s = nn_distance(data_in_obs, stl_t, max_dist)
    stl_above = stl_t[above_plane(stl_t, ground_plane)].contiguous()
    s2d = nn_distance(stl_above, data_in, max_dist)
    mean_d2s, mean_s2d = _mean_below(d2s, max_dist), _mean_below(s2d, max_dist)
    if stats is not None:
        stats.update(points=n, kept=int(data_down.shape[0]), data_in=int(data_in.shape[0]),
                     data_in_obs=int(data_in_obs.shape[0]), stl_above=int(stl_above.shape[0]), rounds=rounds)
    return mean_d2s, mean_s2d, (mean_d2s + mean_s2d) / 2


def DTU_CD(mesh, ObsMask, BB, Res, stl, ground_plane, max_dist: float = 20.0, patch: int = 60, thresh: float = 0.2):
    """Drop-in for utils2.metric.DTU_CD.  ``mesh``: anything with ``.vertices`` and ``.faces``, or a (V, F) pair; it is
    not modified.  ``stl``: an [N, 3] array or anything with ``.vertices``.  The shuffle is seeded (seed 0), and the
    reference's visualisation colours, which it discards, are not computed."""
    if hasattr(mesh, "vertices") and hasattr(mesh, "faces"):
        v, f = mesh.vertices, mesh.faces
    else:
        v, f = mesh
    return dtu_chamfer(v, f, ObsMask, BB, Res, stl, ground_plane, max_dist, patch, thresh)


# ----------------------------------------------------------------------------------------------------------------------
# files

_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
              "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
              "double": "f8", "float64": "f8"}


def _ply_header(f):
    if f.readline().strip() != b"ply":
        raise ValueError("read_ply: not a PLY file")
    fmt, elements = None, []
    while True:
        line = f.readline()
        if not line:
            raise ValueError("read_ply: the header has no end_header")
        w = line.decode("ascii", "replace").split()
        if not w or w[0] in ("comment", "obj_info"):
            continue
        if w[0] == "format":
            fmt = w[1]
        elif w[0] == "element":
            elements.append((w[1], int(w[2]), []))
        elif w[0] == "property":
            if w[1] == "list":
                elements[-1][2].append((w[4], ("list", w[2], w[3])))
            else:
                elements[-1][2].append((w[2], w[1]))
        elif w[0] == "end_header":
            return fmt, elements


def read_ply(path):
    """(vertices f64 [N, 3] from x, y, z, faces i64 [F, 3] or None) of an ASCII or binary PLY with any other vertex
    properties (binary big-endian too).  Faces: the first list property of the face element, triangles only."""
    with open(path, "rb") as f:
        fmt, elements = _ply_header(f)
        if fmt not in ("ascii", "binary_little_endian", "binary_big_endian"):
            raise ValueError(f"read_ply: unknown format {fmt}")
        end = "<" if fmt == "binary_little_endian" else ">"
        verts = faces = None
        tokens = None
        if fmt == "ascii":
            tokens = iter(f.read().split())
        for name, count, props in elements:
            if fmt == "ascii":
                if any(isinstance(t, tuple) for _, t in props):
                    rows = []
                    for _ in range(count):
                        row = []
                        for _, t in props:
                            if isinstance(t, tuple):
                                k = int(next(tokens))
                                row.append([float(next(tokens)) for _ in range(k)])
                            else:
                                row.append(float(next(tokens)))
                        rows.append(row)
                    if name == "face":
                        li = next(i for i, (_, t) in enumerate(props) if isinstance(t, tuple))
                        faces = np.asarray([r[li] for r in rows], dtype=np.int64).reshape(-1, 3)
                    continue
                a = np.array([float(next(tokens)) for _ in range(count * len(props))], dtype=np.float64)
                a = a.reshape(count, len(props))
                if name == "vertex":
                    cols = [p for p, _ in props]
                    verts = a[:, [cols.index(c) for c in ("x", "y", "z")]].astype(np.float64)
                continue
            if all(not isinstance(t, tuple) for _, t in props):
                dt = np.dtype([(p, end + _PLY_TYPES[t]) for p, t in props])
                a = np.frombuffer(f.read(dt.itemsize * count), dtype=dt, count=count)
                if name == "vertex":
                    verts = np.stack([a[c].astype(np.float64) for c in ("x", "y", "z")], 1)
                continue
            rows = []
            for _ in range(count):
                row = None
                for p, t in props:
                    if isinstance(t, tuple):
                        ct, it = np.dtype(end + _PLY_TYPES[t[1]]), np.dtype(end + _PLY_TYPES[t[2]])
                        k = int(np.frombuffer(f.read(ct.itemsize), ct)[0])
                        vals = np.frombuffer(f.read(it.itemsize * k), it)
                        if row is None:
                            row = vals
                    else:
                        f.read(np.dtype(_PLY_TYPES[t]).itemsize)
                rows.append(row)
            if name == "face":
                faces = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
    if verts is None:
        raise ValueError("read_ply: no vertex element")
    return verts, faces


def write_ply(path, vertices, triangles=None):
    """A binary little-endian PLY: double x, y, z, and int32 triangle lists when ``triangles`` is given (what
    mesh.export("mesh.ply") wrote, at full precision)."""
    v = np.ascontiguousarray(np.asarray(vertices, dtype="<f8").reshape(-1, 3))
    t = None if triangles is None else np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}", "property double x",
            "property double y", "property double z"]
    if t is not None:
        head += [f"element face {len(t)}", "property list uchar int vertex_indices"]
    head.append("end_header")
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode("ascii"))
        f.write(v.tobytes())
        if t is not None:
            rec = np.empty(len(t), dtype=[("n", "u1"), ("v", "<i4", (3,))])
            rec["n"] = 3
            rec["v"] = t
            f.write(rec.tobytes())


def load_dtu_pcd(root, scene: int):
    """(ObsMask, BB, Res, stl, ground_plane) of a DTU scene, as data/dtu/dtu.py:63-72 of the reference builds DTU.pcd;
    stl is the f64 [N, 3] array of Points/stl/stl{scene:03}_total.ply."""
    from scipy.io import loadmat
    m = loadmat(os.path.join(root, "ObsMask", f"ObsMask{scene}_10.mat"))
    ObsMask, BB, Res = (m[k] for k in ("ObsMask", "BB", "Res"))
    stl, _ = read_ply(os.path.join(root, "Points", "stl", f"stl{scene:03}_total.ply"))
    ground_plane = loadmat(os.path.join(root, "ObsMask", f"Plane{scene}.mat"))["P"]
    return ObsMask, BB, Res, stl, ground_plane


__all__ = ["sample_mesh_points", "radius_downsample", "nn_distance", "dtu_chamfer", "DTU_CD", "read_ply", "write_ply",
           "load_dtu_pcd", "CellIndex"]
