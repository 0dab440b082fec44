"""Mesh export on the device: the reference's ``extract_geometry`` (app/fine/model/voxurff.py:745-780) over
libesr_hip.so's esr_mesh_* kernels (esr_nerf_amd/csrc/mesh.hip).

``sdf_field``       the -sdf lattice field (optional Gaussian smoothing with esr_gauss3d_fwd, then esr_mesh_field)
``marching_cubes``  count -> scan -> emit; vertices in index space, triangles as vertex ids, both on the device
``extract_geometry`` world-space numpy arrays, what the reference returns
``connected_components`` / ``component_stats`` / ``keep_components`` / ``keep_largest``  mesh connectivity over the
                    esr_cc_* kernels (esr_nerf_amd/csrc/meshcc.hip): device tensors in, device tensors out
``simplify`` / ``simplify_to``  quadric vertex clustering over the esr_simplify_* kernels (esr_nerf_amd/csrc/simplify.hip)

The lattice axes are ``torch.linspace`` as the reference builds them (plumbing: the coordinates are the torch path's bit
for bit); the block-total scan is one ``torch.cumsum`` over 2 ceil(R^3 / 256) int64 totals.  No host copy of the field.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .modules import Gaussian3DConv


def _box(model):
    return model.xyz_min.float().cpu(), model.xyz_max.float().cpu()


def smooth_grid(grid: torch.Tensor, sigma: float = 0.5) -> torch.Tensor:
    """esr_gauss3d_fwd with the weights of ``Gaussian3DConv(sigma=sigma)`` (ksize 3, replicate padding).
    grid: device float32 [X, Y, Z]."""
    L = _lib.lib()
    w = Gaussian3DConv(sigma=sigma).m.weight.detach().reshape(-1).tolist()
    out = torch.empty_like(grid)
    with torch.cuda.device(grid.device):
        _lib.check(L.esr_gauss3d_fwd(_lib.ptr(grid), (C.c_float * len(w))(*w), 3, *grid.shape, _lib.ptr(out),
                                     _lib.stream_ptr(grid.device)), "esr_gauss3d_fwd")
    return out


def lattice_axes(lo: torch.Tensor, hi: torch.Tensor, resolution: int, device):
    """the three lattice axes, as app/utils/base/functions.py:115-117 builds them"""
    return [torch.linspace(float(lo[a]), float(hi[a]), resolution, device=device) for a in range(3)]


def field(grid: torch.Tensor, lo: torch.Tensor, hi: torch.Tensor, axes) -> torch.Tensor:
    """u[i,j,k] = -trilinear(grid, (xs[i], ys[j], zs[k])) (esr_mesh_field).  grid: device float32 [X, Y, Z];
    lo, hi: the box [3]; axes: three device float32 vectors."""
    L = _lib.lib()
    if grid.dim() != 3 or grid.dtype != torch.float32:
        raise ValueError("field: grid must be float32 [X, Y, Z]")
    axes = [a.to(grid.device, torch.float32).contiguous() for a in axes]
    dims = [int(a.numel()) for a in axes]
    box = (C.c_float * 6)(*[float(v) for v in lo.float()], *[float(v) for v in hi.float()])
    u = torch.empty(dims, dtype=torch.float32, device=grid.device)
    with torch.cuda.device(grid.device):
        _lib.check(L.esr_mesh_field(_lib.ptr(grid.contiguous()), *grid.shape, box, *[_lib.ptr(a) for a in axes], *dims,
                                    _lib.ptr(u), _lib.stream_ptr(grid.device)), "esr_mesh_field")
    return u


@torch.no_grad()
def sdf_field(model, resolution=512, smooth: bool = True, sigma: float = 0.5) -> torch.Tensor:
    """The HIP lattice field of ``modules.extract_sdf_field`` on the model's device: -sdf (smoothed by
    ``Gaussian3DConv(sigma=sigma)`` when ``smooth``) on a resolution^3 lattice of the bounding box."""
    grid = model.sdf.grid
    if not grid.is_cuda:
        raise RuntimeError("sdf_field needs a model on the GPU (there is no CPU path)")
    g = grid.detach()[0, 0].float().contiguous()
    if smooth:
        g = smooth_grid(g, sigma)
    if resolution is None:
        resolution = int(model.world_size[0])
    lo, hi = _box(model)
    return field(g, lo, hi, lattice_axes(lo, hi, int(resolution), grid.device))


def _scan(counts: torch.Tensor, nb: int):
    """block totals [vertices (nb) | triangles (nb)] -> (exclusive offsets of each half, V, F).  One flat cumsum (a
    device-wide scan; a [2, nb] cumsum along dim 1 was a single workgroup per row, 1.3 ms at R = 512)."""
    incl = torch.cumsum(counts, 0)
    offsets = incl - counts
    offsets[nb:] -= incl[nb - 1]
    n_v, n_all = (int(v) for v in incl[[nb - 1, 2 * nb - 1]].cpu())
    return offsets, n_v, n_all - n_v


@torch.no_grad()
def marching_cubes(u: torch.Tensor, threshold: float = 0.0):
    """Marching cubes of the device field u [R0, R1, R2] (float32) at ``threshold`` (rounded to float32).
    -> (vertices float64 [V, 3] in index space, triangles int64 [F, 3]), both on u's device.  A node is inside iff
    u > threshold; the vertex / triangle order and the winding are the contract of csrc/mesh.hip."""
    L = _lib.lib()
    if not u.is_cuda or u.dtype != torch.float32 or u.dim() != 3:
        raise ValueError("marching_cubes: u must be a float32 [R0, R1, R2] device tensor")
    u = u.contiguous()
    dims = [int(v) for v in u.shape]
    dev = u.device
    nb = int(L.esr_mesh_blocks(*dims))
    if nb < 0:
        raise ValueError(f"marching_cubes: every lattice dimension must be in [2, 1024], got {dims}")
    with torch.cuda.device(dev):
        s = _lib.stream_ptr(dev)
        counts = torch.empty(2 * nb, dtype=torch.int64, device=dev)
        _lib.check(L.esr_mesh_count(_lib.ptr(u), *dims, threshold, _lib.ptr(counts), s), "esr_mesh_count")
        offsets, n_v, n_f = _scan(counts, nb)
        verts = torch.empty(n_v, 3, dtype=torch.float64, device=dev)
        tris = torch.empty(n_f, 3, dtype=torch.int64, device=dev)
        if n_v == 0:
            return verts, tris
        if n_v >= 2 ** 31:
            raise RuntimeError(f"marching_cubes: {n_v} vertices exceed the kernels' 31-bit vertex ids")
        vid = torch.empty(dims, dtype=torch.int32, device=dev)
        _lib.check(L.esr_mesh_emit(_lib.ptr(u), *dims, threshold, _lib.ptr(offsets), _lib.ptr(vid), _lib.ptr(verts),
                                   _lib.ptr(tris), s), "esr_mesh_emit")
    return verts, tris


def extract_geometry(model, resolution=512, threshold=0.0, smooth: bool = True, sigma: float = 0.5):
    """(vertices float64 [V, 3] in world space, triangles int64 [F, 3]) as numpy arrays, as the reference returns them
    (voxurff.py:771-780: v / (R - 1) * (max - min) + min)."""
    u = sdf_field(model, resolution, smooth, sigma)
    verts, tris = marching_cubes(u, threshold)
    lo, hi = (b.numpy() for b in _box(model))
    res = np.array(u.shape, np.float64)
    v = verts.cpu().numpy()
    return v / (res - 1.0)[None, :] * (hi - lo)[None, :] + lo[None, :], tris.cpu().numpy()


# ----------------------------------------------------------------------------------------------------------------------
# connectivity (csrc/meshcc.hip): two selected faces are connected iff they share a vertex id


def _check_mesh(what, triangles, n_vertices):
    if not isinstance(triangles, torch.Tensor) or not triangles.is_cuda or triangles.dtype != torch.int64 or \
            triangles.dim() != 2 or triangles.shape[1] != 3:
        raise ValueError(f"{what}: triangles must be an int64 [F, 3] device tensor")
    n_vertices = int(n_vertices)
    if n_vertices < 0 or n_vertices >= 2 ** 31:
        raise ValueError(f"{what}: {n_vertices} vertices exceed the kernels' 31-bit vertex ids")
    if triangles.numel() and (int(triangles.min()) < 0 or int(triangles.max()) >= n_vertices):
        raise ValueError(f"{what}: a triangle names a vertex that does not exist")
    return triangles.contiguous(), n_vertices


@torch.no_grad()
def connected_components(triangles: torch.Tensor, n_vertices: int, face_mask=None):
    """Connected components of the selected faces.  triangles: device int64 [F, 3]; face_mask: device bool / uint8 [F]
    or None (every face).  -> (face_label int32 [F] on the device, K).  Two selected faces are connected iff they share
    a vertex id; an unselected face links nothing and gets -1.  Components are numbered 0 .. K-1 by the smallest vertex
    id they contain, so the labels are a function of the input alone."""
    L = _lib.lib()
    tris, n_v = _check_mesh("connected_components", triangles, n_vertices)
    dev, n_f = tris.device, int(tris.shape[0])
    mask = None
    if face_mask is not None:
        if not isinstance(face_mask, torch.Tensor) or face_mask.device != dev or face_mask.numel() != n_f or \
                face_mask.dtype not in (torch.bool, torch.uint8):
            raise ValueError("connected_components: face_mask must be a bool / uint8 [F] tensor on the triangles' device")
        mask = face_mask.reshape(-1).to(torch.uint8).contiguous()
    label = torch.empty(n_f, dtype=torch.int32, device=dev)
    if n_f == 0 or n_v == 0:
        return label, 0
    with torch.cuda.device(dev):
        s = _lib.stream_ptr(dev)
        parent = torch.empty(n_v, dtype=torch.int32, device=dev)
        owner = torch.empty(n_v, dtype=torch.int32, device=dev)
        _lib.check(L.esr_cc_link(_lib.ptr(tris), _lib.ptr(mask), n_f, n_v, _lib.ptr(parent), s), "esr_cc_link")
        _lib.check(L.esr_cc_flatten(_lib.ptr(tris), _lib.ptr(mask), n_f, n_v, _lib.ptr(parent), _lib.ptr(owner), s),
                   "esr_cc_flatten")
        incl = torch.cumsum(owner, 0)
        k = int(incl[-1])
        rank = (incl - 1).to(torch.int32)
        _lib.check(L.esr_cc_face_labels(_lib.ptr(tris), _lib.ptr(mask), n_f, _lib.ptr(parent), _lib.ptr(rank),
                                        _lib.ptr(label), s), "esr_cc_face_labels")
    return label, k


@torch.no_grad()
def component_stats(vertices: torch.Tensor, triangles: torch.Tensor, face_label: torch.Tensor, K: int, attr=None, *,
                    per_lane_atomics: bool = False):
    """Per-component sums over the faces with label >= 0.  vertices: device float64 [V, 3]; face_label: device int32 [F]
    in [-1, K); attr: device float32 [V, C], C <= 4, or None.  -> dict of device tensors: n_faces int64 [K], area,
    area_centroid [K, 3], centroid [K, 3] = area_centroid / area, bbox_min, bbox_max [K, 3] (float64) and, with attr,
    area_attr, mean_attr = area_attr / area [K, C] (float64) and peak float32 [K].  Counts, box and peak are exact.
    ``per_lane_atomics``: the kernel form without the in-wave reduction (for timing; the same results)."""
    L = _lib.lib()
    if not isinstance(vertices, torch.Tensor) or not vertices.is_cuda or vertices.dtype != torch.float64 or \
            vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError("component_stats: vertices must be a float64 [V, 3] device tensor")
    tris, n_v = _check_mesh("component_stats", triangles, vertices.shape[0])
    dev, n_f, K = tris.device, int(tris.shape[0]), int(K)
    if not isinstance(face_label, torch.Tensor) or face_label.device != dev or face_label.dtype != torch.int32 or \
            face_label.shape != (n_f,):
        raise ValueError("component_stats: face_label must be an int32 [F] tensor on the triangles' device")
    if K < 0 or (n_f and (int(face_label.min()) < -1 or int(face_label.max()) >= K)):
        raise ValueError("component_stats: a face label lies outside [-1, K)")
    n_attr = 0
    if attr is not None:
        if not isinstance(attr, torch.Tensor) or attr.device != dev or attr.dtype != torch.float32 or attr.dim() != 2 or \
                attr.shape[0] != n_v or not 1 <= attr.shape[1] <= 4:
            raise ValueError("component_stats: attr must be a float32 [V, C] tensor, C in 1 .. 4, on the mesh's device")
        attr, n_attr = attr.contiguous(), int(attr.shape[1])
    f64 = dict(dtype=torch.float64, device=dev)
    out = {"n_faces": torch.empty(K, dtype=torch.int64, device=dev), "area": torch.empty(K, **f64),
           "area_centroid": torch.empty(K, 3, **f64), "bbox_min": torch.empty(K, 3, **f64),
           "bbox_max": torch.empty(K, 3, **f64)}
    if n_attr:
        out["area_attr"] = torch.empty(K, n_attr, **f64)
        out["peak"] = torch.empty(K, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(L.esr_cc_stats(_lib.ptr(vertices.contiguous()), _lib.ptr(tris), _lib.ptr(face_label.contiguous()), n_f,
                                  K, _lib.ptr(attr), n_attr, int(bool(per_lane_atomics)), _lib.ptr(out["n_faces"]),
                                  _lib.ptr(out["area"]), _lib.ptr(out["area_centroid"]), _lib.ptr(out["bbox_min"]),
                                  _lib.ptr(out["bbox_max"]), _lib.ptr(out.get("area_attr")), _lib.ptr(out.get("peak")),
                                  _lib.stream_ptr(dev)), "esr_cc_stats")
    out["centroid"] = out["area_centroid"] / out["area"][:, None]
    if n_attr:
        out["mean_attr"] = out["area_attr"] / out["area"][:, None]
    return out


@torch.no_grad()
def keep_components(vertices: torch.Tensor, triangles: torch.Tensor, face_keep: torch.Tensor):
    """The mesh of the faces with ``face_keep`` (bool [F]) in their order, unreferenced vertices removed and the rest in
    their order.  Works on any device (torch indexing and chamfer.remove_unreferenced)."""
    from .chamfer import remove_unreferenced
    keep = torch.as_tensor(face_keep, device=triangles.device).reshape(-1).to(torch.bool)
    if keep.numel() != triangles.shape[0]:
        raise ValueError("keep_components: face_keep must have one entry per face")
    return remove_unreferenced(vertices, triangles[keep])


@torch.no_grad()
def keep_largest(vertices: torch.Tensor, triangles: torch.Tensor, k: int = 1, by: str = "area"):
    """The floater filter: the mesh of the ``k`` largest connected components, by surface ``"area"`` or by ``"faces"``
    (ties: the component with the smaller number first).  Faces and vertices keep their order."""
    if by not in ("area", "faces"):
        raise ValueError(f"keep_largest: by must be 'area' or 'faces', got {by!r}")
    if k < 1:
        raise ValueError("keep_largest: k must be >= 1")
    label, K = connected_components(triangles, vertices.shape[0])
    if K <= k:
        return keep_components(vertices, triangles, label >= 0)
    st = component_stats(vertices, triangles, label, K)
    size = st["area"] if by == "area" else st["n_faces"]
    order = torch.sort(size, descending=True, stable=True).indices
    chosen = torch.zeros(K, dtype=torch.bool, device=label.device)
    chosen[order[:k]] = True
    return keep_components(vertices, triangles, chosen[label.long()])


# ----------------------------------------------------------------------------------------------------------------------
# simplification (csrc/simplify.hip): quadric vertex clustering on a grid of cell size h

SIMPLIFY_MAX_CELLS = 2 ** 21 - 1         # most cells on an axis (the cluster key holds 21 bits per axis)
# A cluster with more pairs (incident faces) or members than this is summed by a workgroup in a fixed-shape tree instead of
# one lane's loop.  The sums' order, and so the last bits of the result, depend on it; everything else does not.
# Measured (tools/simplify_time.py, profiles/simplify_time.json, the cluster pass on 2.5 M faces with 12 channels): at
# cells of 4 lattice steps (52 pairs a cluster) one lane each is fastest, 1.06 ms from 128 up against 1.46 ms at 64; from 8
# steps on the lanes' loops dominate and 64 wins, 0.81 against 2.51 ms at 8 steps, 0.55 against 7.6 at 16, 0.65 against 3.6 at
# 64 steps (the values at 1024).  16 is faster still there (0.61 / 0.32 / 0.50 ms) but sends most clusters of a 2-step grid
# to a workgroup: 4.36 ms against 1.14.
SIMPLIFY_BIG = 64
SIMPLIFY_TRIALS = 24                     # most cell sizes simplify_to tries


def _check_simplify(what, vertices, triangles, attr):
    if not isinstance(vertices, torch.Tensor) or not vertices.is_cuda or vertices.dtype != torch.float64 or \
            vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError(f"{what}: vertices must be a float64 [V, 3] device tensor")
    tris, n_v = _check_mesh(what, triangles, vertices.shape[0])
    if tris.device != vertices.device:
        raise ValueError(f"{what}: vertices and triangles are on one device")
    if tris.shape[0] >= 2 ** 31:
        raise ValueError(f"{what}: {tris.shape[0]} faces exceed the kernels' 31-bit face ids")
    if attr is not None:
        if not isinstance(attr, torch.Tensor) or attr.device != vertices.device or attr.dtype != torch.float32 or \
                attr.dim() != 2 or attr.shape[0] != n_v or not 1 <= attr.shape[1] <= _lib.SIMPLIFY_MAX_C:
            raise ValueError(f"{what}: attr must be a float32 [V, C] tensor, C in 1 .. {_lib.SIMPLIFY_MAX_C}, on the mesh's device")
        attr = attr.contiguous()
    if n_v and not bool(torch.isfinite(vertices).all()):
        raise ValueError(f"{what}: a vertex is not finite")
    return vertices.contiguous(), tris, attr


def _check_cell(what, verts, cell):
    """the origin (device [3]) of the grid of cell size ``cell`` over ``verts``; refuses a grid of too many cells"""
    h = float(cell)
    if not (0.0 < h < float("inf")):
        raise ValueError(f"{what}: cell must be positive and finite, got {cell!r}")
    origin = verts.amin(0)
    dims = [int(d) for d in (torch.floor((verts.amax(0) - origin) / h) + 1.0).cpu()]
    if max(dims) > SIMPLIFY_MAX_CELLS:
        raise ValueError(f"{what}: cell {h} makes a grid of {dims} cells; an axis holds at most {SIMPLIFY_MAX_CELLS}")
    return h, origin.contiguous()


def _simplify_faces(verts, tris, h, origin, alloc):
    """the clustering and the face pass: everything of ``simplify`` that does not need the quadrics"""
    L = _lib.lib()
    dev, n_v, n_f = verts.device, int(verts.shape[0]), int(tris.shape[0])
    s = _lib.stream_ptr(dev)
    keys = alloc((n_v,), torch.int64)
    _lib.check(L.esr_simplify_cell_keys(_lib.ptr(verts), n_v, _lib.ptr(origin), h, _lib.ptr(keys), s), "esr_simplify_cell_keys")
    ckeys, inverse, counts = torch.unique(keys, sorted=True, return_inverse=True, return_counts=True)
    vc = inverse.to(torch.int32).contiguous()
    n_k = int(ckeys.shape[0])
    key_hi, key_lo = alloc((n_f,), torch.int64), alloc((n_f,), torch.int32)
    _lib.check(L.esr_simplify_face_keys(_lib.ptr(tris), n_f, _lib.ptr(vc), n_v, _lib.ptr(key_hi), _lib.ptr(key_lo), s),
               "esr_simplify_face_keys")
    # (key_hi, key_lo, face id) ascending: two stable sorts, the minor key first
    by_lo = torch.sort(key_lo, stable=True).indices
    order = by_lo[torch.sort(key_hi[by_lo], stable=True).indices].contiguous()
    keep, used = alloc((n_f,), torch.uint8), alloc((n_k,), torch.uint8)
    _lib.check(L.esr_simplify_keep(_lib.ptr(order), _lib.ptr(key_hi), _lib.ptr(key_lo), n_f, _lib.ptr(tris), _lib.ptr(vc), n_v,
                                   n_k, _lib.ptr(keep), _lib.ptr(used), s), "esr_simplify_keep")
    return ckeys.contiguous(), counts, vc, keep, used


def _simplify_segments(tris, vc, counts, alloc):
    """every cluster's members and incident faces as segments: (member_start [K + 1], member_ids [V], pair_start [K + 1],
    pairs [3 F] sorted, the INT64_MAX entries of repeated clusters last)"""
    L = _lib.lib()
    dev, n_v, n_f, n_k = vc.device, int(vc.shape[0]), int(tris.shape[0]), int(counts.shape[0])
    member_ids = torch.sort(vc, stable=True).indices.contiguous()
    member_start = torch.zeros(n_k + 1, dtype=torch.int64, device=dev)
    torch.cumsum(counts, 0, out=member_start[1:])
    pairs = alloc((3 * n_f,), torch.int64)
    _lib.check(L.esr_simplify_pair_keys(_lib.ptr(tris), n_f, _lib.ptr(vc), n_v, _lib.ptr(pairs), _lib.stream_ptr(dev)),
               "esr_simplify_pair_keys")
    pairs = torch.sort(pairs).values
    # (the INT64_MAX tail lies behind every segment: pair_start[K] is the number of real pairs)
    pair_start = torch.searchsorted(pairs, torch.arange(n_k + 1, dtype=torch.int64, device=dev) << 32).contiguous()
    return member_start, member_ids, pair_start, pairs


def _simplify_clusters(verts, tris, attr, vc, ckeys, seg, origin, h, lam, big, debug, alloc):
    """the per-cluster pass -> (positions [K, 3], attributes [K, C] or None, the debug sums [K, 15] or None)"""
    L = _lib.lib()
    n_v, n_f, n_k = int(verts.shape[0]), int(tris.shape[0]), int(ckeys.shape[0])
    n_c = 0 if attr is None else int(attr.shape[1])
    member_start, member_ids, pair_start, pairs = seg
    pos = alloc((n_k, 3), torch.float64)
    new_attr = alloc((n_k, n_c), torch.float32) if n_c else None
    sums = alloc((n_k, _lib.SIMPLIFY_DEBUG), torch.float64) if debug else None
    _lib.check(L.esr_simplify_clusters(_lib.ptr(verts), n_v, _lib.ptr(tris), n_f, _lib.ptr(vc), _lib.ptr(ckeys), n_k,
                                       _lib.ptr(member_start), _lib.ptr(member_ids), _lib.ptr(pair_start), _lib.ptr(pairs),
                                       3 * n_f, _lib.ptr(origin), h, lam, _lib.ptr(attr), n_c, big, _lib.ptr(pos),
                                       _lib.ptr(new_attr), _lib.ptr(sums), _lib.stream_ptr(verts.device)), "esr_simplify_clusters")
    return pos, new_attr, sums


@torch.no_grad()
def simplify(vertices: torch.Tensor, triangles: torch.Tensor, cell: float, lam: float = 1e-3, attr=None, big=None):
    """Quadric vertex clustering of a mesh on a grid of cell size ``cell`` (world units): every occupied cell becomes one
    vertex, placed where the regularised plane quadric of its incident faces is smallest along the segment from the
    members' mean that stays in the cell.  The definition is the comment of section S of include/esr_hip.h.

    vertices: device float64 [V, 3], finite; triangles: device int64 [F, 3]; attr: device float32 [V, C], C <= 16, or None.
    -> ``(vertices' float64 [V', 3], triangles' int64 [F', 3], attr' float32 [V', C] or None, vertex_map int32 [V],
    face_origin int64 [F'])``: ``vertex_map`` is the new id of each old vertex's cluster, -1 where no kept face names it;
    ``face_origin`` the old id of each kept face.  Kept faces stay in their order and keep their winding.  All on the
    device; only the finiteness flag and sizes (the grid's extent, V', F') are read back.  ``cell`` is never changed: a
    grid of more than 2^21 - 1 cells on an axis raises ``ValueError``.  The result is a function of the input and ``big``
    alone."""
    return _simplify(vertices, triangles, cell, lam, attr, big)


def _simplify(vertices, triangles, cell, lam, attr, big, debug=False, alloc=None):
    """``simplify``; for the tests, ``debug`` appends a dict of the per-cluster values BEFORE unreferenced clusters are
    dropped -- ``cluster_keys`` int64 [K], ``vertex_cluster`` int32 [V], ``positions`` float64 [K, 3], ``attr`` float32
    [K, C] or None, ``used`` uint8 [K], ``origin`` float64 [3] and ``sums`` float64 [K, 15] (A00 A01 A02 A11 A12 A22, b, c,
    S, W, xbar) -- and ``alloc(shape, dtype)`` allocates every buffer a kernel writes."""
    verts, tris, attr = _check_simplify("simplify", vertices, triangles, attr)
    lam = float(lam)
    if not (0.0 < lam < float("inf")):
        raise ValueError(f"simplify: lam must be positive and finite, got {lam!r}")
    big = SIMPLIFY_BIG if big is None else int(big)
    if big < 1:
        raise ValueError(f"simplify: big must be at least 1, got {big}")
    dev, n_v = verts.device, int(verts.shape[0])
    if alloc is None:
        def alloc(shape, dtype):
            return torch.empty(shape, dtype=dtype, device=dev)

    with torch.cuda.device(dev):
        if n_v == 0:
            out = (verts.clone(), tris.clone(), None if attr is None else attr.clone(),
                   torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.int64, device=dev))
            return out + ({},) if debug else out
        h, origin = _check_cell("simplify", verts, cell)
        ckeys, counts, vc, keep, used = _simplify_faces(verts, tris, h, origin, alloc)
        seg = _simplify_segments(tris, vc, counts, alloc)
        pos, new_attr, sums = _simplify_clusters(verts, tris, attr, vc, ckeys, seg, origin, h, lam, big, debug, alloc)
        face_origin = torch.nonzero(keep).reshape(-1)
        live = used.bool()
        new_id = torch.where(live, torch.cumsum(used, 0, dtype=torch.int32) - 1, -1).to(torch.int32)
        vertex_map = new_id[vc.long()]
        out = (pos[live], vertex_map[tris[face_origin]].long(), None if new_attr is None else new_attr[live], vertex_map,
               face_origin)
        if debug:
            out += (dict(cluster_keys=ckeys, vertex_cluster=vc, positions=pos, attr=new_attr, used=used, origin=origin, sums=sums),)
    return out


@torch.no_grad()
def simplify_to(vertices: torch.Tensor, triangles: torch.Tensor, target_faces: int, lam: float = 1e-3, attr=None, big=None,
                cell_min=None, rel_tol: float = 0.02, max_trials: int = SIMPLIFY_TRIALS):
    """``simplify`` at a cell size found by geometric bisection between ``cell_min`` (default: the bounding-box diagonal
    / 2^20, which the grid can always hold) and the bounding-box diagonal, so that at most ``target_faces`` faces remain.
    At most ``max_trials`` (<= 24) cell sizes are tried, each by the clustering and face pass alone; the bisection stops
    early once the bracket's ends are within ``rel_tol`` of each other.
    -> ``(mesh, cell, cell_over)``: ``mesh`` the five outputs of ``simplify`` at ``cell``, the smallest tried cell size
    whose face count is <= ``target_faces``; ``cell_over`` the largest tried cell size that exceeded the target, or None
    when the lower end already met it.  ``ValueError`` when even the diagonal leaves more than ``target_faces``."""
    verts, tris, attr = _check_simplify("simplify_to", vertices, triangles, attr)
    target = int(target_faces)
    max_trials = int(max_trials)
    if target < 0:
        raise ValueError(f"simplify_to: target_faces must not be negative, got {target_faces!r}")
    if not 2 <= max_trials <= SIMPLIFY_TRIALS:
        raise ValueError(f"simplify_to: max_trials must be in 2 .. {SIMPLIFY_TRIALS}, got {max_trials}")
    if not float(rel_tol) >= 0.0:
        raise ValueError(f"simplify_to: rel_tol must not be negative, got {rel_tol!r}")
    dev = verts.device
    if verts.shape[0] == 0:
        raise ValueError("simplify_to: the mesh has no vertices")

    def alloc(shape, dtype):
        return torch.empty(shape, dtype=dtype, device=dev)

    with torch.cuda.device(dev):
        diag = float(torch.linalg.vector_norm(verts.amax(0) - verts.amin(0)))
        if not diag > 0.0:
            raise ValueError("simplify_to: the mesh has no extent")
        lo = diag / 2.0 ** 20 if cell_min is None else float(cell_min)
        if not (0.0 < lo <= diag):
            raise ValueError(f"simplify_to: cell_min must lie in (0, {diag}], got {cell_min!r}")

        def faces_at(h):
            return int(_simplify_faces(verts, tris, *_check_cell("simplify_to", verts, h), alloc)[3].sum())

        if faces_at(diag) > target:
            raise ValueError(f"simplify_to: a cell of the bounding-box diagonal still leaves more than {target} faces")
        ok, over, trials = diag, None, 2
        if faces_at(lo) <= target:
            ok = lo
        else:
            over = lo
            while trials < max_trials and ok > over * (1.0 + float(rel_tol)):
                mid = (ok * over) ** 0.5
                if not over < mid < ok:
                    break
                trials += 1
                if faces_at(mid) <= target:
                    ok = mid
                else:
                    over = mid
    return simplify(verts, tris, ok, lam=lam, attr=attr, big=big), ok, over
