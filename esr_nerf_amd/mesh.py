"""Mesh export on the device: the reference's ``extract_geometry`` (app/fine/model/voxurff.py:745-780) over
libesr_hip.so's esr_mesh_* kernels (esr_nerf_amd/csrc/mesh.hip).

``sdf_field``       the -sdf lattice field (optional Gaussian smoothing with esr_gauss3d_fwd, then esr_mesh_field)
``marching_cubes``  count -> scan -> emit; vertices in index space, triangles as vertex ids, both on the device
``extract_geometry`` world-space numpy arrays, what the reference returns
``connected_components`` / ``component_stats`` / ``keep_components`` / ``keep_largest``  mesh connectivity over the
                    esr_cc_* kernels (esr_nerf_amd/csrc/meshcc.hip): device tensors in, device tensors out

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
    thr = C.c_float(threshold)
    nb = int(L.esr_mesh_blocks(*dims))
    if nb < 0:
        raise ValueError(f"marching_cubes: every lattice dimension must be in [2, 1024], got {dims}")
    with torch.cuda.device(dev):
        s = _lib.stream_ptr(dev)
        counts = torch.empty(2 * nb, dtype=torch.int64, device=dev)
        _lib.check(L.esr_mesh_count(_lib.ptr(u), *dims, thr, _lib.ptr(counts), s), "esr_mesh_count")
        offsets, n_v, n_f = _scan(counts, nb)
        verts = torch.empty(n_v, 3, dtype=torch.float64, device=dev)
        tris = torch.empty(n_f, 3, dtype=torch.int64, device=dev)
        if n_v == 0:
            return verts, tris
        if n_v >= 2 ** 31:
            raise RuntimeError(f"marching_cubes: {n_v} vertices exceed the kernels' 31-bit vertex ids")
        vid = torch.empty(dims, dtype=torch.int32, device=dev)
        _lib.check(L.esr_mesh_emit(_lib.ptr(u), *dims, thr, _lib.ptr(offsets), _lib.ptr(vid), _lib.ptr(verts),
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
