"""Rays against the exported surface: a linear BVH over the faces, built on the device, and a nearest-hit / any-hit walk
(csrc/bvh.hip; the definition is section T of include/esr_hip.h, the restatement tests/raycast_ref.py).

``build``              the face keys and boxes (esr_bvh_keys), torch's stable sort, the radix tree (esr_bvh_tree) and the node
                       boxes (esr_bvh_fit) -> ``Bvh``, device tensors only
``cast``               the nearest hit of every ray: face, t (in units of d), two barycentrics
``occluded``           any hit inside (t_min, t_max], one byte per ray
``occluded_segments``  any hit strictly inside the segment p -> q: eps < t <= 1 - eps of d = q - p
``cast_cameras``       the pixel rays of ``camera.Cameras`` views, built in float64 from the binary32 camera with d's
                       camera-space z equal to 1, so that t is the camera depth ``raster.rasterize`` stores

Nothing here reads anything back from the device; the answer is a function of the input alone.
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass
from typing import NamedTuple, Optional

import torch

from . import _lib
from .mesh import _check_mesh

NODE_WORDS = ctypes.sizeof(_lib.EsrBvhNode) // 4   # an esr_bvh_node_t as int32 words: 12 of boxes, child[2], parent, pad


@dataclass
class Bvh:
    vertices: torch.Tensor               # device float64 [V, 3]
    triangles: torch.Tensor              # device int64 [F, 3]
    nodes: torch.Tensor                  # device int32 [max(F - 1, 0), 16]: esr_bvh_node_t records
    order: torch.Tensor                  # device int64 [F]: the face id at every sorted position
    keys: torch.Tensor                   # device int64 [F]: the sorted Morton keys
    face_boxes: torch.Tensor             # device float32 [F, 6]: every face's box, rounded outward
    leaf_parent: torch.Tensor            # device int32 [F]: 2 * parent + side of the leaf at every sorted position
    scene_box: torch.Tensor              # device float64 [6]: lo, hi of the finite vertices (the keys' frame)
    root_box: torch.Tensor               # device float32 [6]: the box of the whole tree

    @property
    def n_faces(self) -> int:
        return int(self.triangles.shape[0])


class Hits(NamedTuple):
    face: torch.Tensor                   # int32 [N]: -1 for none
    t: torch.Tensor                      # float64 [N]: +inf for none
    bary: torch.Tensor                   # float64 [N, 2]: the weights of the face's second and third vertex
    stats: Optional[torch.Tensor] = None  # int32 [N, 2]: boxes tested, triangles tested


def _check_geometry(what, vertices, triangles):
    if not isinstance(vertices, torch.Tensor) or not vertices.is_cuda or vertices.dtype != torch.float64 or \
            vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError(f"{what}: vertices must be a float64 [V, 3] device tensor")
    tris, n_v = _check_mesh(what, triangles, vertices.shape[0])
    if tris.device != vertices.device:
        raise ValueError(f"{what}: vertices and triangles are on one device")
    if tris.shape[0] >= 2 ** 31 or n_v >= 2 ** 31:
        raise ValueError(f"{what}: {tris.shape[0]} faces on {n_v} vertices exceed the kernels' 31-bit ids")
    return vertices.contiguous(), tris


@torch.no_grad()
def build(vertices: torch.Tensor, triangles: torch.Tensor) -> Bvh:
    """The BVH of a mesh (``vertices`` device float64 [V, 3], ``triangles`` device int64 [F, 3]).  A face with a vertex that
    is not finite stays in the tree with an empty box and is never hit.  No read-back."""
    return _build(vertices, triangles)


def _build(vertices, triangles, alloc=None):
    """``build``; ``alloc(shape, dtype)`` allocates every buffer a kernel writes (for the tests)"""
    verts, tris = _check_geometry("raycast.build", vertices, triangles)
    dev, n_v, n_f = verts.device, int(verts.shape[0]), int(tris.shape[0])
    if alloc is None:
        def alloc(shape, dtype):
            return torch.empty(shape, dtype=dtype, device=dev)
    L = _lib.lib()
    with torch.cuda.device(dev):
        s = _lib.stream_ptr(dev)
        inf = torch.full((1, 3), math.inf, dtype=torch.float64, device=dev)
        ok = torch.isfinite(verts).all(1, keepdim=True)
        scene = torch.cat([torch.cat([torch.where(ok, verts, inf), inf]).amin(0),
                           torch.cat([torch.where(ok, verts, -inf), -inf]).amax(0)]).contiguous()
        keys, boxes = alloc((n_f,), torch.int64), alloc((n_f, 6), torch.float32)
        _lib.check(L.esr_bvh_keys(_lib.ptr(verts), n_v, _lib.ptr(tris), n_f, _lib.ptr(scene), _lib.ptr(keys), _lib.ptr(boxes), s),
                   "esr_bvh_keys")
        skeys, order = torch.sort(keys, stable=True)               # equal keys keep the order of their face ids
        skeys, order = skeys.contiguous(), order.contiguous()
        nodes = alloc((max(n_f - 1, 0), NODE_WORDS), torch.int32)
        leaf_parent = alloc((n_f,), torch.int32)
        counters = alloc((max(n_f - 1, 0),), torch.int32)
        root_box = alloc((6,), torch.float32)
        _lib.check(L.esr_bvh_tree(_lib.ptr(skeys), _lib.ptr(order), n_f, _lib.ptr(nodes), _lib.ptr(leaf_parent), s), "esr_bvh_tree")
        if n_f == 1:
            leaf_parent.fill_(-1)
        if n_f == 0:
            root_box.copy_(torch.tensor([math.inf] * 3 + [-math.inf] * 3, dtype=torch.float32, device=dev))
        _lib.check(L.esr_bvh_fit(_lib.ptr(nodes), _lib.ptr(leaf_parent), _lib.ptr(order), _lib.ptr(boxes), n_f,
                                 _lib.ptr(counters), _lib.ptr(root_box), s), "esr_bvh_fit")
    return Bvh(verts, tris, nodes, order, skeys, boxes, leaf_parent, scene, root_box)


def _rays(what, bvh, rays_o, rays_d):
    dev = bvh.vertices.device
    for name, x in (("rays_o", rays_o), ("rays_d", rays_d)):
        if not isinstance(x, torch.Tensor) or x.device != dev or x.dtype not in (torch.float32, torch.float64) or \
                x.dim() != 2 or x.shape[1] != 3:
            raise ValueError(f"{what}: {name} must be a float32 or float64 [N, 3] tensor on the mesh's device")
    if rays_o.shape[0] != rays_d.shape[0]:
        raise ValueError(f"{what}: {rays_o.shape[0]} origins and {rays_d.shape[0]} directions")
    if rays_o.shape[0] >= 2 ** 31:
        raise ValueError(f"{what}: {rays_o.shape[0]} rays exceed the kernel's 31-bit count")
    return rays_o.double().contiguous(), rays_d.double().contiguous()      # (binary32 widens exactly)


def _interval(what, n, dev, value, name):
    """-> (per-ray tensor or None, scalar)"""
    if isinstance(value, torch.Tensor):
        if value.device != dev or value.shape != (n,) or value.dtype not in (torch.float32, torch.float64):
            raise ValueError(f"{what}: {name} must be a number or a float [N] tensor on the mesh's device")
        return value.double().contiguous(), 0.0
    return None, float(value)


def _skip(what, n, dev, skip_face):
    if skip_face is None:
        return None
    if not isinstance(skip_face, torch.Tensor) or skip_face.device != dev or skip_face.shape != (n,) or \
            skip_face.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{what}: skip_face must be an int32 [N] tensor on the mesh's device")
    return skip_face.to(torch.int32).contiguous()


def _cast(what, bvh, rays_o, rays_d, t_min, t_max, skip_face, any_hit, stats=False, alloc=None):
    o, d = _rays(what, bvh, rays_o, rays_d)
    dev, n = o.device, int(o.shape[0])
    lo, lo_all = _interval(what, n, dev, t_min, "t_min")
    hi, hi_all = _interval(what, n, dev, t_max, "t_max")
    skip = _skip(what, n, dev, skip_face)
    if alloc is None:
        def alloc(shape, dtype):
            return torch.empty(shape, dtype=dtype, device=dev)
    L = _lib.lib()
    with torch.cuda.device(dev):
        face = t = bary = hit = None
        if any_hit:
            hit = alloc((n,), torch.uint8)
        else:
            face, t, bary = alloc((n,), torch.int32), alloc((n,), torch.float64), alloc((n, 2), torch.float64)
        st = alloc((n, 2), torch.int32) if stats else None
        _lib.check(L.esr_bvh_cast(_lib.ptr(bvh.nodes), bvh.n_faces, _lib.ptr(bvh.vertices), int(bvh.vertices.shape[0]),
                                  _lib.ptr(bvh.triangles), _lib.ptr(o), _lib.ptr(d), n, _lib.ptr(lo), _lib.ptr(hi), lo_all, hi_all,
                                  _lib.ptr(skip), 1 if any_hit else 0, _lib.ptr(face), _lib.ptr(t), _lib.ptr(bary), _lib.ptr(hit),
                                  _lib.ptr(st), _lib.stream_ptr(dev)), "esr_bvh_cast")
    return (hit, st) if any_hit else Hits(face, t, bary, st)


@torch.no_grad()
def cast(bvh: Bvh, rays_o, rays_d, t_min=0.0, t_max=math.inf, skip_face=None, stats: bool = False) -> Hits:
    """The nearest hit of every ray ``o + t d`` with ``t_min < t <= t_max`` (numbers or per-ray tensors; ``d`` is not
    normalised): Moeller-Trumbore in float64, both windings, all three barycentrics >= 0; a determinant of exactly 0 is no
    hit; among equal ``t`` the smaller face id.  ``skip_face`` int32 [N]: a face the ray never hits (-1: none).  float32
    rays are widened exactly.  A ray with a component that is not finite hits nothing.  ``stats`` adds int32 [N, 2]: boxes
    and triangles tested."""
    return _cast("raycast.cast", bvh, rays_o, rays_d, t_min, t_max, skip_face, False, stats)


@torch.no_grad()
def occluded(bvh: Bvh, rays_o, rays_d, t_min, t_max, skip_face=None) -> torch.Tensor:
    """uint8 [N]: 1 iff ``cast`` with the same interval would hit a face; the walk ends at the first hit"""
    return _cast("raycast.occluded", bvh, rays_o, rays_d, t_min, t_max, skip_face, True)[0]


@torch.no_grad()
def occluded_segments(bvh: Bvh, p, q, skip_face=None, eps: float = 1e-6) -> torch.Tensor:
    """uint8 [N]: 1 iff a face is hit strictly between ``p`` and ``q``: the ray is p -> q with d = q - p (float64, one
    rounding) and t in (eps, 1 - eps]"""
    o, e = _rays("raycast.occluded_segments", bvh, p, q)
    return _cast("raycast.occluded_segments", bvh, o, e - o, float(eps), 1.0 - float(eps), skip_face, True)[0]


def pixel_rays(cams, views=None):
    """(o, d, v): o, d float64 [v * H * W, 3] of the pixels of the views in row order: o = the pose's translation,
    d = px R[:, 0] + py R[:, 1] + R[:, 2] with px = ((i + 0.5) - cx) / fx, py = ((j + 0.5) - cy) / fy, all in float64 from
    the binary32 camera"""
    from .raster import _view_range
    v0, v1 = _view_range(cams, views)
    dev = cams.device
    m = cams.poses[v0:v1].double()                                        # [v, 3, 4]
    # (the focal lengths as tensors: a division by a Python number is a product with its reciprocal on the device)
    fx, fy = (torch.tensor(f, dtype=torch.float64, device=dev) for f in (cams.fx, cams.fy))
    px = ((torch.arange(cams.width, dtype=torch.float64, device=dev) + 0.5) - cams.cx) / fx
    py = ((torch.arange(cams.height, dtype=torch.float64, device=dev) + 0.5) - cams.cy) / fy
    d = (px[None, None, :, None] * m[:, None, None, :, 0] + py[None, :, None, None] * m[:, None, None, :, 1]) + m[:, None, None, :, 2]
    o = m[:, None, None, :, 3].expand_as(d)
    return o.reshape(-1, 3).contiguous(), d.reshape(-1, 3).contiguous(), v1 - v0


@torch.no_grad()
def cast_cameras(bvh: Bvh, cams, views=None):
    """-> (face int32 [v, H, W], depth float64 [v, H, W]) of the views ``views`` (as ``raster.rasterize`` takes them): the
    nearest face along every pixel's ray and its camera depth, +inf where there is none.  Any fx, fy, cx, cy."""
    if cams.device != bvh.vertices.device:
        raise ValueError("raycast.cast_cameras: the mesh and the cameras are on one device")
    o, d, n = pixel_rays(cams, views)
    h = cast(bvh, o, d)
    return h.face.reshape(n, cams.height, cams.width), h.t.reshape(n, cams.height, cams.width)


__all__ = ["Bvh", "Hits", "build", "cast", "occluded", "occluded_segments", "pixel_rays", "cast_cameras"]
