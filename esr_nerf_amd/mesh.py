"""Mesh export on the device: the reference's ``extract_geometry`` (app/fine/model/voxurff.py:745-780) over
libesr_hip.so's esr_mesh_* kernels (esr_nerf_amd/csrc/mesh.hip).

``sdf_field``       the -sdf lattice field (optional Gaussian smoothing with esr_gauss3d_fwd, then esr_mesh_field)
``marching_cubes``  count -> scan -> emit; vertices in index space, triangles as vertex ids, both on the device
``extract_geometry`` world-space numpy arrays, what the reference returns

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
