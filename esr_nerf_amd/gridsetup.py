"""Stage hand-over on the device (esr_nerf_amd/csrc/gridsetup.hip): what runs when one stage gives its grids to the next.

``resample_grid``     trilinear, align_corners=True, on the channels-last memory ``DenseGrid.device_view()`` hands out
                      (``DenseGrid.scale_volume_grid``, ``checkpoint.fine_from_coarse``)
``maxpool3d``         ``F.max_pool3d(kernel_size=ks, padding=ks // 2, stride=1)`` of ``MaskCache.__init__``
``nonempty_mask``     ``MaskCache.forward`` at every node of an SDF grid, the SDF pinned to 1 outside (``set_nonempty_mask``)
``density_bounds``    the bounding box of an alphamask density's active nodes (``compute_bbox_by_coarse_geo``,
                      app/coarse/coarse.py:152-182; ``checkpoint.coarse_from_alphamask``)

Every function runs on the current stream of its tensors' device and is not waited for, except ``density_bounds``, whose
answer the host needs.  There is no CPU kernel: every function here raises on CPU tensors (the callers keep their torch
lines for CPU-resident models).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import torch

from . import _lib


def _need_device(what: str, *tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError(f"{what} runs on libesr_hip.so and needs device tensors (there is no CPU kernel)")


def _f32(what: str, *tensors):
    for t in tensors:
        if t is not None and t.dtype != torch.float32:
            raise ValueError(f"{what}: tensors are float32, got {t.dtype}")


def _box(lo_hi) -> "C.Array":
    """(c_float * 6) from six numbers, or from a (min, max) pair of 3-vectors (tensors, lists)"""
    if len(lo_hi) == 2:
        lo_hi = [*(lo_hi[0].tolist() if torch.is_tensor(lo_hi[0]) else lo_hi[0]),
                 *(lo_hi[1].tolist() if torch.is_tensor(lo_hi[1]) else lo_hi[1])]
    if len(lo_hi) != 6:
        raise ValueError(f"a box is six numbers (min xyz, max xyz) or a (min, max) pair, got {len(lo_hi)} values")
    return (C.c_float * 6)(*[float(v) for v in lo_hi])


@torch.no_grad()
def resample_grid(view: torch.Tensor, size: Sequence[int]) -> torch.Tensor:
    """``view`` [X,Y,Z,C] (or [X,Y,Z]) contiguous float32 -> a new [*size, C] (or [*size]) tensor: trilinear, align_corners."""
    _need_device("resample_grid", view)
    _f32("resample_grid", view)
    if view.dim() not in (3, 4) or not view.is_contiguous():
        raise ValueError(f"resample_grid: a contiguous [X,Y,Z,C] or [X,Y,Z] tensor, got {tuple(view.shape)}")
    ch = int(view.shape[3]) if view.dim() == 4 else 1
    size = tuple(int(v) for v in size)
    if len(size) != 3 or min(size) < 1 or not 1 <= ch <= _lib.RESAMPLE_MAX_C or min(view.shape[:3]) < 1:
        raise ValueError(f"resample_grid: {tuple(view.shape)} -> {size}: sizes >= 1 and 1 .. {_lib.RESAMPLE_MAX_C} channels")
    dev = view.device
    with torch.cuda.device(dev):
        out = torch.empty(*size, *view.shape[3:], dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().esr_grid_resample(_lib.ptr(view), *[int(v) for v in view.shape[:3]], ch, _lib.ptr(out), *size,
                                                _lib.stream_ptr(dev)), "esr_grid_resample")
    return out


@torch.no_grad()
def maxpool3d(density: torch.Tensor, ks: int) -> torch.Tensor:
    """``F.max_pool3d(density, kernel_size=ks, padding=ks // 2, stride=1)`` of a 1-channel volume ([1,1,X,Y,Z] or [X,Y,Z]);
    ``ks`` odd, 1 .. 7.  Returns a new contiguous tensor of the input's shape."""
    _need_device("maxpool3d", density)
    _f32("maxpool3d", density)
    ks = int(ks)
    if ks < 1 or ks > 7 or ks % 2 == 0:
        raise NotImplementedError(f"esr_maxpool3d supports odd kernel sizes 1 .. 7, got {ks}")
    if density.dim() == 5 and tuple(density.shape[:2]) == (1, 1):
        dims = tuple(int(v) for v in density.shape[2:])
    elif density.dim() == 3:
        dims = tuple(int(v) for v in density.shape)
    else:
        raise ValueError(f"maxpool3d: a [1,1,X,Y,Z] or [X,Y,Z] volume, got {tuple(density.shape)}")
    dev = density.device
    with torch.cuda.device(dev):
        src = density.contiguous()
        out = torch.empty_like(src)
        _lib.check(_lib.lib().esr_maxpool3d(_lib.ptr(src), *dims, ks, _lib.ptr(out), _lib.stream_ptr(dev)), "esr_maxpool3d")
    return out


@torch.no_grad()
def nonempty_mask(pooled: torch.Tensor, mask_box, act_shift: float, thres: float, axes: Sequence[torch.Tensor],
                  sdf: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(mask, count)``: ``mask`` bool [X,Y,Z] = the mask cache's decision (``MaskCache.forward``) at the nodes
    ``(axes[0][i], axes[1][j], axes[2][k])``; ``count`` int64 [1] on the device = ``mask.sum()``.  ``pooled``: the cache's
    max-pooled density ([1,1,mx,my,mz] or [mx,my,mz]) in the box ``mask_box``.  ``sdf`` (any shape of X*Y*Z contiguous
    floats) is set to 1 where the mask is false, in place."""
    axes = [a.contiguous() for a in axes]
    _need_device("nonempty_mask", pooled, *axes, sdf)
    _f32("nonempty_mask", pooled, *axes, sdf)
    if len(axes) != 3 or any(a.dim() != 1 or a.numel() < 1 for a in axes):
        raise ValueError("nonempty_mask: three non-empty axis vectors")
    n = tuple(int(a.numel()) for a in axes)
    mdims = tuple(int(v) for v in pooled.shape[-3:])
    if pooled.numel() != mdims[0] * mdims[1] * mdims[2]:
        raise ValueError(f"nonempty_mask: a 1-channel pooled density, got {tuple(pooled.shape)}")
    if sdf is not None and (sdf.numel() != n[0] * n[1] * n[2] or not sdf.is_contiguous()):
        raise ValueError(f"nonempty_mask: the SDF grid holds {sdf.numel()} values, its axes {n}")
    dev = pooled.device
    box = _box(mask_box)
    with torch.cuda.device(dev):
        mask = torch.empty(n, dtype=torch.uint8, device=dev)
        count = torch.zeros(1, dtype=torch.int64, device=dev)
        _lib.check(_lib.lib().esr_nonempty_mask(
            _lib.ptr(pooled.contiguous()), *mdims, box, float(act_shift), float(thres), *[_lib.ptr(a) for a in axes], *n,
            _lib.ptr(sdf), _lib.ptr(mask), _lib.ptr(count), _lib.stream_ptr(dev)), "esr_nonempty_mask")
    return mask.view(torch.bool), count


def bounds_axes(lo: torch.Tensor, hi: torch.Tensor, dims: Sequence[int]):
    """The per-axis coordinates of coarse.py:154-168: ``lo * (1 - t) + hi * t`` over ``t = linspace(0, 1, n)`` (the
    reference's ``dense_xyz`` is separable per axis, so three vectors hold the same floats)."""
    out = []
    for a, n in enumerate(dims):
        t = torch.linspace(0, 1, int(n), device=lo.device)
        out.append(lo[a] * (1 - t) + hi[a] * t)
    return out


@torch.no_grad()
def density_bounds(density: torch.Tensor, box, act_shift: float, thres: float):
    """``(xyz_min, xyz_max)`` float32 [3] on the device: the bounding box of the nodes of ``density`` ([1,1,X,Y,Z] or [X,Y,Z],
    in the box ``box`` = (xyz_min, xyz_max)) whose alpha ``1 - exp(-softplus(d + act_shift))`` exceeds ``thres``
    (compute_bbox_by_coarse_geo, coarse.py:152-182).  Raises ``ValueError`` when no node is active (where the reference's
    ``amin`` of an empty tensor raises).  One read-back."""
    _need_device("density_bounds", density)
    _f32("density_bounds", density)
    dims = tuple(int(v) for v in density.shape[-3:])
    if density.numel() != dims[0] * dims[1] * dims[2] or min(dims) < 1:
        raise ValueError(f"density_bounds: a 1-channel density, got {tuple(density.shape)}")
    dev = density.device
    lo, hi = (torch.as_tensor(v, dtype=torch.float32).to(dev) for v in box)
    with torch.cuda.device(dev):
        axes = bounds_axes(lo, hi, dims)
        part = torch.empty(_lib.DENSITY_BOUNDS_BLOCKS * 6, dtype=torch.float32, device=dev)
        out = torch.empty(6, dtype=torch.float32, device=dev)
        count = torch.zeros(1, dtype=torch.int64, device=dev)
        _lib.check(_lib.lib().esr_density_bounds(
            _lib.ptr(density.contiguous()), *dims, _box((lo, hi)), float(act_shift), float(thres),
            *[_lib.ptr(a) for a in axes], _lib.ptr(part), _lib.ptr(out), _lib.ptr(count), _lib.stream_ptr(dev)),
            "esr_density_bounds")
        if int(count) == 0:
            raise ValueError(f"density_bounds: no node of the density has alpha > {thres}")
    return out[:3].clone(), out[3:].clone()
