"""A texture atlas of a surface: every face gets a chart of its own, the texels know their face and world point, and a
texture is looked up bilinearly at a point of a face (csrc/atlas.hip, section W of include/esr_hip.h).

``build``   levels (how large a cell each face gets at a texel density) -> one stable sort -> charts (where each face's
            cell lies, its UVs) -> texels (which face, barycentrics and world point every texel has); with
            ``texels_per_unit=None`` the largest density whose cells fit the square is found by bisection on the level pass
``texels``  the texel pass again with vertex attributes: the bake without a model
``sample``  a ``[W, W, C]`` texture at (face, barycentrics) queries, as ``raycast.Hits`` carries them

The layout is all integer: half cells of power-of-two squares in Z-order, largest first.  Limits: per-face charts distort (any
triangle maps to a right isosceles one), spend texels on gutters, make every edge a seam, and there is no mip chain.
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib

MAX_LEVELS = _lib.ATLAS_MAX_LEVELS
MAX_CHANNELS = _lib.ATLAS_MAX_CHANNELS
BISECT_TRIALS = 24


@dataclass
class Atlas:
    size: int                            # W: the atlas is W x W texels
    gutter: int
    lmin: int
    lmax: int
    density: float                       # texels per world unit
    counts: tuple                        # the faces of every level, indexed by the level (MAX_LEVELS entries)
    level: torch.Tensor                  # device int32 [F]
    rot: torch.Tensor                    # device int32 [F]: corners rot, rot + 1, rot + 2 are the chart's a, b, c
    order: torch.Tensor                  # device int64 [F]: the face at every sorted rank
    chart: torch.Tensor                  # device int32 [F, 4]: x0, y0, level | half << 8 | rot << 16, rank
    uv: torch.Tensor                     # device float32 [F, 3, 2]: x / W, y / W of the face's three corners
    face: torch.Tensor                   # device int32 [W, W] (row y, column x): -1 for a texel of no face
    bary: torch.Tensor                   # device float32 [W, W, 2]: the weights of the rotated corners b and c, not clamped
    point: torch.Tensor                  # device float32 [W, W, 3]
    flags: torch.Tensor                  # device uint8 [W, W]: bit 0 = the texel centre is inside its face's triangle


def leg(level: int, gutter: int) -> int:
    return (1 << level) - (3 * gutter + 1)


def _layout(what, size, gutter, lmin, lmax):
    for name, x in (("size", size), ("gutter", gutter)):
        if isinstance(x, bool) or not isinstance(x, int):
            raise ValueError(f"{what}: {name} is an int, got {x!r}")
    if size < _lib.ATLAS_MIN_SIZE or size > _lib.ATLAS_MAX_SIZE or size & (size - 1):
        raise ValueError(f"{what}: size is a power of two from {_lib.ATLAS_MIN_SIZE} to {_lib.ATLAS_MAX_SIZE}, got {size}")
    if gutter < 1:
        raise ValueError(f"{what}: the gutter is at least one texel, got {gutter}")
    low = max(0, (3 * gutter + 1).bit_length())                   # the smallest l with 2^l >= 3 g + 2
    top = size.bit_length() - 1
    lmin = low if lmin is None else lmin
    lmax = top if lmax is None else lmax
    for name, x in (("lmin", lmin), ("lmax", lmax)):
        if isinstance(x, bool) or not isinstance(x, int):
            raise ValueError(f"{what}: {name} is an int, got {x!r}")
    if not low <= lmin <= lmax <= top:
        raise ValueError(f"{what}: {low} <= lmin <= lmax <= {top} for size {size} and gutter {gutter}, got {lmin}, {lmax}")
    return lmin, lmax


def fits(counts, size: int, lmin: int, lmax: int) -> bool:
    """whether the cells of the level counts fit the square (the test of esr_atlas_charts)"""
    unit = sum(((counts[l] + 1) >> 1) << (2 * (l - lmin)) for l in range(lmin, lmax + 1))
    return unit <= (size >> lmin) ** 2


def _geometry(what, vertices, triangles):
    if not isinstance(vertices, torch.Tensor) or not vertices.is_cuda or vertices.dtype != torch.float64 or vertices.dim() != 2 or \
            vertices.shape[1] != 3:
        raise ValueError(f"{what}: vertices must be a device float64 [V, 3] tensor")
    if not isinstance(triangles, torch.Tensor) or triangles.device != vertices.device or triangles.dtype != torch.int64 or \
            triangles.dim() != 2 or triangles.shape[1] != 3:
        raise ValueError(f"{what}: triangles must be an int64 [F, 3] tensor on the vertices' device")
    if vertices.shape[0] >= 2 ** 31 or triangles.shape[0] >= 2 ** 31:
        raise ValueError(f"{what}: the kernels count vertices and faces in 31 bits")
    return vertices.contiguous(), triangles.contiguous()


def _levels(v, t, size, gutter, lmin, lmax, rho, level, rot, hist):
    """the level pass at the density rho -> the counts (one 128-byte read-back)"""
    rho2 = float(rho) * float(rho)
    with torch.cuda.device(v.device):
        _lib.check(_lib.lib().esr_atlas_levels(_lib.ptr(v), int(v.shape[0]), _lib.ptr(t), int(t.shape[0]), size, gutter, lmin, lmax,
                                               rho2 * rho2, _lib.ptr(level), _lib.ptr(rot), _lib.ptr(hist), _lib.stream_ptr(v.device)),
                   "esr_atlas_levels")
    return tuple(int(x) for x in hist.tolist())


@torch.no_grad()
def build(vertices: torch.Tensor, triangles: torch.Tensor, size: int = 2048, gutter: int = 1, texels_per_unit: Optional[float] = None,
          lmin: Optional[int] = None, lmax: Optional[int] = None) -> Atlas:
    """The atlas of the mesh: ``size`` x ``size`` texels, ``gutter`` texels around every chart, cells of 2^lmin .. 2^lmax texels
    (by default the smallest cell the gutter allows up to the whole square).  A face whose area is A gets the smallest cell whose
    usable leg is at least ``texels_per_unit * sqrt(2 A)``.  With ``texels_per_unit=None`` the largest density that fits is
    searched: a geometric bisection of at most 24 trial level passes between the density at which every face has the
    smallest cell and 2^24 times that, and one more pass at the density found.  A layout that does not fit is a ValueError.
    The same input gives the same bytes."""
    what = "atlas.build"
    v, t = _geometry(what, vertices, triangles)
    lmin, lmax = _layout(what, size, gutter, lmin, lmax)
    dev, F = v.device, int(t.shape[0])
    level = torch.zeros(F, dtype=torch.int32, device=dev)
    rot = torch.zeros(F, dtype=torch.int32, device=dev)
    hist = torch.zeros(MAX_LEVELS, dtype=torch.int64, device=dev)
    run = lambda rho: _levels(v, t, size, gutter, lmin, lmax, rho, level, rot, hist)
    if texels_per_unit is not None:
        rho = float(texels_per_unit)
        if not (0.0 <= rho < math.inf) or (rho * rho) * (rho * rho) == math.inf:
            raise ValueError(f"{what}: texels_per_unit is a finite density, got {texels_per_unit!r}")
        counts = run(rho)
        if not fits(counts, size, lmin, lmax):
            raise ValueError(f"{what}: at {rho} texels per unit the {F} faces do not fit {size} x {size} texels")
    else:
        # at leg(lmin) / diagonal texels per unit no face can need more than the smallest cell
        ok = torch.isfinite(v).all(dim=1)
        diag = float(torch.linalg.norm(v[ok].amax(0) - v[ok].amin(0))) if bool(ok.any()) else 0.0
        lo = leg(lmin, gutter) / diag if diag > 0.0 and math.isfinite(diag) else 1.0
        counts = run(lo)
        if not fits(counts, size, lmin, lmax):
            raise ValueError(f"{what}: {F} faces do not fit {size} x {size} texels even in the smallest cells")
        rho, hi = lo, lo * 2.0 ** 24
        if fits(run(hi), size, lmin, lmax):
            rho = hi
        else:
            for _ in range(BISECT_TRIALS - 2):
                mid = math.sqrt(rho * hi)
                if fits(run(mid), size, lmin, lmax):
                    rho = mid
                else:
                    hi = mid
        counts = run(rho)
    order = torch.sort(lmax - level, stable=True).indices.contiguous()
    chart = torch.zeros(F, 4, dtype=torch.int32, device=dev)
    uv = torch.zeros(F, 3, 2, dtype=torch.float32, device=dev)
    host = (ctypes.c_int64 * MAX_LEVELS)(*counts)
    with torch.cuda.device(dev):
        code = _lib.lib().esr_atlas_charts(F, _lib.ptr(order), _lib.ptr(rot), host, size, gutter, lmin, lmax, _lib.ptr(chart),
                                           _lib.ptr(uv), _lib.stream_ptr(dev))
    _lib.check(code, "esr_atlas_charts")
    atlas = Atlas(size, gutter, lmin, lmax, rho, counts, level, rot, order, chart, uv, None, None, None, None)
    atlas.face, atlas.bary, atlas.point, atlas.flags, _ = texels(atlas, v, t)
    return atlas


@torch.no_grad()
def texels(atlas: Atlas, vertices: torch.Tensor, triangles: torch.Tensor, attr: Optional[torch.Tensor] = None):
    """The texel pass of ``atlas`` over the mesh it was built from -> (face, bary, point, flags, tex).  With ``attr`` float32
    [V, C], C <= 16, ``tex`` float32 [W, W, C] holds the vertex attributes interpolated (and, in the gutter, extrapolated) with
    float32 weights; else None."""
    what = "atlas.texels"
    v, t = _geometry(what, vertices, triangles)
    dev, W, F = v.device, atlas.size, int(t.shape[0])
    if atlas.order.device != dev or atlas.order.shape[0] != F:
        raise ValueError(f"{what}: the atlas was built from another mesh")
    C, tex = 0, None
    if attr is not None:
        if not isinstance(attr, torch.Tensor) or attr.device != dev or attr.dtype != torch.float32 or attr.dim() != 2 or \
                attr.shape[0] != v.shape[0] or not 1 <= attr.shape[1] <= MAX_CHANNELS:
            raise ValueError(f"{what}: attr must be a float32 [V, C] tensor on the mesh's device, C <= {MAX_CHANNELS}")
        attr = attr.contiguous()
        C = int(attr.shape[1])
        tex = torch.empty(W, W, C, dtype=torch.float32, device=dev)
    # (the pass writes every texel of every output: nothing to clear first)
    face = torch.empty(W, W, dtype=torch.int32, device=dev)
    bary = torch.empty(W, W, 2, dtype=torch.float32, device=dev)
    point = torch.empty(W, W, 3, dtype=torch.float32, device=dev)
    flags = torch.empty(W, W, dtype=torch.uint8, device=dev)
    host = (ctypes.c_int64 * MAX_LEVELS)(*atlas.counts)
    with torch.cuda.device(dev):
        code = _lib.lib().esr_atlas_texels(_lib.ptr(v), int(v.shape[0]), _lib.ptr(t), F, _lib.ptr(atlas.order), _lib.ptr(atlas.rot), host,
                                           W, atlas.gutter, atlas.lmin, atlas.lmax, _lib.ptr(attr), C, _lib.ptr(face), _lib.ptr(bary),
                                           _lib.ptr(point), _lib.ptr(flags), _lib.ptr(tex), _lib.stream_ptr(dev))
    _lib.check(code, "esr_atlas_texels")
    return face, bary, point, flags, tex


@torch.no_grad()
def sample(atlas: Atlas, texture: torch.Tensor, face: torch.Tensor, bary: torch.Tensor) -> torch.Tensor:
    """``texture`` float32 [W, W, C] (or [W, W]), C <= 16, looked up bilinearly at the points of the faces ``face`` int32 [N]
    with the barycentrics ``bary`` [N, 2] (the weights of the face's second and third corner, as ``raycast.Hits`` carries
    them).  -> float32 [N, C] (or [N]); 0 where ``face`` is -1."""
    what = "atlas.sample"
    dev, W = atlas.uv.device, atlas.size
    if not isinstance(texture, torch.Tensor) or texture.device != dev or texture.dtype != torch.float32 or texture.dim() not in (2, 3) or \
            tuple(texture.shape[:2]) != (W, W):
        raise ValueError(f"{what}: the texture must be a float32 [{W}, {W}, C] tensor on the atlas's device")
    flat = texture.dim() == 2
    tex = texture.reshape(W, W, -1).contiguous()
    C = int(tex.shape[2])
    if not 1 <= C <= MAX_CHANNELS:
        raise ValueError(f"{what}: 1 .. {MAX_CHANNELS} channels, got {C}")
    if not isinstance(face, torch.Tensor) or face.device != dev or face.dtype != torch.int32 or face.dim() != 1:
        raise ValueError(f"{what}: face must be an int32 [N] tensor on the atlas's device")
    N = int(face.shape[0])
    if not isinstance(bary, torch.Tensor) or bary.device != dev or bary.dtype not in (torch.float32, torch.float64) or \
            tuple(bary.shape) != (N, 2):
        raise ValueError(f"{what}: bary must be a float [N, 2] tensor on the atlas's device")
    if N >= 2 ** 31:
        raise ValueError(f"{what}: {N} queries exceed the kernel's 31-bit count")
    out = torch.zeros(N, C, dtype=torch.float32, device=dev)
    if N:
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().esr_atlas_sample(_lib.ptr(atlas.uv), int(atlas.uv.shape[0]), W, _lib.ptr(tex), C, N,
                                                   _lib.ptr(face.contiguous()), _lib.ptr(bary.double().contiguous()), _lib.ptr(out),
                                                   _lib.stream_ptr(dev)), "esr_atlas_sample")
    return out[:, 0] if flat else out


__all__ = ["Atlas", "build", "texels", "sample", "fits", "leg"]
