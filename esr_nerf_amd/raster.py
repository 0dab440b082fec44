"""The exported surface projected into camera views: per pixel the face in front, its depth, and the image masks of the
emissive sources -- the link between ``sources.emissive_sources`` (sources in 3-D, a source id per face) and
``relight.EditRaySelector`` / ``finetune_radiance`` (sources as per-view masks, ``test_data["em_masks"]``).

The reference reads those masks from the synthetic dataset's annotations (data/esrnerf/esrnerf.py: ``areas``, ``em_masks``)
or renders ``any(lin/emit > k_val)`` (app/fine/pdra.py:684-688), which names no source and costs a volumetric render; a
user's own capture has neither.  Here a z-buffer rasteriser (esr_nerf_amd/csrc/raster.hip) does it from the mesh.

``rasterize``        ``face`` / ``depth`` / ``n_dropped`` of a mesh in all or some views of a ``camera.Cameras``
``source_masks``     per view and edit condition the 0/1 mask of the pixels that see one of its sources, and the visible
                     pixels of every source
``edit_view_data``   the ``test_data`` dictionary of one view that ``EditRaySelector.apply`` and ``finetune_radiance`` take

Limits.  There is no near-plane clipping: a face with a vertex at camera depth <= ``z_near`` is dropped whole and counted
in ``n_dropped``, which says when that bit.  No anti-aliasing: a pixel is its centre.  There is no CPU kernel: every
function here raises on CPU tensors.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .camera import BLENDER2OPENCV, Cameras, _need_device
from .mesh import _check_mesh
from .relight import LIGHT_MODES, MAX_CONDITIONS

Z_NEAR = 1e-6
# A face whose clamped bounding box holds more pixel centres than this is rasterised by a workgroup instead of one lane.
# Measured (tools/raster_time.py, profiles/raster_time.json, 800 x 800): a 512^3 surface queues nothing from 16 up and
# costs the same for every value; a 64^3 surface of ~100-pixel faces is fastest from 256 up (a workgroup per such face
# costs more than one lane's loop), so 256 -- the largest value that still keeps a lane's loop to a few hundred pixels.
BIG_PX = 256
CHUNK_BYTES = 256 << 20                    # most bytes of z-buffer words plus queue entries alive at once
EDIT_MODES = ("off", "i_change", "c_change", "ic_change")


@dataclass
class Raster:
    face: torch.Tensor                     # device int32 [v, H, W]: the face in front at each pixel centre, -1 where none
    depth: torch.Tensor                    # device float32 [v, H, W]: its camera-space z (the ray parameter), +inf where none
    n_dropped: torch.Tensor                # device int32 [v]: faces dropped for a vertex at camera depth <= z_near


def world_to_camera(cams: Cameras) -> np.ndarray:
    """[V, 12] float64: per view the first three rows of the float64 inverse of its 4 x 4 camera-to-world matrix (the
    float32 pose, exactly).  A point on a ray of csrc/camera_ray.h then projects back to that ray's pixel even where the
    pose's rotation is not exactly orthonormal."""
    p = cams.poses.detach().cpu().numpy().astype(np.float64)
    m = np.zeros((p.shape[0], 4, 4))
    m[:, :3, :] = p
    m[:, 3, 3] = 1.0
    return np.ascontiguousarray(np.linalg.inv(m)[:, :3, :].reshape(-1, 12)) if p.shape[0] else np.zeros((0, 12))


def blender_pose(cams: Cameras, view: int) -> torch.Tensor:
    """[4, 4] float32, on the cameras' device: the pose of ``view`` back in the loader's Blender convention, as
    ``relight.label_edit_rays`` takes it.  ``Cameras.from_blender`` stores ``float32(matrix) @ blender2opencv``; the flip
    is its own inverse and only changes signs, so this returns ``float32(matrix)`` exactly."""
    view = int(view)
    if not 0 <= view < cams.n_views:
        raise ValueError(f"view {view} of a set of {cams.n_views}")
    dev = cams.device
    pose = torch.cat([cams.poses[view], torch.tensor([[0.0, 0.0, 0.0, 1.0]], dtype=torch.float32, device=dev)], 0)
    return pose * torch.tensor(BLENDER2OPENCV, dtype=torch.float32, device=dev).diagonal()[None, :]


def _view_range(cams: Cameras, views):
    if views is None:
        v0, v1 = 0, cams.n_views
    elif isinstance(views, int):
        v0, v1 = views, views + 1
    elif isinstance(views, range) and views.step == 1:
        v0, v1 = views.start, views.stop
    else:
        v0, v1 = (int(v) for v in views)
    if not 0 <= v0 <= v1 <= cams.n_views:
        raise ValueError(f"rasterize: views [{v0}, {v1}) of a set of {cams.n_views}")
    return v0, v1


@torch.no_grad()
def rasterize(vertices: torch.Tensor, triangles: torch.Tensor, cams: Cameras, views=None, z_near: float = Z_NEAR,
              big_px: Optional[int] = None) -> Raster:
    """Z-buffer of the mesh (``vertices`` float64 [Nv, 3] in world space, ``triangles`` int64 [F, 3], both on the cameras'
    device) in the views ``views`` of ``cams``: None = all, an int = that view, a ``range`` / ``(v0, v1)`` = v0 .. v1 - 1.
    The definition -- float64 projection, inclusive edges, both windings, perspective-correct depth rounded once to
    float32, nearest face and on equal depth the smaller id -- is the header of csrc/raster.hip; the result is a function
    of the input alone.  Nothing is read back.

    Views are processed in chunks: a chunk holds an 8-byte word per pixel and an 8-byte queue entry per face for each of
    its views, and takes as many views as keep that under ``CHUNK_BYTES`` (256 MiB), at least one.  The result does not
    depend on the chunking."""
    _need_device("rasterize", cams.poses, vertices, triangles)
    if vertices.dtype != torch.float64 or vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError(f"rasterize: vertices must be a float64 [Nv, 3] device tensor, got {vertices.dtype} {tuple(vertices.shape)}")
    tris, n_v = _check_mesh("rasterize", triangles, vertices.shape[0])
    dev = cams.device
    if vertices.device != dev or tris.device != dev:
        raise ValueError("rasterize: the mesh and the cameras are on one device")
    z_near = float(z_near)
    if not (0.0 < z_near < float("inf")):
        raise ValueError(f"rasterize: z_near must be positive and finite, got {z_near}")
    big_px = BIG_PX if big_px is None else int(big_px)
    if big_px < 0:
        raise ValueError(f"rasterize: big_px must not be negative, got {big_px}")
    v0, v1 = _view_range(cams, views)
    verts = vertices.contiguous()
    n_f, n_px, n = int(tris.shape[0]), cams.width * cams.height, v1 - v0
    per_view = 8 * (n_px + n_f)
    step = min(max(1, CHUNK_BYTES // per_view), max(n, 1))
    cam = cams.struct()
    L = _lib.lib()
    with torch.cuda.device(dev):
        s = _lib.stream_ptr(dev)
        face = torch.empty(n, cams.height, cams.width, dtype=torch.int32, device=dev)
        depth = torch.empty(n, cams.height, cams.width, dtype=torch.float32, device=dev)
        dropped = torch.empty(n, dtype=torch.int32, device=dev)
        if n == 0:
            return Raster(face, depth, dropped)
        w2c = torch.from_numpy(world_to_camera(cams)).to(dev)
        zbuf = torch.empty(step * n_px, dtype=torch.int64, device=dev)
        queue = torch.empty(max(step * n_f, 1), dtype=torch.int64, device=dev)
        count = torch.empty(1, dtype=torch.int64, device=dev)
        for a in range(v0, v1, step):
            b = min(a + step, v1)
            _lib.check(L.esr_raster_faces(C.byref(cam), _lib.ptr(w2c), a, b, _lib.ptr(verts), n_v, _lib.ptr(tris), n_f, z_near,
                                          big_px, _lib.ptr(zbuf), _lib.ptr(dropped[a - v0:b - v0]), _lib.ptr(queue),
                                          int(queue.numel()), _lib.ptr(count), s), "esr_raster_faces")
            _lib.check(L.esr_raster_resolve(_lib.ptr(zbuf), (b - a) * n_px, _lib.ptr(face[a - v0:b - v0]),
                                            _lib.ptr(depth[a - v0:b - v0]), s), "esr_raster_resolve")
    return Raster(face, depth, dropped)


def _conditions(n_sources: int, groups: Sequence[Sequence[int]]) -> np.ndarray:
    """cond_of_source int32 [S]: the condition (group) each source belongs to, -1 for a source in none"""
    n_sources = int(n_sources)
    if n_sources < 0:
        raise ValueError(f"source_masks: {n_sources} sources")
    if len(groups) > MAX_CONDITIONS:
        raise ValueError(f"source_masks: {len(groups)} conditions; a view takes at most {MAX_CONDITIONS}")
    cond = np.full(n_sources, -1, np.int32)
    for c, group in enumerate(groups):
        for src in group:
            if isinstance(src, bool) or int(src) != src or not 0 <= int(src) < n_sources:
                raise ValueError(f"source_masks: source {src!r} of condition {c} is not one of the {n_sources} sources")
            if cond[int(src)] >= 0:
                raise ValueError(f"source_masks: source {int(src)} is listed twice (conditions {cond[int(src)]} and {c})")
            cond[int(src)] = c
    return cond


@torch.no_grad()
def source_masks(face: torch.Tensor, face_source: torch.Tensor, n_sources: int, groups: Sequence[Sequence[int]]):
    """``face`` int32 [v, H, W] (``rasterize``), ``face_source`` int32 [F] (``SourceReport.face_source``), ``groups``: one
    list of source ids per edit condition.  -> ``(masks, pixels)``: masks float32 [v, n_cond, H, W], 1 where the pixel
    sees a source of that condition (an occluded source is not seen); pixels int64 [v, S], the visible pixels of every
    source, grouped or not.  A source in two groups, or an id outside [0, n_sources), raises ``ValueError``."""
    cond = _conditions(n_sources, groups)
    _need_device("source_masks", face, face_source)
    if face.dtype != torch.int32 or face.dim() != 3:
        raise ValueError(f"source_masks: face must be an int32 [v, H, W] device tensor, got {face.dtype} {tuple(face.shape)}")
    if face_source.dtype != torch.int32 or face_source.dim() != 1 or face_source.device != face.device:
        raise ValueError("source_masks: face_source must be an int32 [F] tensor on the device of face")
    dev = face.device
    n, h, w = (int(v) for v in face.shape)
    n_cond, n_src = len(groups), int(n_sources)
    with torch.cuda.device(dev):
        masks = torch.empty(n, n_cond, h, w, dtype=torch.float32, device=dev)
        pixels = torch.empty(n, n_src, dtype=torch.int64, device=dev)
        cond_d = torch.from_numpy(cond).to(dev)
        _lib.check(_lib.lib().esr_source_masks(_lib.ptr(face.contiguous()), n, h * w, _lib.ptr(face_source.contiguous()),
                                               int(face_source.shape[0]), _lib.ptr(cond_d), n_src, n_cond, _lib.ptr(masks),
                                               _lib.ptr(pixels), _lib.stream_ptr(dev)), "esr_source_masks")
    return masks, pixels


@torch.no_grad()
def edit_view_data(surface, report, cams: Cameras, view: int, edits: List[dict], z_near: float = Z_NEAR) -> Dict[str, torch.Tensor]:
    """The ``test_data`` of view ``view`` for ``EditRaySelector.apply`` / ``finetune_radiance``, its source masks
    rasterised from the surface: ``surface`` a ``sources.Surface``, ``report`` its ``sources.SourceReport``, ``edits`` a
    list of ``dict(sources=[ids], mode="off" | "i_change" | "c_change" | "ic_change", intensity=1.0, color=(0, 0, 0))``,
    one edit condition each.  Returns ``poses`` [4, 4] float32 (the view's pose back in the loader's Blender convention:
    ``BLENDER2OPENCV`` applied again, which only flips signs), ``em_masks`` [n_cond, H, W], ``em_modes`` int64 [n_cond],
    ``em_intensities`` [n_cond], ``em_colors`` [n_cond, 3], and beside them ``source_pixels`` int64 [S] (the visible
    pixels of every source) and ``n_dropped`` (faces lost at ``z_near``).

    ``relight.label_edit_rays`` projects with K = [[-f, 0, w/2 - 0.5], [0, f, h/2 - 0.5]] (pdra.py:941-943): one focal
    length and the centre in the middle of the image.  A camera set with fx != fy or another centre is refused."""
    if cams.fx != cams.fy or cams.cx != cams.width * 0.5 or cams.cy != cams.height * 0.5:
        raise ValueError(f"edit_view_data: the edit-ray labels project with one focal length and the centre at (W/2, H/2) "
                         f"(pdra.py:941-943); this camera set has fx, fy = {cams.fx}, {cams.fy} and the centre "
                         f"({cams.cx}, {cams.cy}) in a {cams.width} x {cams.height} image")
    view = int(view)
    if not 0 <= view < cams.n_views:
        raise ValueError(f"edit_view_data: view {view} of a set of {cams.n_views}")
    if not edits:
        raise ValueError("edit_view_data: no edit given")
    modes, inten, cols, groups = [], [], [], []
    for e in edits:
        if e.get("mode") not in EDIT_MODES:
            raise ValueError(f"edit_view_data: mode {e.get('mode')!r} is not one of {EDIT_MODES}")
        col = [float(c) for c in e.get("color", (0.0, 0.0, 0.0))]
        if len(col) not in (2, 3):
            raise ValueError(f"edit_view_data: a colour has 2 or 3 components, got {len(col)}")
        modes.append(LIGHT_MODES[e["mode"]])
        inten.append(float(e.get("intensity", 1.0)))
        cols.append((col + [0.0])[:3])
        groups.append(list(e.get("sources", ())))
    _conditions(len(report), groups)                         # (refuses before anything is launched)
    r = rasterize(surface.vertices, surface.triangles, cams, views=view, z_near=z_near)
    masks, pixels = source_masks(r.face, report.face_source, len(report), groups)
    return dict(poses=blender_pose(cams, view), em_masks=masks[0], em_modes=torch.tensor(modes, dtype=torch.int64),
                em_intensities=torch.tensor(inten, dtype=torch.float32), em_colors=torch.tensor(cols, dtype=torch.float32),
                source_pixels=pixels[0], n_dropped=r.n_dropped[0])


__all__ = ["Raster", "rasterize", "source_masks", "edit_view_data", "blender_pose", "world_to_camera", "Z_NEAR", "BIG_PX"]
