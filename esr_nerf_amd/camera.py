"""Camera-defined ray sets: a stage's rays described by its cameras and images, made in the kernels from (view, pixel)
(esr_nerf_amd/csrc/camera.hip, csrc/camera_ray.h) instead of stored as per-ray arrays.

``Cameras``               [V, 3, 4] camera-to-world poses on the device + shared intrinsics (``from_blender``: the ESR-NeRF
                          loader, data/esrnerf/esrnerf.py:39-59,253; ``from_intrinsics``: the DTU loader, data/dtu/dtu.py:74-86)
``camera_rays``           dense ``(rays_o, rays_d, viewdirs)`` of all or some views (``pose2ray`` + ``F.normalize``)
``camera_batch``          the trainers' batch dictionary of given ray rows in ONE launch (rays, composited colours, em_modes)
``frustum_bbox``          the alphamask stage's bounding box of the near / far frustum points (app/coarse/alphamask.py:108-122)
``filter_camera_rays``    ``rayfilter.filter_rays`` over every ray of the set, without ray arrays
``CameraBatchSampler`` / ``CameraRayGroupManager``   the samplers of data.py on a camera set: the same constructor arguments,
                          attributes, shuffle / filter / sample order, sharding and checkpointed ``data_idxs``.  They replace
                          the three hooks data.py gives its samplers -- ``_preload`` (always the device), ``_adopt`` (take
                          cameras + images in) and ``_gather`` (the row gather of ``sample``: one kernel launch) -- and
                          the by-key accessors built on the arrays (``current``, ``uncert``, ``cert``)

A ray's row is ``view * H * W + pixel`` with ``pixel = j * W + i``: the row order of the loaders' flattened training arrays, so
index vectors are interchangeable between the two forms.  A stage's set costs 48 B per view plus the image store (4 B per
pixel as RGBA8) instead of 56 B per ray.  There is no CPU kernel: every function here raises on CPU tensors.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Optional

import numpy as np
import torch

from . import _lib
from .data import BatchSampler, RayGroupManager, _preload_to_cpu
from .rayfilter import MODE_FIXED, MODE_MARCH, fixed_n_samples

MAX_ROWS = 1 << 31                         # rows are 32-bit inside the kernels
RAY_KEYS = ("rays_o", "rays_d", "viewdirs", "rgbs", "em_modes")
BLENDER2OPENCV = ((1, 0, 0, 0), (0, -1, 0, 0), (0, 0, -1, 0), (0, 0, 0, 1))       # esrnerf.py:44-46


def uint8_table() -> np.ndarray:
    """float32 value of every uint8 channel value as the loaders compute it: ``torch.FloatTensor(np.asarray(image) / 255.0)``
    (esrnerf.py:159-161, dtu.py:169-171) -- the division in float64, one rounding to float32"""
    return (np.arange(256) / 255.0).astype(np.float32)


class Cameras:
    """V pinhole cameras sharing ``fx, fy, cx, cy`` (binary32 values) and the image size; ``poses`` [V, 3, 4] float32
    camera-to-world matrices in the kernels' one convention (x right, y down, z forward), on the device they are given on."""

    def __init__(self, poses: torch.Tensor, fx, fy, cx, cy, width: int, height: int):
        if not torch.is_tensor(poses) or poses.dim() != 3 or tuple(poses.shape[1:]) != (3, 4):
            raise ValueError(f"Cameras: poses are [V, 3, 4], got {tuple(getattr(poses, 'shape', ()))}")
        if poses.dtype != torch.float32:
            raise ValueError(f"Cameras: poses are float32, got {poses.dtype}")
        width, height = int(width), int(height)
        if width < 1 or height < 1:
            raise ValueError(f"Cameras: image size {width} x {height}")
        if int(poses.shape[0]) * width * height >= MAX_ROWS:
            raise ValueError(f"Cameras: {poses.shape[0]} views of {width} x {height} are {int(poses.shape[0]) * width * height} "
                             f"rays; a camera set holds fewer than 2^31 (split the views over several sets)")
        if not bool(torch.isfinite(poses).all()):          # (frustum_bbox folds with min / max, which would drop a NaN)
            raise ValueError("Cameras: poses are finite")
        self.poses = poses.contiguous()
        self.fx, self.fy, self.cx, self.cy = (float(np.float32(v)) for v in (fx, fy, cx, cy))
        if not (self.fx != 0.0 and self.fy != 0.0 and all(math.isfinite(v) for v in (self.fx, self.fy, self.cx, self.cy))):
            raise ValueError("Cameras: focal lengths are finite and non-zero, the centre is finite")
        self.width, self.height = width, height

    @classmethod
    def from_blender(cls, transform_matrices, camera_angle_x: float, width: int, height: int, device=None) -> "Cameras":
        """The ESR-NeRF loader's cameras (esrnerf.py:39-59,253): ``transform_matrices`` [V, 4, 4] (or [V, 3, 4]) as in
        ``transforms_*.json``.  focal = width / 2 / tan(angle / 2) in float64, rounded to float32 where the loader's
        tensor-by-scalar division rounds it; centre = (width * 0.5, height * 0.5); pose = float32(matrix) @ blender2opencv."""
        m = torch.as_tensor(np.asarray(transform_matrices, dtype=np.float64)).to(torch.float32)      # torch.FloatTensor(pose)
        if m.dim() != 3 or m.shape[1] not in (3, 4) or m.shape[2] != 4:
            raise ValueError(f"from_blender: transform matrices are [V, 4, 4], got {tuple(m.shape)}")
        flip = torch.tensor(BLENDER2OPENCV, dtype=torch.float32)
        poses = (m @ flip)[:, :3, :4]
        flen = width / 2.0 / math.tan(float(camera_angle_x) / 2.0)
        return cls(poses.to(device) if device is not None else poses, flen, flen, width * 0.5, height * 0.5, width, height)

    @classmethod
    def from_intrinsics(cls, poses, K, width: int, height: int, device=None) -> "Cameras":
        """The DTU loader's cameras (dtu.py:74-86): ``poses`` [V, 4, 4] or [V, 3, 4] camera-to-world (already in the kernels'
        convention), ``K`` the 3x3 (or 4x4) intrinsics in float64; fx = K[0][0], fy = K[1][1], cx = K[0][2], cy = K[1][2], each
        rounded to float32 where the loader's tensor-by-scalar arithmetic rounds it."""
        p = torch.as_tensor(np.asarray(poses.cpu() if torch.is_tensor(poses) else poses)).to(torch.float32)
        if p.dim() != 3 or p.shape[1] not in (3, 4) or p.shape[2] != 4:
            raise ValueError(f"from_intrinsics: poses are [V, 4, 4] or [V, 3, 4], got {tuple(p.shape)}")
        K = np.asarray(K, dtype=np.float64)
        p = p[:, :3, :4]
        return cls(p.to(device) if device is not None else p, K[0][0], K[1][1], K[0][2], K[1][2], width, height)

    @property
    def n_views(self) -> int:
        return int(self.poses.shape[0])

    @property
    def n_rays(self) -> int:
        return self.n_views * self.width * self.height

    @property
    def device(self) -> torch.device:
        return self.poses.device

    def to(self, device) -> "Cameras":
        return Cameras(self.poses.to(device), self.fx, self.fy, self.cx, self.cy, self.width, self.height)

    def struct(self) -> _lib.EsrCamera:
        return _lib.EsrCamera(self.fx, self.fy, self.cx, self.cy, self.width, self.height, self.n_views)


def _need_device(what: str, *tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError(f"{what} runs on libesr_hip.so and needs device tensors (there is no CPU kernel)")


def validate_rows(cams: Cameras, rows: torch.Tensor):
    """Raise unless ``rows`` is an int64 vector of rows of ``cams`` (one read-back for a device tensor)."""
    if not torch.is_tensor(rows) or rows.dtype != torch.int64 or rows.dim() != 1:
        raise ValueError(f"camera rows are an int64 vector, got {getattr(rows, 'dtype', type(rows))} "
                         f"{tuple(getattr(rows, 'shape', ()))}")
    if rows.numel():
        lo, hi = (int(v) for v in torch.stack([rows.min(), rows.max()]).tolist())
        if lo < 0 or hi >= cams.n_rays:
            raise ValueError(f"camera rows out of range: [{lo}, {hi}] for a set of {cams.n_rays} rays")


def check_images(cams: Cameras, images: torch.Tensor, em_modes: torch.Tensor) -> int:
    """The image store and the per-view mode table of a camera set; returns the kernel's ``channels`` argument."""
    n = cams.n_rays
    if images.dim() != 2 or images.shape[0] != n:
        raise ValueError(f"camera images are [V * H * W, C] = [{n}, C], got {tuple(images.shape)}")
    if images.dtype == torch.uint8 and images.shape[1] in (3, 4):
        ch = int(images.shape[1])
    elif images.dtype == torch.float32 and images.shape[1] == 3:
        ch = 0
    else:
        raise ValueError(f"camera images are uint8 [n, 3 or 4] or composited float32 [n, 3], got {images.dtype} "
                         f"{tuple(images.shape)}")
    if em_modes.dtype != torch.int64 or tuple(em_modes.shape) != (cams.n_views,):
        raise ValueError(f"camera em_modes are one int64 per view [{cams.n_views}], got {em_modes.dtype} {tuple(em_modes.shape)}")
    return ch


_tables: Dict[torch.device, torch.Tensor] = {}


def _table(dev: torch.device) -> torch.Tensor:
    if dev not in _tables:
        _tables[dev] = torch.from_numpy(uint8_table()).to(dev)
    return _tables[dev]


@torch.no_grad()
def camera_rays(cams: Cameras, views=None):
    """``(rays_o, rays_d, viewdirs)`` [n * H * W, 3] float32 of the views ``views``: None = all, an int = that view, a
    ``range`` / ``(v0, v1)`` = the views v0 .. v1 - 1.  One launch, not waited for."""
    _need_device("camera_rays", cams.poses)
    if views is None:
        v0, v1 = 0, cams.n_views
    elif isinstance(views, int):
        v0, v1 = views, views + 1
    elif isinstance(views, range) and views.step == 1:
        v0, v1 = views.start, views.stop
    else:
        v0, v1 = (int(v) for v in views)
    if not 0 <= v0 <= v1 <= cams.n_views:
        raise ValueError(f"camera_rays: views [{v0}, {v1}) of a set of {cams.n_views}")
    dev = cams.device
    n = (v1 - v0) * cams.width * cams.height
    cam = cams.struct()
    with torch.cuda.device(dev):
        ro, rd, vd = (torch.empty(n, 3, dtype=torch.float32, device=dev) for _ in range(3))
        _lib.check(_lib.lib().esr_camera_rays(C.byref(cam), _lib.ptr(cams.poses), v0, v1, _lib.ptr(ro), _lib.ptr(rd),
                                              _lib.ptr(vd), _lib.stream_ptr(dev)), "esr_camera_rays")
    return ro, rd, vd


@torch.no_grad()
def camera_batch(cams: Cameras, images: torch.Tensor, em_modes: torch.Tensor, rows: torch.Tensor, white_bg,
                 check_rows: bool = True) -> Dict[str, torch.Tensor]:
    """The batch dictionary (``rays_o``, ``rays_d``, ``viewdirs``, ``rgbs`` [n, 3] float32, ``em_modes`` [n] int64) of the ray
    rows ``rows`` (int64, any order, repeats allowed) in one launch.  ``images``: uint8 [V*H*W, 3 or 4] (RGBA is composited
    over ``white_bg`` as the loader does, esrnerf.py:235-236) or float32 [V*H*W, 3] already composited; ``em_modes`` int64
    [V].  ``check_rows=False`` skips the range check's read-back (the samplers' index vectors are in range by construction;
    the kernel reads nothing for a row out of range and returns NaN for it)."""
    if not torch.is_tensor(rows) or rows.dtype != torch.int64 or rows.dim() != 1:
        raise ValueError(f"camera_batch: rows are an int64 vector, got {getattr(rows, 'dtype', type(rows))} "
                         f"{tuple(getattr(rows, 'shape', ()))}")
    _need_device("camera_batch", cams.poses, images, em_modes, rows)
    ch = check_images(cams, images, em_modes)
    dev = cams.device
    if not (images.device == em_modes.device == rows.device == dev):
        raise ValueError("camera_batch: cameras, images, em_modes and rows are on one device")
    if check_rows:
        validate_rows(cams, rows)
    n = int(rows.numel())
    cam = cams.struct()
    with torch.cuda.device(dev):
        ro, rd, vd, rgb = (torch.empty(n, 3, dtype=torch.float32, device=dev) for _ in range(4))
        em = torch.empty(n, dtype=torch.int64, device=dev)
        _lib.check(_lib.lib().esr_camera_batch(
            C.byref(cam), _lib.ptr(cams.poses), _lib.ptr(em_modes.contiguous()), _lib.ptr(images.contiguous()), ch,
            _lib.ptr(_table(dev)) if ch else None, float(white_bg), _lib.ptr(rows.contiguous()), n, _lib.ptr(ro), _lib.ptr(rd),
            _lib.ptr(vd), _lib.ptr(rgb), _lib.ptr(em), _lib.stream_ptr(dev)), "esr_camera_batch")
    return dict(rays_o=ro, rays_d=rd, viewdirs=vd, rgbs=rgb, em_modes=em)


@torch.no_grad()
def frustum_bbox(cams: Cameras, near: float, far: float):
    """``(xyz_min, xyz_max)`` [3] float32 over ``o + viewdir * near`` and ``o + viewdir * far`` of every ray of every view:
    the alphamask stage's ``compute_bbox_by_cam_frustrm`` (alphamask.py:108-122) without the rays."""
    _need_device("frustum_bbox", cams.poses)
    dev = cams.device
    cam = cams.struct()
    with torch.cuda.device(dev):
        part = torch.empty(_lib.CAMERA_BOUNDS_BLOCKS * 6, dtype=torch.float32, device=dev)
        out = torch.empty(6, dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().esr_camera_bounds(C.byref(cam), _lib.ptr(cams.poses), float(near), float(far), _lib.ptr(part),
                                                _lib.ptr(out), _lib.stream_ptr(dev)), "esr_camera_bounds")
    return out[:3], out[3:]


@torch.no_grad()
def filter_camera_rays(renderer, cams: Cameras, fixed: bool, want_first_hit: bool = False):
    """``rayfilter.filter_rays`` over every ray of the set in row order, the rays made in the kernel: ``keep`` [V*H*W] bool,
    or ``(keep, first_hit)`` with ``first_hit`` int32.  Bit-equal to ``filter_rays(renderer, *camera_rays(cams)[:2], fixed)``."""
    _need_device("filter_camera_rays", cams.poses)
    density = renderer.mask_cache.density
    dev = cams.device
    if density.device != dev:
        raise ValueError(f"filter_camera_rays: cameras on {dev}, mask cache on {density.device}")
    n = cams.n_rays
    scene = renderer.scene_struct()
    cam = cams.struct()
    with torch.cuda.device(dev):
        keep = torch.empty(n, dtype=torch.uint8, device=dev)
        first = torch.empty(n, dtype=torch.int32, device=dev) if want_first_hit else None
        _lib.check(_lib.lib().esr_ray_filter_cameras(
            C.byref(scene), _lib.ptr(density.view(*density.shape[2:])), C.byref(cam), _lib.ptr(cams.poses),
            MODE_FIXED if fixed else MODE_MARCH, float(renderer.far), fixed_n_samples(renderer), _lib.ptr(keep),
            _lib.ptr(first), _lib.stream_ptr(dev)), "esr_ray_filter_cameras")
    keep = keep.view(torch.bool)
    return (keep, first) if want_first_hit else keep


class _CameraRows:
    """What the camera samplers change in the samplers of data.py: where the ray set lives and how rows are gathered."""

    @staticmethod
    def _preload(cfg) -> bool:
        _preload_to_cpu(cfg)          # (the setting is still validated)
        return False                  # data_preload: cpu is accepted and ignored: the set is cameras + RGBA8, 14 x smaller
                                      # than the ray arrays the setting exists for, and rays are made by a device kernel

    def _adopt(self, data) -> int:
        cams, images, em_modes = data
        self.cams = cams.to(self.device)
        self.images = images.to(self.device).contiguous()
        self.em_modes = em_modes.to(self.device).contiguous()
        check_images(self.cams, self.images, self.em_modes)
        self.white_bg = self.cfg.data.white_bg
        self.data: Dict[str, torch.Tensor] = {}          # per-row arrays put beside the cameras later (set_rows)
        return self.cams.n_rays

    def _gather(self, rows: torch.Tensor) -> Dict[str, torch.Tensor]:
        made = camera_batch(self.cams, self.images, self.em_modes, rows, self.white_bg, check_rows=False)
        # an array a caller has attached under a key (RayGroupManager.set_rows) replaces the camera set's value for it
        missing = [k for k in self.keys if k not in self.data and k not in made]
        if missing:
            raise KeyError(f"a camera ray set provides {RAY_KEYS}; attach {missing} with set_rows before sampling")
        return {k: (self.data[k][rows] if k in self.data else made[k]) for k in self.keys}


class CameraBatchSampler(_CameraRows, BatchSampler):
    """``BatchSampler`` on a camera set: ``CameraBatchSampler(cfg, cams, images, em_modes, keys, batch_size, ...)``."""

    def __init__(self, cfg, cams: Cameras, images: torch.Tensor, em_modes: torch.Tensor, keys: List[str], batch_size: int,
                 batch_st: int = 0, data_idxs: Optional[torch.Tensor] = None, rank: int = 0, world: int = 1):
        _check_keys(keys)
        super().__init__(cfg, (cams, images, em_modes), keys, batch_size, batch_st, data_idxs, rank, world)
        validate_rows(self.cams, self.data_idxs)

    def current(self, key: str) -> torch.Tensor:
        return self._gather(self.data_idxs)[key]


class CameraRayGroupManager(_CameraRows, RayGroupManager):
    """``RayGroupManager`` on a camera set: ``CameraRayGroupManager(cfg, cams, images, em_modes, keys, uncert_batch_size,
    cert_batch_size, ...)``."""

    def __init__(self, cfg, cams: Cameras, images: torch.Tensor, em_modes: torch.Tensor, keys: List[str],
                 uncert_batch_size: int, cert_batch_size: int, uncert_batch_st: int = 0, cert_batch_st: int = 0,
                 uncert_data_idxs: Optional[torch.Tensor] = None, cert_data_idxs: Optional[torch.Tensor] = None,
                 rank: int = 0, world: int = 1):
        _check_keys(keys, extra_ok=True)
        super().__init__(cfg, (cams, images, em_modes), keys, uncert_batch_size, cert_batch_size, uncert_batch_st,
                         cert_batch_st, uncert_data_idxs, cert_data_idxs, rank, world)
        validate_rows(self.cams, self.uncert_data_idxs)
        validate_rows(self.cams, self.cert_data_idxs)

    def uncert(self, key: str) -> torch.Tensor:
        return self._gather(self.uncert_data_idxs)[key]

    def cert(self, key: str) -> torch.Tensor:
        return self._gather(self.cert_data_idxs)[key]


def _check_keys(keys, extra_ok: bool = False):
    bad = [k for k in keys if k not in RAY_KEYS]
    if bad and not extra_ok:
        raise ValueError(f"a camera ray set provides {RAY_KEYS}; no {bad}")
