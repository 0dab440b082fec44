"""Training-ray filter: which rays have an in-box sample inside the mask cache -- the renderers'
``filter_training_rays_in_maskcache_sampling`` (reference: app/coarse/model/voxurfc.py:426-481,
app/fine/model/voxurff.py:463-537) as ONE launch of ``esr_ray_filter`` (esr_nerf_amd/csrc/rayfilter.hip) over all rays.

``filter_rays``            device tensors -> bool flag per ray (and the index of the first kept step on request)
``fixed_n_samples``        the fixed sampler's per-ray sample count, as ``sample_ray_ori`` computes it
``filter_training_rays``   the renderers' method: the kernel for device tensors, their retained torch loop
                           (``_filter_rays_torch``) for CPU tensors, and the reference's printed lines

The reference has two samplers and they keep different ray sets: the fixed one (``sample_ray_ori``: t-range clamped to
[near, far], the same sample count for every ray) is what the coarse renderer always uses and the fine renderer uses while
``sdf_random_init``; the march sampler (far = 1e9) otherwise.  There is no CPU kernel: ``filter_rays`` on CPU tensors raises.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib

MODE_MARCH, MODE_FIXED = _lib.RAY_FILTER_MARCH, _lib.RAY_FILTER_FIXED


def fixed_n_samples(renderer) -> int:
    """voxurfc.py:453-456 / voxurff.py:509-512"""
    return int(np.linalg.norm(np.array(renderer.sdf.grid.shape[2:]) + 1) / renderer.stepsize) + 1


@torch.no_grad()
def filter_rays(renderer, rays_o: torch.Tensor, rays_d: torch.Tensor, fixed: bool, want_first_hit: bool = False):
    """rays_o, rays_d [n, 3] float32 device tensors (any strides) -> ``keep`` [n] bool, or ``(keep, first_hit)`` with
    ``first_hit`` [n] int32: the index of the first kept step, -1 for a dropped ray.  Enqueues one kernel on the current
    stream of the rays' device and returns without waiting for it."""
    if not (rays_o.is_cuda and rays_d.is_cuda):
        raise RuntimeError("filter_rays runs on libesr_hip.so and needs device tensors (there is no CPU kernel)")
    if rays_o.dim() != 2 or rays_o.shape[1] != 3 or rays_o.shape != rays_d.shape:
        raise ValueError(f"filter_rays: rays are [n, 3], got {tuple(rays_o.shape)} and {tuple(rays_d.shape)}")
    if rays_o.dtype != torch.float32 or rays_d.dtype != torch.float32 or rays_o.device != rays_d.device:
        raise ValueError("filter_rays: rays_o and rays_d are float32 tensors on one device")
    density = renderer.mask_cache.density
    if density.device != rays_o.device:
        raise ValueError(f"filter_rays: rays on {rays_o.device}, mask cache on {density.device}")
    dev = rays_o.device
    ro, rd = rays_o.contiguous(), rays_d.contiguous()
    n = int(ro.shape[0])
    scene = renderer.scene_struct()
    with torch.cuda.device(dev):
        keep = torch.empty(n, dtype=torch.uint8, device=dev)
        first = torch.empty(n, dtype=torch.int32, device=dev) if want_first_hit else None
        _lib.check(_lib.lib().esr_ray_filter(
            C.byref(scene), _lib.ptr(density.view(*density.shape[2:])), _lib.ptr(ro), _lib.ptr(rd), n,
            MODE_FIXED if fixed else MODE_MARCH, float(renderer.far), fixed_n_samples(renderer), _lib.ptr(keep),
            _lib.ptr(first), _lib.stream_ptr(dev)), "esr_ray_filter")
    keep = keep.view(torch.bool)
    return (keep, first) if want_first_hit else keep


def filter_training_rays(renderer, rays_o, rays_d, chunk_size: int, fixed: bool):
    """The renderers' ``filter_training_rays_in_maskcache_sampling`` with the reference's printed lines: the kernel for
    device tensors (``chunk_size`` does not touch device work), the torch loop for CPU tensors."""
    import time
    print("get_training_rays_in_maskcache_sampling: start")
    eps_time = time.time()
    if rays_o.is_cuda:
        mask = filter_rays(renderer, rays_o, rays_d, fixed)
    else:
        mask = renderer._filter_rays_torch(rays_o, rays_d, chunk_size)
    ratio = mask.sum() / len(rays_o)            # (the read-back the reference's print does as well)
    eps_time = time.time() - eps_time
    print(f"get_training_rays_in_maskcache_sampling: ratio {ratio}" + "\n"
          + f"get_training_rays_in_maskcache_sampling: finish (eps time: {eps_time} sec)")
    return mask
