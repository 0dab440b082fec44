"""Drop-in for the reference's alphamask renderer ``app.coarse.model.DVGO`` (reference: app/coarse/model/dvgo.py).

Same constructor ``(cfg, near, far, xyz_min, xyz_max)``, attributes (``num_voxels, alpha_init, stepsize, act_shift,
voxel_size, world_size, N_samples, near, far, xyz_min, xyz_max``), parameters (``density [1,1,X,Y,Z]``, ``off_color`` and
``emo_color [1,3,X,Y,Z]``: the optimizer addresses them by name, ``Adam.set_pervoxel_lr`` checks the count's shape, and
checkpoints of either class load into the other) and ``train()`` / ``forward(**kwargs)`` protocol.

On a model whose grids are on the GPU the hot paths run on libesr_hip.so (csrc/dvgo.hip):

``forward_training``   one autograd node (``_DvgoTrain``) over esr_dvgo_fwd / esr_dvgo_bwd; returns alphainv_cum [N,S+1],
                       weights [N,S], white_bg [N,1], raw_rgb [N,S,3] and rgb [N,3]; the backward takes gradients on any
                       subset of them and returns the three grid gradients (the rays get none)
``forward_evaluate``   esr_dvgo_eval, forward only (``em_modes`` one scalar)
``voxel_count_views``  esr_dvgo_count + esr_dvgo_count_add per view

The per-ray jitter is one ``torch.rand`` of shape [N,1] on the rays' device, as the reference draws it;
``render_training(..., jitter)`` takes a recorded draw.  A CPU-resident model runs the torch expressions below (the
reference's arithmetic, as ``mesh.extract_geometry``'s CPU path does), so the coarse stage can build a DVGO anywhere.
``maskout_near_cam_vox``, ``set_grid_resolution``, ``activate_density`` and ``grid_sampler`` are torch plumbing on
either device.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from .modules import ForwardSwitch


class DVGO(ForwardSwitch, nn.Module):
    def __init__(self, cfg, near: float, far: float, xyz_min: torch.Tensor, xyz_max: torch.Tensor):
        super().__init__()
        self.cfg = cfg
        self.device = cfg.system.device
        self.near, self.far = near, far
        self.xyz_min, self.xyz_max = xyz_min, xyz_max
        self.num_voxels = cfg.app.model.num_voxels
        self.alpha_init = cfg.app.model.alpha_init
        self.stepsize = cfg.app.model.stepsize
        self.set_grid_resolution(self.num_voxels)
        # the density bias that makes a zero grid render alpha_init per unit interval
        self.act_shift = np.log(1 / (1 - self.alpha_init) - 1)
        self.density = nn.Parameter(torch.zeros([1, 1, *self.world_size]))
        self.off_color = nn.Parameter(torch.zeros([1, 3, *self.world_size]))
        self.emo_color = nn.Parameter(torch.zeros([1, 3, *self.world_size]))
        self.N_samples = _n_samples(self.density.shape[2:], self.stepsize)
        self._consts_key = None

    def train(self, mode=True):
        self.forward = self.forward_training if mode else self.forward_evaluate
        return super().train(mode)

    # ---- torch plumbing (either device) ----
    def set_grid_resolution(self, num_voxels):
        self.num_voxels = num_voxels
        extent = self.xyz_max - self.xyz_min
        self.voxel_size = (extent.prod() / num_voxels).pow(1 / 3)
        self.world_size = (extent / self.voxel_size).long()

    @torch.no_grad()
    def maskout_near_cam_vox(self, cam_o):
        """density = -100 at every lattice node within ``near`` of a camera centre"""
        dims = self.density.shape[2:]
        axes = [torch.linspace(self.xyz_min[a], self.xyz_max[a], dims[a], device=self.device) for a in range(3)]
        nodes = torch.stack(torch.meshgrid(*axes, indexing="ij"), -1)
        # (cameras in groups of 100 keep the [X,Y,Z,100,3] difference tensor small)
        nearest = torch.stack([(nodes.unsqueeze(-2) - group).pow(2).sum(-1).sqrt().amin(-1)
                               for group in cam_o.split(100)]).amin(0)
        self.density[nearest[None, None] <= self.near] = -100

    def activate_density(self, density, interval=1):
        return 1 - torch.exp(-F.softplus(density + self.act_shift) * interval)

    def grid_sampler(self, xyz, grid):
        """trilinear lookup of grid [1,C,X,Y,Z] at world points xyz [...,3] (align_corners, zero padding) -> [...,C]
        (the channel dimension squeezed when C == 1)"""
        lead = xyz.shape[:-1]
        unit = (xyz.reshape(1, 1, 1, -1, 3) - self.xyz_min) / (self.xyz_max - self.xyz_min)
        coords = unit.flip((-1,)) * 2 - 1
        out = F.grid_sample(grid, coords, mode="bilinear", align_corners=True)
        return out.reshape(grid.shape[1], -1).T.reshape(*lead, grid.shape[1]).squeeze(-1)

    # ---- rendering ----
    def forward_training(self, **kwargs):
        rays_o = kwargs["rays_o"]
        jitter = torch.rand(rays_o.shape[0], 1, device=rays_o.device)
        return self.render_training(rays_o, kwargs["rays_d"], kwargs["em_modes"], jitter)

    def render_training(self, rays_o, rays_d, em_modes, jitter):
        """forward_training with the per-ray jitter given (jitter [N,1], what the reference's torch.rand drew)"""
        if not self.density.is_cuda:
            return _torch_training(self, rays_o, rays_d, em_modes, jitter)
        n = rays_o.shape[0]
        em = (em_modes.reshape(-1) == 1).to(torch.int32).contiguous()
        outs = _DvgoTrain.apply(self, self.density, self.off_color, self.emo_color, rays_o.float().contiguous(),
                                rays_d.float().contiguous(), em, jitter.reshape(n).float().contiguous())
        alphainv_cum, weights, white_bg, raw_rgb, rgb = outs
        return {"etc/alphainv_cum": alphainv_cum, "etc/weights": weights, "etc/white_bg": white_bg,
                "srgb/raw_rgb": raw_rgb, "srgb/rgb": rgb}

    def forward_evaluate(self, **kwargs):
        rays_o, rays_d, em_modes = kwargs["rays_o"], kwargs["rays_d"], kwargs["em_modes"]
        # the reference draws (and multiplies by 0) a jitter here as well: drawing it keeps the generator's stream the same
        torch.rand(rays_o.shape[0], 1, device=rays_o.device)
        if not self.density.is_cuda:
            return _torch_evaluate(self, rays_o, rays_d, em_modes)
        L, dev = _lib.lib(), self.density.device
        n, S = rays_o.shape[0], self.N_samples
        rays_o, rays_d = rays_o.float().contiguous(), rays_d.float().contiguous()
        f = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
        t = dict(alpha=f(n, S), depth=f(n), disp=f(n), white_bg=f(n, 1), off_rgb=f(n, 3), on_rgb=f(n, 3), emo_rgb=f(n, 3))
        nrm = rays_d.norm(dim=-1).contiguous()
        with torch.no_grad(), torch.cuda.device(dev):
            P = self._model_struct()
            R = _rays_struct(rays_o, rays_d, nrm, None, None, 0)
            O = _lib.EsrDvgoOut(**{k: _lib.ptr(v).value or 0 for k, v in t.items()})
            _lib.check(L.esr_dvgo_eval(C.byref(P), C.byref(R), C.byref(O), _lib.stream_ptr(dev)), "esr_dvgo_eval")
        rgb = t["off_rgb"] if int(em_modes) == 0 else t["on_rgb"]
        return {"etc/depth": t["depth"], "etc/disp": t["disp"], "etc/white_bg": t["white_bg"], "srgb/off_rgb": t["off_rgb"],
                "srgb/on_rgb": t["on_rgb"], "srgb/emo_rgb": t["emo_rgb"], "srgb/rgb": rgb}

    def voxel_count_views(self, rays_o: torch.Tensor, rays_d: torch.Tensor, chunk_size: int):
        """rays_o, rays_d [V, H*W, 3] -> float count shaped like density: per voxel, the number of views whose summed
        trilinear weight over every sample of every ray is > 1"""
        if not self.density.is_cuda:
            return _torch_count_views(self, rays_o, rays_d, chunk_size)
        L, dev = _lib.lib(), self.density.device
        count = torch.zeros_like(self.density.detach())
        total = torch.empty(count.numel(), dtype=torch.float32, device=dev)
        with torch.no_grad(), torch.cuda.device(dev):
            P = self._model_struct()
            s = _lib.stream_ptr(dev)
            for ro, rd in zip(rays_o, rays_d):
                ro = ro.to(dev, torch.float32).contiguous()
                rd = rd.to(dev, torch.float32).contiguous()
                nrm = rd.norm(dim=-1).contiguous()
                R = _rays_struct(ro, rd, nrm, None, None, 0)
                total.zero_()
                _lib.check(L.esr_dvgo_count(C.byref(P), C.byref(R), _lib.ptr(total), s), "esr_dvgo_count")
                _lib.check(L.esr_dvgo_count_add(_lib.ptr(total), total.numel(), _lib.ptr(count), s), "esr_dvgo_count_add")
        return count

    def _model_struct(self) -> _lib.EsrDvgo:
        """esr_dvgo_t of the current grids.  The box, near / far and the step scale are read to the host once per
        (box, voxel size) object pair."""
        key = (id(self.xyz_min), id(self.xyz_max), id(self.voxel_size), self.near, self.far, self.stepsize)
        if self._consts_key != key:
            self._consts = (self.xyz_min.float().tolist(), self.xyz_max.float().tolist(),
                            float(torch.as_tensor(self.stepsize * self.voxel_size).float()))
            self._consts_key = key
        lo, hi, step_scale = self._consts
        for g in (self.density, self.off_color, self.emo_color):
            if not g.is_contiguous() or g.dtype != torch.float32:
                raise RuntimeError("DVGO grids must be contiguous float32")
        return _lib.EsrDvgo(self.density.data_ptr(), self.off_color.data_ptr(), self.emo_color.data_ptr(),
                            (C.c_int32 * 3)(*self.density.shape[2:]), (C.c_float * 3)(*lo), (C.c_float * 3)(*hi),
                            float(self.near), float(self.far), step_scale, float(self.stepsize), float(self.act_shift),
                            self.N_samples)


def _n_samples(dims, stepsize) -> int:
    return int(np.linalg.norm(np.array(dims) + 1) / stepsize) + 1


def _rays_struct(rays_o, rays_d, nrm, jitter, em, em_all) -> _lib.EsrDvgoRays:
    p = lambda t: _lib.ptr(t).value or 0
    return _lib.EsrDvgoRays(p(rays_o), p(rays_d), p(nrm), p(jitter), p(em), em_all, rays_o.shape[0])


class _DvgoTrain(torch.autograd.Function):
    """(density, off_color, emo_color) -> (alphainv_cum, weights, white_bg, raw_rgb, rgb) of one ray batch"""

    @staticmethod
    def forward(ctx, model, density, off_color, emo_color, rays_o, rays_d, em, jitter):
        L, dev = _lib.lib(), density.device
        n, S = rays_o.shape[0], model.N_samples
        f = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
        t = dict(alpha=f(n, S), alphainv_cum=f(n, S + 1), weights=f(n, S), raw_rgb=f(n, S, 3), rgb=f(n, 3))
        nrm = rays_d.norm(dim=-1).contiguous()
        with torch.cuda.device(dev):
            P = model._model_struct()
            R = _rays_struct(rays_o, rays_d, nrm, jitter, em, 0)
            O = _lib.EsrDvgoOut(**{k: _lib.ptr(v).value or 0 for k, v in t.items()})
            _lib.check(L.esr_dvgo_fwd(C.byref(P), C.byref(R), C.byref(O), _lib.stream_ptr(dev)), "esr_dvgo_fwd")
        ctx.model = model
        ctx.save_for_backward(rays_o, rays_d, nrm, em, jitter, t["alpha"], t["alphainv_cum"], t["raw_rgb"])
        ctx.set_materialize_grads(False)
        white_bg = t["alphainv_cum"][:, S:].clone()
        return t["alphainv_cum"], t["weights"], white_bg, t["raw_rgb"], t["rgb"]

    @staticmethod
    def backward(ctx, g_cum, g_weights, g_white, g_raw, g_rgb):
        model = ctx.model
        rays_o, rays_d, nrm, em, jitter, alpha, cum, raw = ctx.saved_tensors
        L, dev = _lib.lib(), cum.device
        n, S = alpha.shape
        if g_white is not None:
            g_cum = (torch.zeros_like(cum) if g_cum is None else g_cum.float().clone())
            g_cum[:, S:] += g_white
        prep = lambda g: None if g is None else g.float().contiguous()
        g_cum, g_weights, g_raw, g_rgb = (prep(g) for g in (g_cum, g_weights, g_raw, g_rgb))
        grads = [torch.zeros_like(p) for p in (model.density, model.off_color, model.emo_color)]
        if n > 0 and any(g is not None for g in (g_cum, g_weights, g_raw, g_rgb)):
            with torch.cuda.device(dev):
                P = model._model_struct()
                R = _rays_struct(rays_o, rays_d, nrm, jitter, em, 0)
                p = lambda t: _lib.ptr(t).value or 0
                B = _lib.EsrDvgoBwd(p(alpha), p(cum), p(raw), p(g_cum), p(g_weights), p(g_raw), p(g_rgb), *map(p, grads))
                _lib.check(L.esr_dvgo_bwd(C.byref(P), C.byref(R), C.byref(B), _lib.stream_ptr(dev)), "esr_dvgo_bwd")
        return (None, *grads, None, None, None, None)


# ---------------------------------------------------------------------------
# CPU-resident model: the reference's torch arithmetic
# ---------------------------------------------------------------------------
def _torch_sample(m, rays_o, rays_d, n_samples, jitter=None, masked=True):
    """sample points [N,S,3] (and the out-of-box mask [N,S]) in the reference's float32 expressions"""
    slab_d = torch.where(rays_d == 0, torch.full_like(rays_d, 1e-6), rays_d)
    to_max = (m.xyz_max - rays_o) / slab_d
    to_min = (m.xyz_min - rays_o) / slab_d
    t_min = torch.minimum(to_max, to_min).amax(-1).clamp(min=m.near, max=m.far)
    rng = torch.arange(n_samples, device=rays_o.device)[None].float().repeat(rays_d.shape[-2], 1)
    if jitter is not None:
        rng += jitter
    interpx = t_min[..., None] + m.stepsize * m.voxel_size * rng / rays_d.norm(dim=-1, keepdim=True)
    pts = rays_o[..., None, :] + rays_d[..., None, :] * interpx[..., None]
    if not masked:
        return pts, None
    t_max = torch.maximum(to_max, to_min).amin(-1).clamp(min=m.near, max=m.far)
    outside = (t_max <= t_min)[..., None] | ((m.xyz_min > pts) | (pts > m.xyz_max)).any(-1)
    return pts, outside


def _torch_alpha_weights(m, pts, outside):
    alpha = torch.zeros_like(pts[..., 0])
    alpha[~outside] = m.activate_density(m.grid_sampler(pts[~outside], m.density), m.stepsize)
    p = (1 - alpha).clamp_min(1e-10)
    alphainv_cum = torch.cat([torch.ones_like(p[..., :1]), p.cumprod(-1)], -1)
    return alpha * alphainv_cum[..., :-1], alphainv_cum


def _torch_training(m, rays_o, rays_d, em_modes, jitter):
    pts, outside = _torch_sample(m, rays_o, rays_d, m.N_samples, jitter)
    weights, alphainv_cum = _torch_alpha_weights(m, pts, outside)
    on = em_modes == 1
    rgb = torch.zeros_like(pts)
    rgb[on] = torch.sigmoid(m.grid_sampler(pts[on], m.emo_color))
    rgb = rgb + torch.sigmoid(m.grid_sampler(pts, m.off_color))
    return {"etc/alphainv_cum": alphainv_cum, "etc/weights": weights, "etc/white_bg": alphainv_cum[..., [-1]],
            "srgb/raw_rgb": rgb, "srgb/rgb": (weights[..., None] * rgb).sum(-2)}


def _torch_evaluate(m, rays_o, rays_d, em_modes):
    pts, outside = _torch_sample(m, rays_o, rays_d, m.N_samples)
    weights, alphainv_cum = _torch_alpha_weights(m, pts, outside)
    off = torch.sigmoid(m.grid_sampler(pts, m.off_color))
    emo = torch.sigmoid(m.grid_sampler(pts, m.emo_color))
    w = weights[..., None]
    off_rgb, emo_rgb, on_rgb = (w * off).sum(-2), (w * emo).sum(-2), (w * (off + emo)).sum(-2)
    depth = (weights * (rays_o[..., None, :] - pts).norm(dim=-1)).sum(-1)
    disp = 1 / (depth + alphainv_cum[..., -1] * m.far)
    return {"etc/depth": depth, "etc/disp": disp, "etc/white_bg": alphainv_cum[..., [-1]], "srgb/off_rgb": off_rgb,
            "srgb/on_rgb": on_rgb, "srgb/emo_rgb": emo_rgb, "srgb/rgb": off_rgb if em_modes == 0 else on_rgb}


def _torch_count_views(m, rays_o, rays_d, chunk_size):
    count = torch.zeros_like(m.density.detach())
    for view_o, view_d in zip(rays_o, rays_d):
        ones = torch.ones_like(m.density).requires_grad_()
        for ro, rd in zip(view_o.split(chunk_size), view_d.split(chunk_size)):
            pts, _ = _torch_sample(m, ro, rd, m.N_samples, masked=False)
            m.grid_sampler(pts, ones).sum().backward()
        with torch.no_grad():
            count += ones.grad > 1
    return count
