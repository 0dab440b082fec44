"""Drop-in for the reference's fine-stage renderer ``app.fine.model.VoxurfF``
(reference: app/fine/model/voxurff.py).

Same constructor, same ``train(mode)`` / ``forward(**kwargs)`` protocol, same
result-dict keys, same sub-module names (the reference's optimizer builds its
param groups by attribute name, app/utils/optimizer.py:14-34) and the same
``state_dict`` keys (checkpoint hand-off between stages, app/fine/fine.py:163).
``forward_training`` is ONE autograd node whose forward/backward enqueue the fused
HIP kernels of libesr_hip.so (esr_nerf_amd/fine_engine.py); nothing on that path
is evaluated by torch ops.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np
import torch
import torch.nn as nn

from . import render_utils
from .fine_engine import KIND_RADIANCE, KIND_TONEMAP, FineEngine, make_scene
from .modules import DenseGrid, ForwardSwitch, GradientConv, MaskCache, RadianceNet, TonemapNet


class _FineRender(torch.autograd.Function):
    """(sdf, off_color, emo_color, 8+8 radiance tensors, 4 tonemap tensors) ->
    (alphainv_last, srgb_marched, lin_marched)."""

    @staticmethod
    def forward(ctx, model, batch, sdf, off_color, emo_color, *mlp_params):
        eng: FineEngine = model.engine
        off_p, emo_p, tone_p = mlp_params[0:8], mlp_params[8:16], mlp_params[16:20]

        def prelude():        # runs on the device while the host waits for the march's plan header
            with eng.packing():
                eng.pack("off", KIND_RADIANCE, list(off_p[0::2]), list(off_p[1::2]))
                eng.pack("emo", KIND_RADIANCE, list(emo_p[0::2]), list(emo_p[1::2]))
                eng.pack("tone", KIND_TONEMAP, list(tone_p[0::2]), list(tone_p[1::2]))

        scene = model.scene_struct()
        fctx, last, srgb, lin = eng.forward(
            scene, batch["rays_o"], batch["rays_d"], batch["viewdirs"], batch["em_modes"],
            model.mask_cache.density.view(*model.mask_cache.density.shape[2:]),
            model.sdf.device_view(), model.off_color.device_view(), model.emo_color.device_view(), prelude=prelude)
        ctx.fctx = fctx
        ctx.model = model
        ctx.shapes = [tuple(p.shape) for p in mlp_params]
        model.last_counts = fctx.counts
        # (fresh tensor objects: the engine's context keeps some of these results for the backward, and a result that left
        #  forward() carries this node as its grad_fn -- node -> ctx -> context -> result -> node would keep the step's buffers alive
        #  until Python's cycle collector runs)
        return last.detach(), srgb.detach(), lin.detach()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_last, g_srgb, g_lin):
        model = ctx.model
        dev = g_last.device
        z = lambda shape: torch.zeros(shape, dtype=torch.float32, device=dev)
        X, Y, Z = model._world_size_l           # host copy: int(device scalar) is a sync each
        g_sdf = z((1, 1, X, Y, Z))
        g_off = z((1, X, Y, Z, 6))
        g_emo = z((1, X, Y, Z, 6))
        mlp_grads = [z(s) for s in ctx.shapes]
        grads = dict(sdf=g_sdf, off_color=g_off, emo_color=g_emo,
                     off_w=mlp_grads[0:8:2], off_b=mlp_grads[1:8:2],
                     emo_w=mlp_grads[8:16:2], emo_b=mlp_grads[9:16:2],
                     tone_w=mlp_grads[16:20:2], tone_b=mlp_grads[17:20:2])
        model.engine.backward(ctx.fctx, g_last, g_srgb, g_lin, grads)
        # colour-grid grads: logical [1,6,X,Y,Z] view over channels-last memory
        return (None, None, g_sdf, g_off.permute(0, 4, 1, 2, 3), g_emo.permute(0, 4, 1, 2, 3), *mlp_grads)


class _SmoothGradTV(torch.autograd.Function):
    """Smoothed-gradient TV term (voxurff.py:609-617) as one differentiable op on the HIP path."""

    @staticmethod
    def forward(ctx, model, sdf_grid, weight):
        if not sdf_grid.is_cuda:
            raise RuntimeError("the TV term runs on the HIP path (no CPU fallback)")
        loss = torch.zeros(1, dtype=torch.float32, device=sdf_grid.device)
        model.smooth_grad_tv_fwd(weight, loss)
        ctx.model, ctx.weight = model, weight
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        m = ctx.model
        grad = torch.zeros_like(m.sdf.grid)
        m.smooth_grad_tv_bwd(ctx.weight, grad, g.reshape(1).float().contiguous())
        return None, grad, None


class VoxurfF(ForwardSwitch, nn.Module):
    def __init__(self, cfg, near: float, far: float, xyz_min: torch.Tensor, xyz_max: torch.Tensor,
                 mask_xyz_min: torch.Tensor, mask_xyz_max: torch.Tensor, mask_alpha_init: float,
                 mask_density: torch.Tensor, s_val: float, num_voxles: int):
        super().__init__()
        self.cfg = cfg
        self.device = cfg.system.device
        m = cfg.app.model
        self.near, self.far = near, far
        self.xyz_min = xyz_min.to(self.device)
        self.xyz_max = xyz_max.to(self.device)
        self.mask_xyz_min = mask_xyz_min.to(self.device)
        self.mask_xyz_max = mask_xyz_max.to(self.device)
        self.mask_alpha_init = mask_alpha_init
        self.mask_density = mask_density.to(self.device)
        self.s_val = s_val
        self.num_voxels = num_voxles

        self.mask_ks = m.mask_ks
        self.maskcache_thres = m.maskcache_thres
        self.fastcolor_thres = m.fastcolor_thres
        self.stepsize = m.stepsize
        self.color_dim = m.color_dim
        self.rgbnet_width, self.rgbnet_depth = m.rgbnet_width, m.rgbnet_depth
        self.tonemap_width, self.tonemap_depth = m.tonemap_width, m.tonemap_depth
        self.posbase_pe, self.viewbase_pe, self.colorbase_pe = m.posbase_pe, m.viewbase_pe, m.colorbase_pe
        self.grad_feat = torch.tensor(list(m.grad_feat), device=self.device)
        self.neus_alpha = m.neus_alpha
        self._check_kernel_config()

        self.set_grid_resolution(self.num_voxels)
        grid_args = dict(world_size=self.world_size, xyz_min=self.xyz_min, xyz_max=self.xyz_max)
        self.sdf = DenseGrid(channels=1, **grid_args)
        ws = [int(v) for v in self.world_size]
        ax = [np.linspace(-1.0, 1.0, n) for n in ws]
        gx, gy, gz = np.meshgrid(*ax, indexing="ij")
        self.sdf.grid.data = torch.from_numpy(np.sqrt(gx ** 2 + gy ** 2 + gz ** 2) - 1).float()[None, None]
        self.sdf_random_init = True
        self.tv_smooth_conv = GradientConv()
        self.mask_cache = MaskCache(self.mask_xyz_min, self.mask_xyz_max, self.mask_density,
                                    self.mask_alpha_init, self.maskcache_thres, self.mask_ks)

        self.off_color = DenseGrid(channels=self.color_dim, **grid_args)
        dim0 = (3 + 3 * self.posbase_pe * 2) + (3 * self.viewbase_pe * 3) + self.color_dim
        dim0 += len(self.grad_feat) * 3 + len(self.grad_feat) * 6 + 1
        self.off_rgbnet = RadianceNet(dim0, self.rgbnet_width, self.rgbnet_depth)
        self.emo_color = DenseGrid(channels=self.color_dim, **grid_args)
        self.emo_rgbnet = RadianceNet(dim0, self.rgbnet_width, self.rgbnet_depth)
        self.tonemapper = TonemapNet(3 + 3 * self.colorbase_pe * 2, self.tonemap_width, self.tonemap_depth)

        self.to(self.device)
        self.set_nonempty_mask()
        self._engine = None
        self.last_counts: Dict[str, int] = {}
        self.gradient = None

    # ------------------------------------------------------------------ config
    def _check_kernel_config(self):
        """The HIP kernels are instantiated for the fine.yaml model; anything else must fail loudly."""
        want = dict(color_dim=6, rgbnet_width=192, rgbnet_depth=4, tonemap_width=192, tonemap_depth=2,
                    posbase_pe=5, viewbase_pe=1, colorbase_pe=5)
        for k, v in want.items():
            if getattr(self, k) != v:
                raise NotImplementedError(f"libesr_hip kernels are built for {k}={v}, got {getattr(self, k)}")
        if len(self.grad_feat) != 4:
            raise NotImplementedError("libesr_hip kernels are built for 4 grad_feat radii")
        if self.neus_alpha not in ("interp", "grad"):
            raise ValueError(f"neus_alpha must be 'interp' or 'grad' (functions.py:45-105), got {self.neus_alpha!r}")
        # (ESRNeRF's grad mode passes the same radius-1 finite-difference gradient to the alpha -- esrnerf.py:587-591,
        # 700-706, sample_sdf_grad / sample_sdf_expgrad_grad_normal -- so its marches use the same kernels)

    @property
    def engine(self) -> FineEngine:
        if self._engine is None:
            if not str(self.device).startswith("cuda"):
                raise RuntimeError("VoxurfF renders through libesr_hip.so and needs a GPU device "
                                   "(there is no CPU fallback)")
            self._engine = FineEngine(self.device, getattr(self, "mlp_dtype", "f32"))
            self._engine.neus_grad = self.neus_alpha == "grad"
        return self._engine

    def scene_struct(self):
        if not hasattr(self, "_mask_box"):
            self._mask_box = (self.mask_xyz_min.tolist(), self.mask_xyz_max.tolist())
        return make_scene(
            self._xyz_cache[0], self._xyz_cache[1], self._mask_box[0], self._mask_box[1],
            self._world_size_l, list(self.mask_cache.density.shape[2:]), self.near,
            self._stepdist, self._voxel_size_f, self.mask_cache.act_shift, self.maskcache_thres,
            self.fastcolor_thres, self.s_val, self._grad_feat_l)

    # ------------------------------------------------------------------ protocol
    def train(self, mode=True):
        self.forward = self.forward_training if mode else self.forward_evaluate
        return super().train(mode)

    def _mlp_params(self) -> List[torch.Tensor]:
        ps = []
        for net in (self.off_rgbnet, self.emo_rgbnet, self.tonemapper):
            for lin in net.layers():
                ps += [lin.weight, lin.bias]
        return ps

    def forward_training(self, **kwargs):
        self.s_val = kwargs["s_val"]
        batch = dict(rays_o=kwargs["rays_o"].contiguous(), rays_d=kwargs["rays_d"].contiguous(),
                     viewdirs=kwargs["viewdirs"].contiguous(), em_modes=kwargs["em_modes"].contiguous())
        last, srgb, lin = _FineRender.apply(self, batch, self.sdf.grid, self.off_color.grid,
                                            self.emo_color.grid, *self._mlp_params())
        return {
            "etc/alphainv_cum": last,
            "etc/white_bg": last[..., None],
            "srgb/rgb": srgb,
            "lin/rgb": lin,
        }

    @torch.no_grad()
    def forward_evaluate(self, **kwargs):
        """Image rendering (voxurff.py:280-461): kwargs rays_o, rays_d, viewdirs [N,3], em_modes (one scalar),
        pos_rt [3,3]; uses ``self.s_val``.  Returns the reference's 12 result keys."""
        eng = self.engine
        for name, kind, net in (("off", KIND_RADIANCE, self.off_rgbnet), ("emo", KIND_RADIANCE, self.emo_rgbnet),
                                ("tone", KIND_TONEMAP, self.tonemapper)):
            lins = net.layers()
            eng.pack(name, kind, [l.weight.detach() for l in lins], [l.bias.detach() for l in lins])
        em = kwargs["em_modes"]
        em = int(em.reshape(-1)[0]) if torch.is_tensor(em) else int(em)
        return eng.evaluate(self.scene_struct(), kwargs["rays_o"].contiguous(), kwargs["rays_d"].contiguous(),
                            kwargs["viewdirs"].contiguous(),
                            self.mask_cache.density.view(*self.mask_cache.density.shape[2:]), self.sdf.device_view(),
                            self.off_color.device_view(), self.emo_color.device_view(), kwargs["pos_rt"], self.far, em)

    # ------------------------------------------------------------------ geometry
    def set_grid_resolution(self, num_voxels: int):
        """voxel_size / world_size as voxurff.py:539-545.  Evaluated on the HOST in fp32 so that the
        grid resolution and the step length are the same bits as the CPU oracle's (a device pow() may
        differ in the last place and would shift every sample)."""
        self.num_voxels = num_voxels
        lo, hi = self.xyz_min.detach().cpu(), self.xyz_max.detach().cpu()
        voxel_size = ((hi - lo).prod() / num_voxels).pow(1 / 3)
        world_size = ((hi - lo) / voxel_size).long()
        self.voxel_size = voxel_size.to(self.xyz_min.device)
        self.world_size = world_size.to(self.xyz_min.device)
        self._voxel_size_f = float(voxel_size)
        self._stepdist = float(self.stepsize * voxel_size)          # fp32 product, as the reference passes it
        self._xyz_cache = (lo.tolist(), hi.tolist())
        self._world_size_l = [int(v) for v in world_size]
        self._grad_feat_l = [float(v) for v in self.grad_feat.tolist()]
        print("voxel_size       {}".format(self.voxel_size))
        print("world_size       {}".format(self.world_size))

    @torch.no_grad()
    def scale_volume_grid(self, num_voxels):
        old = self.world_size
        self.set_grid_resolution(num_voxels)
        print(f"fine: scale_volume_grid scale world_size from {old} to {self.world_size}")
        for g in (self.sdf, self.off_color, self.emo_color):
            g.scale_volume_grid(self.world_size)
        self.set_nonempty_mask()

    @torch.no_grad()
    def set_nonempty_mask(self):
        """Grid nodes inside the mask cache's occupied space; SDF outside is pinned to 1."""
        lin = [torch.linspace(float(self.xyz_min[i]), float(self.xyz_max[i]), self.sdf.grid.shape[2 + i],
                              device=self.xyz_min.device) for i in range(3)]
        if self.sdf.grid.is_cuda:
            # one HIP pass over the nodes: no [X,Y,Z,3] point tensor, the SDF pinned in the same pass
            from .gridsetup import nonempty_mask
            mc = self.mask_cache
            mask, _ = nonempty_mask(mc.density, (mc.xyz_min, mc.xyz_max), mc.act_shift, mc.mask_cache_thres, lin,
                                    sdf=self.sdf.grid.data)
            self.nonempty_mask = mask[None, None]
        else:
            self._set_nonempty_mask_torch(lin)

    @torch.no_grad()
    def _set_nonempty_mask_torch(self, lin):
        """The torch body (CPU-resident models; tools/stage_setup_time.py times it against the kernel)."""
        pts = torch.stack(torch.meshgrid(*lin, indexing="ij"), -1)
        self.nonempty_mask = self.mask_cache(pts)[None, None].contiguous()
        self.sdf.grid[~self.nonempty_mask] = 1

    # ------------------------------------------------------------------ regularisers
    def neus_sdf_gradient(self):
        """Dense central differences of the SDF grid (voxurff.py:723-742).  The reference
        evaluates this on EVERY forward although only the TV term reads it; here it is
        computed on demand by density_total_variation -- identical values, no per-step pass."""
        g = self.sdf.grid
        out = torch.zeros([1, 3, *g.shape[-3:]], device=g.device)
        out[:, 0, 1:-1] = (g[:, 0, 2:] - g[:, 0, :-2]) / 2 / self.voxel_size
        out[:, 1, :, 1:-1] = (g[:, 0, :, 2:] - g[:, 0, :, :-2]) / 2 / self.voxel_size
        out[:, 2, :, :, 1:-1] = (g[:, 0, :, :, 2:] - g[:, 0, :, :, :-2]) / 2 / self.voxel_size
        return out

    def density_total_variation(self, sdf_tv: float = 0, smooth_grad_tv: float = 0):
        tv = 0
        if sdf_tv > 0:
            v, m = self.sdf.grid, self.nonempty_mask
            parts = []
            for d in (2, 3, 4):
                diff = v.diff(dim=d).abs()
                lo = [slice(None)] * 5
                hi = [slice(None)] * 5
                lo[d], hi[d] = slice(None, -1), slice(1, None)
                parts.append(diff[m[tuple(lo)] & m[tuple(hi)]].mean())
            tv = tv + sum(parts) / 3 / 2 / self.voxel_size * sdf_tv
        if smooth_grad_tv > 0:
            # fused HIP kernels (csrc/tv.hip): gradient field, detached 3x3x3 smoothing, masked mean of squares and,
            # in the backward, the adjoint of the central differences -- no dense torch chain, no CPU fallback
            tv = tv + _SmoothGradTV.apply(self, self.sdf.grid, float(smooth_grad_tv))
        return tv

    def _tv_state(self):
        """Host-side constants of the smoothed-gradient TV term: mask bytes + count, conv taps, workspace."""
        st = getattr(self, "_tv_cache", None)
        key = (self.nonempty_mask.data_ptr(), tuple(self.sdf.grid.shape))
        if st is None or st["key"] != key:
            import ctypes as C
            mask = self.nonempty_mask.contiguous().view(torch.uint8)
            w = self.tv_smooth_conv.m.weight.detach().float().cpu().reshape(-1).tolist()
            st = dict(key=key, mask=mask, count=int(self.nonempty_mask.sum()), w27=(C.c_float * 27)(*w),
                      bias=float(self.tv_smooth_conv.m.bias.detach().cpu()),
                      work=torch.empty(6 * self.sdf.grid.numel(), dtype=torch.float32, device=self.sdf.grid.device))
            self._tv_cache = st
        return st

    def smooth_grad_tv_fwd(self, weight: float, loss_out: torch.Tensor):
        """loss_out[0] += weight * smoothed-gradient TV term; leaves the error field for smooth_grad_tv_bwd."""
        import ctypes as C
        from . import _lib
        st, g = self._tv_state(), self.sdf.grid
        X, Y, Z = g.shape[2:]
        _lib.check(_lib.lib().esr_smooth_grad_tv_fwd(
            _lib.ptr(g.detach()), _lib.ptr(st["mask"]), st["w27"], st["bias"], X, Y, Z,
            self._voxel_size_f, st["count"], weight, _lib.ptr(st["work"]),
            _lib.ptr(loss_out), _lib.stream_ptr(g.device)), "esr_smooth_grad_tv_fwd")

    def smooth_grad_tv_bwd(self, weight: float, grad_sdf: torch.Tensor, grad_out: Optional[torch.Tensor] = None):
        """grad_sdf (+)= grad_out * d(term)/d(sdf.grid), from the error field of the last smooth_grad_tv_fwd."""
        import ctypes as C
        from . import _lib
        st = self._tv_state()
        X, Y, Z = self.sdf.grid.shape[2:]
        _lib.check(_lib.lib().esr_smooth_grad_tv_bwd(
            _lib.ptr(st["work"]), X, Y, Z, self._voxel_size_f, st["count"], weight,
            _lib.ptr(grad_out), _lib.ptr(grad_sdf), _lib.stream_ptr(grad_sdf.device)), "esr_smooth_grad_tv_bwd")

    def sdf_total_variation_add_grad(self, weight: float, dense_mode: bool):
        w = weight * max(self._world_size_l) / 128
        self.sdf.total_variation_add_grad(w, w, w, dense_mode)

    # ------------------------------------------------------------------ data filtering
    def sample_ray(self, rays_o: torch.Tensor, rays_d: torch.Tensor):
        """In-box samples of a ray batch, sorted near to far: (ray_pts, ray_id, step_id)."""
        stepdist = self.stepsize * self.voxel_size
        pts, out_box, ray_id, step_id = render_utils.sample_pts_on_rays(
            rays_o.contiguous(), rays_d.contiguous(), self.xyz_min, self.xyz_max, self.near, 1e9, stepdist)[:4]
        keep = ~out_box
        return pts[keep], ray_id[keep], step_id[keep]

    def sample_ray_ori(self, rays_o: torch.Tensor, rays_d: torch.Tensor, is_train: bool = False):
        """Fixed-count sampler of the random-init set-up path (voxurff.py:505-537): every ray gets the same
        ``N = int(|grid_shape + 1| / stepsize) + 1`` steps of ``stepsize * voxel`` starting at its box entry, with the
        t-range clamped to [near, far] (the march sampler uses far = 1e9).  Returns (pts [N,S,3], out-of-box [N,S],
        step lengths).  One-time data filtering, torch ops on the rays' device."""
        n_samples = int(np.linalg.norm(np.array(self.sdf.grid.shape[2:]) + 1) / self.stepsize) + 1
        d_safe = torch.where(rays_d == 0, torch.full_like(rays_d, 1e-6), rays_d)
        ta, tb = (self.xyz_max - rays_o) / d_safe, (self.xyz_min - rays_o) / d_safe
        t_min = torch.minimum(ta, tb).amax(-1).clamp(min=self.near, max=self.far)
        t_max = torch.maximum(ta, tb).amin(-1).clamp(min=self.near, max=self.far)
        miss = t_max <= t_min
        k = torch.arange(n_samples, device=rays_o.device)[None].float()
        if is_train:
            k = k.repeat(rays_d.shape[-2], 1)
            k += torch.rand_like(k[:, [0]])
        step = self.stepsize * self.voxel_size * k
        t = t_min[..., None] + step / rays_d.norm(dim=-1, keepdim=True)
        pts = rays_o[..., None, :] + rays_d[..., None, :] * t[..., None]
        out = miss[..., None] | ((self.xyz_min > pts) | (pts > self.xyz_max)).any(dim=-1)
        return pts, out, step

    def filter_training_rays_in_maskcache_sampling(self, rays_o, rays_d, chunk_size: int):
        """True for rays with at least one in-box sample inside the mask cache (voxurff.py:463-502).  Two branches, as
        in the reference: with ``sdf_random_init`` the fixed-count sampler ``sample_ray_ori`` (t-range clamped to
        near/far), otherwise the march sampler with far = 1e9; they keep different ray sets.  Device tensors go through
        ONE launch of esr_ray_filter over all rays (rayfilter.py; ``chunk_size`` does not touch device work), CPU tensors
        through ``_filter_rays_torch``."""
        from . import rayfilter
        return rayfilter.filter_training_rays(self, rays_o, rays_d, chunk_size, fixed=bool(self.sdf_random_init))

    @torch.no_grad()
    def _filter_rays_torch(self, rays_o, rays_d, chunk_size: int):
        """The reference's chunk loop in torch ops: every sample of a chunk materialised, compacted by boolean mask,
        ``MaskCache.forward`` on the survivors.  What runs for CPU tensors, and what tools/ray_filter_time.py times the
        kernel against."""
        dev = rays_o.device
        keep_all = torch.ones(len(rays_o), dtype=torch.bool, device=dev)
        for idx in torch.arange(len(rays_o), device=dev).split(chunk_size):
            if self.sdf_random_init:
                pts, out, _ = self.sample_ray_ori(rays_o[idx], rays_d[idx])
                inside = ~out
                inside[inside.clone()] = self.mask_cache(pts[inside])
                keep_all[idx] &= inside.any(-1)
            else:
                pts, ray_id, _ = self.sample_ray(rays_o[idx], rays_d[idx])
                hit = torch.zeros(len(idx), dtype=torch.bool, device=dev)
                hit[ray_id[self.mask_cache(pts)]] = True
                keep_all[idx] = hit
        return keep_all

    def extract_geometry(self, resolution: int = 512, threshold: float = 0.0, batch_size: int = 64, smooth: bool = True,
                         sigma: float = 0.5):
        """Mesh export (marching cubes over -sdf); a utility outside the rendering path, see modules.extract_geometry."""
        from .modules import extract_geometry
        return extract_geometry(self, resolution, threshold, batch_size, smooth, sigma)
