"""A torch restatement of the DVGO pre-stage's contract (esr_nerf_amd/dvgo.py, csrc/dvgo.hip): the checker of the GPU tests.

Sampling runs in float32 with torch's rounding (the sample points and the out-of-box decisions are part of the contract,
bit for bit); everything after it -- lookups, activation, compositing, colours, the view count's sums -- runs in ``dtype``
(float64 for the parity tests, float32 for the torch baseline of the training test and the timing tool).

``m`` is any object with the model's attributes: xyz_min, xyz_max (float32 [3]), near, far, stepsize, voxel_size,
act_shift, N_samples.  ``grids`` = dict(density [1,1,X,Y,Z], off_color, emo_color [1,3,X,Y,Z]) of ``dtype``.
"""
import torch
import torch.nn.functional as F


def step_scale(m):
    """stepsize * voxel_size as torch rounds it (float32)"""
    return (m.stepsize * torch.as_tensor(m.voxel_size)).float()


def sample(m, rays_o, rays_d, n_samples, jitter=None, with_mask=True):
    """-> (points [N,S,3] float32, out-of-box mask [N,S] or None)"""
    lo, hi = m.xyz_min.to(rays_o), m.xyz_max.to(rays_o)
    d_slab = torch.where(rays_d == 0, torch.full_like(rays_d, 1e-6), rays_d)
    ta, tb = (hi - rays_o) / d_slab, (lo - rays_o) / d_slab
    t_min = torch.minimum(ta, tb).amax(-1).clamp(min=m.near, max=m.far)
    i = torch.arange(n_samples, device=rays_o.device, dtype=torch.float32)[None].expand(rays_o.shape[0], -1)
    if jitter is not None:
        i = i + jitter.reshape(-1, 1)
    t = t_min[:, None] + (step_scale(m).to(rays_o.device) * i) / rays_d.norm(dim=-1, keepdim=True)
    pts = rays_o[:, None, :] + rays_d[:, None, :] * t[..., None]
    if not with_mask:
        return pts, None
    t_max = torch.maximum(ta, tb).amin(-1).clamp(min=m.near, max=m.far)
    out = (t_max <= t_min)[:, None] | (pts < lo).any(-1) | (pts > hi).any(-1)
    return pts, out


def lookup(m, pts, grid):
    """trilinear (align_corners, zero padding) of grid [1,C,X,Y,Z] at world points [...,3], in grid's dtype -> [...,C]"""
    dt = grid.dtype
    lo, hi = m.xyz_min.to(pts.device, dt), m.xyz_max.to(pts.device, dt)
    u = (pts.to(dt) - lo) / (hi - lo)
    g = (u * 2 - 1).flip(-1).reshape(1, 1, 1, -1, 3)
    v = F.grid_sample(grid, g, mode="bilinear", align_corners=True)
    return v.reshape(grid.shape[1], -1).T.reshape(*pts.shape[:-1], grid.shape[1])


def _alpha(m, grids, pts, out):
    d = lookup(m, pts, grids["density"])[..., 0]
    a = 1 - torch.exp(-F.softplus(d + m.act_shift) * m.stepsize)
    return torch.where(out, torch.zeros_like(a), a)


def _composite(alpha):
    p = (1 - alpha).clamp_min(1e-10)
    T = torch.cat([torch.ones_like(p[:, :1]), torch.cumprod(p, -1)], -1)
    return alpha * T[:, :-1], T


def training(m, grids, rays_o, rays_d, em_modes, jitter):
    """the five outputs of forward_training, differentiable in the grids"""
    pts, out = sample(m, rays_o, rays_d, m.N_samples, jitter)
    w, T = _composite(_alpha(m, grids, pts, out))
    on = (em_modes.reshape(-1) == 1).to(w.dtype)[:, None, None]
    raw = torch.sigmoid(lookup(m, pts, grids["off_color"])) + on * torch.sigmoid(lookup(m, pts, grids["emo_color"]))
    return {"etc/alphainv_cum": T, "etc/weights": w, "etc/white_bg": T[:, -1:], "srgb/raw_rgb": raw,
            "srgb/rgb": (w[..., None] * raw).sum(1)}


def evaluate(m, grids, rays_o, rays_d, em_mode):
    pts, out = sample(m, rays_o, rays_d, m.N_samples)
    w, T = _composite(_alpha(m, grids, pts, out))
    off = torch.sigmoid(lookup(m, pts, grids["off_color"]))
    emo = torch.sigmoid(lookup(m, pts, grids["emo_color"]))
    off_rgb, emo_rgb, on_rgb = ((w[..., None] * c).sum(1) for c in (off, emo, off + emo))
    depth = (w * (rays_o[:, None, :].to(w.dtype) - pts.to(w.dtype)).norm(dim=-1)).sum(1)
    return {"etc/depth": depth, "etc/disp": 1 / (depth + T[:, -1] * m.far), "etc/white_bg": T[:, -1:],
            "srgb/off_rgb": off_rgb, "srgb/on_rgb": on_rgb, "srgb/emo_rgb": emo_rgb,
            "srgb/rgb": off_rgb if int(em_mode) == 0 else on_rgb}


def view_sums(m, rays_o, rays_d, dims, dtype=torch.float64):
    """per view, the summed trilinear weight of every unjittered sample of every ray at each voxel -> [V, X, Y, Z]"""
    sums = []
    for ro, rd in zip(rays_o, rays_d):
        pts, _ = sample(m, ro, rd, m.N_samples, with_mask=False)
        ones = torch.ones(1, 1, *dims, dtype=dtype, device=ro.device, requires_grad=True)
        lookup(m, pts, ones).sum().backward()
        sums.append(ones.grad[0, 0])
    return torch.stack(sums)


def count_views(m, rays_o, rays_d, dims):
    """-> (count [1,1,X,Y,Z] float32, the float64 per-view sums [V,X,Y,Z])"""
    s = view_sums(m, rays_o, rays_d, dims)
    return (s > 1).sum(0).float()[None, None], s


def alphamask_loss(res, rgbs, white_bg=1.0, weight_entropy_last=0.01, weight_rgbper=0.1):
    """the alphamask trainer's loss on one batch: clamped white-background MSE, entropy of the last transmittance, and
    the per-sample colour term weighted by the detached weights"""
    rgb = (res["srgb/rgb"] + res["etc/white_bg"] * white_bg).clamp(0.0, 1.0)
    loss = F.mse_loss(rgb, rgbs)
    pout = res["etc/alphainv_cum"][..., -1].clamp(1e-6, 1 - 1e-6)
    loss = loss + weight_entropy_last * -(pout * torch.log(pout) + (1 - pout) * torch.log(1 - pout)).mean()
    per = (res["srgb/raw_rgb"] - rgbs.unsqueeze(-2)).pow(2).sum(-1)
    return loss + weight_rgbper * (per * res["etc/weights"].detach()).sum(-1).mean()
