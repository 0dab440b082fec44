"""Write tests/golden/dvgo_small.npz: the reference's own DVGO (app/coarse/model/dvgo.py) on a small case, on CPU.

    python tools/gen_dvgo_golden.py            (CPU host with the reference tree)

The reference module is loaded by path with ``omegaconf`` stubbed (absent here); the config is a namespace with the
fields DVGO reads.  The case: a 19 x 16 x 12 grid of random density with a block at -100 (what maskout and
``cnt <= 2`` write) and a dense cluster where 1 - alpha rounds to 0 (the clamp and the underflow of T); 48 rays that
miss the box, start inside it (t_min clamped to near), have exact zero direction components or leave the box midway;
both em_modes.  Recorded: the inputs and the jitter drawn, forward_training's five outputs, the grid gradients under
fixed random upstream gradients on alphainv_cum, weights, raw_rgb and rgb, the grid gradients and value of the alphamask
loss (alphamask.py:247-260), forward_evaluate for em_modes 0 and 1, and voxel_count_views over three 8 x 8 views.  The GPU
tests only read the .npz.
"""
import importlib.util
import os
import sys
import types
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF_ROOT = os.environ.get("ESR_REFERENCE_ROOT", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden", "dvgo_small.npz")

XYZ_MIN, XYZ_MAX = [-1.0, -0.8, -0.6], [1.0, 0.9, 0.7]
NEAR, FAR, NUM_VOXELS, STEPSIZE, ALPHA_INIT = 0.2, 6.0, 4000, 0.5, 1e-4


def cfg():
    return SimpleNamespace(system=SimpleNamespace(device="cpu"),
                           app=SimpleNamespace(model=SimpleNamespace(num_voxels=NUM_VOXELS, stepsize=STEPSIZE,
                                                                     alpha_init=ALPHA_INIT)))


def rays(seed=0):
    """[48,3] origins and directions covering the cases of the module docstring, and em_modes [48]"""
    g = torch.Generator().manual_seed(seed)
    lo, hi = torch.tensor(XYZ_MIN), torch.tensor(XYZ_MAX)
    o, d = [], []
    # through the box from outside (they leave it midway along the march)
    for _ in range(20):
        tgt = lo + (hi - lo) * torch.rand(3, generator=g)
        src = torch.randn(3, generator=g)
        src = src / src.norm() * 2.5
        o.append(src)
        d.append((tgt - src) * (0.5 + torch.rand(1, generator=g)))
    # starting inside the box (t_min clamped to near)
    for _ in range(8):
        o.append(lo + (hi - lo) * (0.2 + 0.6 * torch.rand(3, generator=g)))
        d.append(torch.randn(3, generator=g))
    # exact zero direction components, from outside and inside
    for dd, oo in (([1.0, 0.0, 0.0], [-2.0, 0.1, 0.05]), ([0.0, -1.3, 0.0], [0.2, 2.0, -0.1]),
                   ([0.0, 0.0, 0.7], [-0.3, 0.25, -1.5]), ([0.6, 0.0, -0.8], [-1.5, 0.3, 1.2]),
                   ([0.0, 0.9, 0.4], [0.1, -1.4, -1.0]), ([-0.5, 0.5, 0.0], [0.0, 0.0, 0.0]),
                   ([0.0, 0.0, -1.0], [0.35, -0.2, 0.0]), ([1.0, 0.0, 0.0], [0.3, 0.5, 0.4])):
        o.append(torch.tensor(oo))
        d.append(torch.tensor(dd))
    # through the dense cluster
    for k in range(6):
        o.append(torch.tensor([-2.0, 0.05 * k - 0.1, 0.05 - 0.03 * k]))
        d.append(torch.tensor([1.0, 0.01 * k, -0.02 * k]))
    # missing the box
    for dd, oo in (([1.0, 0.0, 0.0], [3.0, 3.0, 3.0]), ([0.0, 1.0, 0.2], [2.0, -3.0, 0.0]),
                   ([-1.0, -1.0, 0.0], [-2.0, 2.5, 0.0]), ([0.3, 0.2, 1.0], [0.0, 0.0, 2.0]),
                   ([0.2, -1.0, 0.1], [0.0, -1.5, 0.0]),
                   ([1.0, 1.0, 1.0], [1.5, 1.5, 1.5])):
        o.append(torch.tensor(oo))
        d.append(torch.tensor(dd))
    rays_o, rays_d = torch.stack(o).float(), torch.stack(d).float()
    em = (torch.arange(len(rays_o)) % 3 == 1).long()
    return rays_o, rays_d, em


def grids(dims, seed=1):
    """density: smooth random field; a block at -100; a dense cluster (1e4: 1 - alpha == 0) on the cluster rays' path"""
    g = torch.Generator().manual_seed(seed)
    X, Y, Z = dims
    coarse = torch.randn(1, 1, 5, 5, 5, generator=g) * 4 - 2
    density = torch.nn.functional.interpolate(coarse, size=(X, Y, Z), mode="trilinear", align_corners=True)
    density = density + 0.5 * torch.randn(1, 1, X, Y, Z, generator=g)
    density[..., 2:6, 9:14, 3:8] = -100
    density[..., 8:13, 6:10, 4:8] = 1e4
    off = torch.randn(1, 3, X, Y, Z, generator=g)
    emo = torch.randn(1, 3, X, Y, Z, generator=g)
    return density.contiguous(), off, emo


def views(n_views=3, hw=8, seed=2):
    """[V, hw*hw, 3] pinhole rays of cameras on a circle around the box, looking at its centre"""
    g = torch.Generator().manual_seed(seed)
    centre = (torch.tensor(XYZ_MIN) + torch.tensor(XYZ_MAX)) / 2
    os_, ds = [], []
    for v in range(n_views):
        a = 2 * np.pi * v / n_views + 0.3
        cam = centre + torch.tensor([2.2 * np.cos(a), 2.2 * np.sin(a), 0.6 + 0.1 * v], dtype=torch.float32)
        fwd = centre - cam
        fwd = fwd / fwd.norm()
        right = torch.linalg.cross(fwd, torch.tensor([0.0, 0.0, 1.0]))
        right = right / right.norm()
        up = torch.linalg.cross(right, fwd)
        s = torch.linspace(-0.45, 0.45, hw)
        jj, ii = torch.meshgrid(s, s, indexing="ij")
        d = fwd + ii[..., None] * right + jj[..., None] * up + 0.01 * torch.randn(hw, hw, 3, generator=g)
        os_.append(cam.expand(hw * hw, 3))
        ds.append(d.reshape(-1, 3))
    return torch.stack(os_).float().contiguous(), torch.stack(ds).float().contiguous()


def load_dvgo():
    om = types.ModuleType("omegaconf")
    om.DictConfig = type("DictConfig", (dict,), {})
    sys.modules.setdefault("omegaconf", om)
    spec = importlib.util.spec_from_file_location("ref_dvgo", os.path.join(REF_ROOT, "app", "coarse", "model", "dvgo.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.DVGO


def main():
    DVGO = load_dvgo()
    m = DVGO(cfg(), NEAR, FAR, torch.tensor(XYZ_MIN), torch.tensor(XYZ_MAX))
    dims = tuple(m.density.shape[2:])
    density, off, emo = grids(dims)
    with torch.no_grad():
        m.density.copy_(density)
        m.off_color.copy_(off)
        m.emo_color.copy_(emo)
    rays_o, rays_d, em = rays()
    n = len(rays_o)
    out = dict(xyz_min=np.float32(XYZ_MIN), xyz_max=np.float32(XYZ_MAX), near=np.float64(NEAR), far=np.float64(FAR),
               num_voxels=np.int64(NUM_VOXELS), stepsize=np.float64(STEPSIZE), alpha_init=np.float64(ALPHA_INIT),
               voxel_size=m.voxel_size.numpy(), world_size=m.world_size.numpy(), N_samples=np.int64(m.N_samples),
               act_shift=np.float64(m.act_shift), density=density.numpy(), off_color=off.numpy(), emo_color=emo.numpy(),
               rays_o=rays_o.numpy(), rays_d=rays_d.numpy(), em_modes=em.numpy())
    keys = ("etc/alphainv_cum", "etc/weights", "etc/white_bg", "srgb/raw_rgb", "srgb/rgb")
    names = ("density", "off_color", "emo_color")

    # forward_training, with the jitter it draws recorded
    m.train()
    torch.manual_seed(7)
    out["jitter"] = torch.rand(n, 1).numpy()
    torch.manual_seed(7)
    res = m(rays_o=rays_o, rays_d=rays_d, em_modes=em)
    for k in keys:
        out["train/" + k] = res[k].detach().numpy()

    # grid gradients under fixed upstream gradients on the four differentiable outputs
    g = torch.Generator().manual_seed(3)
    four = ("etc/alphainv_cum", "etc/weights", "srgb/raw_rgb", "srgb/rgb")
    up = {k: torch.randn(res[k].shape, generator=g) for k in four}
    gr = torch.autograd.grad(sum((res[k] * up[k]).sum() for k in four), [getattr(m, k) for k in names],
                             retain_graph=True)
    for k in four:
        out["up/" + k] = up[k].numpy()
    for k, v in zip(names, gr):
        out["grad/" + k] = v.numpy()

    # the alphamask loss (alphamask.py:247-260, white background)
    rgbs = torch.rand(n, 3, generator=g)
    out["rgbs"] = rgbs.numpy()
    rgb = (res["srgb/rgb"] + res["etc/white_bg"] * 1.0).clamp(min=0.0, max=1.0)
    loss = torch.nn.functional.mse_loss(rgb, rgbs)
    pout = res["etc/alphainv_cum"][..., -1].clamp(1e-6, 1 - 1e-6)
    loss = loss + 0.01 * -(pout * torch.log(pout) + (1 - pout) * torch.log(1 - pout)).mean()
    rgbper = (res["srgb/raw_rgb"] - rgbs.unsqueeze(-2)).pow(2).sum(-1)
    loss = loss + 0.1 * (rgbper * res["etc/weights"].detach()).sum(-1).mean()
    gl = torch.autograd.grad(loss, [getattr(m, k) for k in names])
    out["loss"] = np.float64(loss.item())
    for k, v in zip(names, gl):
        out["loss_grad/" + k] = v.numpy()

    # forward_evaluate for both em_modes
    m.eval()
    for mode in (0, 1):
        with torch.no_grad():
            ev = m(rays_o=rays_o, rays_d=rays_d, em_modes=mode)
        for k, v in ev.items():
            out[f"eval{mode}/{k}"] = v.numpy()

    # voxel_count_views over three views
    vo, vd = views()
    out["views_o"], out["views_d"] = vo.numpy(), vd.numpy()
    out["count"] = m.voxel_count_views(vo, vd, 50).numpy()

    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} B): world_size {dims}, N_samples {m.N_samples}, "
          f"count total {out['count'].sum()}")


if __name__ == "__main__":
    main()
