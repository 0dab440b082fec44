"""Time and peak memory of a stage hand-over on the device: the kernels of esr_nerf_amd/gridsetup.py against the torch bodies
the package keeps for CPU-resident models (``checkpoint._alphamask_bounds_torch``, ``F.max_pool3d``,
the lines of the renderers' ``_set_nonempty_mask_torch``, ``DenseGrid._scale_volume_grid_torch``).

    python tools/stage_setup_time.py [--repeats 5] [--out FILE]

Sizes a user runs:
  alphamask -> coarse   the alphamask grid of cfg/app/alphamask.yaml (1,024,000 voxels: 100^3 in a cube) holding a bumpy blob
                        through the bounding box (``density_bounds``), the mask cache's max pool (ks 3) and the non-empty
                        mask of a coarse SDF grid at coarse.yaml's 884,736 voxels (96^3)
  progressive up-scale  ESRNeRF's four grids (SDF + three 6-channel grids) 160^3 -> 256^3 (fine.yaml pg_scale), then the
                        non-empty mask at 256^3; ``torch.cuda.max_memory_allocated`` above the level before the event, with
                        the old and the new grids alive, on both paths

Each stage: both paths warmed up, then ``--repeats`` rounds that ALTERNATE the kernel and the torch body in one process, each
call between two device events; median and minimum.  The bytes a kernel must move (from the shapes) are printed beside
its time.  The two paths' results are compared (masks: differing nodes; bounds: equal; grids: worst difference) and printed.
One JSON line.
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def alternate(hip, ref, repeats, warmup=2):
    """(hip median, hip min, torch median, torch min) in ms, and the last result of each"""
    for _ in range(warmup):
        hip()
        ref()
    torch.cuda.synchronize()
    th, tr = [], []
    for _ in range(repeats):
        ms, a = _once(hip)
        th.append(ms)
        ms, b = _once(ref)
        tr.append(ms)
    r = lambda v: round(float(v), 4)
    return dict(hip_ms_median=r(np.median(th)), hip_ms_min=r(np.min(th)), torch_ms_median=r(np.median(tr)),
                torch_ms_min=r(np.min(tr)), speedup=round(float(np.median(tr) / np.median(th)), 1)), a, b


def with_bytes(d, n_bytes):
    d["kernel_bytes"] = int(n_bytes)
    d["kernel_gb_per_s"] = round(n_bytes / (d["hip_ms_median"] * 1e-3) / 1e9, 1)
    return d


def blob_density(res, dev):
    """[1,1,res,res,res]: ~12 inside a bumpy blob around the centre, falling through the occupancy threshold (6.9 at
    alpha_init 1e-6, thres 1e-3) at its surface, -10 far outside"""
    ax = torch.linspace(-1, 1, res, device=dev)
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    r = torch.sqrt(x * x + 1.3 * y * y + 0.8 * z * z)
    bumps = 0.12 * torch.sin(5 * x + 1.0) * torch.cos(4 * y) * torch.sin(6 * z + 0.5)
    return (7.0 - 40.0 * (r - 0.62 - bumps)).clamp(-10.0, 12.0)[None, None].contiguous()


def mask_paths(mc, lo, hi, res, dev):
    """the kernel and the torch body of set_nonempty_mask on an SDF grid of res^3 nodes in the box lo .. hi"""
    from esr_nerf_amd.gridsetup import nonempty_mask
    lin = [torch.linspace(float(lo[i]), float(hi[i]), res, device=dev) for i in range(3)]
    sdf_h = torch.randn(1, 1, res, res, res, device=dev)
    sdf_t = sdf_h.clone()
    box = (mc.xyz_min, mc.xyz_max)

    def hip():
        return nonempty_mask(mc.density, box, mc.act_shift, mc.mask_cache_thres, lin, sdf=sdf_h)[0]

    def ref():
        pts = torch.stack(torch.meshgrid(*lin, indexing="ij"), -1)
        mask = mc(pts)[None, None].contiguous()
        sdf_t[~mask] = 1
        return mask[0, 0]
    return hip, ref, sdf_h, sdf_t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("stage_setup_time.py measures on the GPU; none is visible")
    from esr_nerf_amd import checkpoint
    from esr_nerf_amd.gridsetup import density_bounds, maxpool3d, resample_grid
    from esr_nerf_amd.modules import DenseGrid, MaskCache

    dev = torch.device("cuda:0")
    out = dict(device=torch.cuda.get_device_name(0), repeats=a.repeats, stages={})
    alpha_init, thres = 1e-6, 1e-3
    act_shift = math.log(1 / (1 - alpha_init) - 1)
    lo, hi = torch.tensor([-1.0, -1.0, -1.0], device=dev), torch.tensor([1.0, 1.0, 1.0], device=dev)

    # ---- alphamask -> coarse ----
    res = 100
    density = blob_density(res, dev)
    n = res ** 3
    t, b_h, b_t = alternate(lambda: density_bounds(density, (lo, hi), act_shift, thres),
                            lambda: checkpoint._alphamask_bounds_torch(density, lo, hi, act_shift, thres), a.repeats)
    t["equal"] = bool(torch.equal(torch.cat(b_h), torch.cat(b_t)))
    out["stages"]["bounds_100^3"] = with_bytes(t, 4 * n)
    t, p_h, p_t = alternate(lambda: maxpool3d(density, 3),
                            lambda: F.max_pool3d(density, kernel_size=3, padding=1, stride=1).contiguous(), a.repeats)
    t["equal"] = bool(torch.equal(p_h, p_t))
    out["stages"]["maxpool_100^3_ks3"] = with_bytes(t, 8 * n)
    mc = MaskCache(lo, hi, density, alpha_init, thres, 3)
    shift = (b_h[1] - b_h[0]) * (1.05 - 1) / 2                     # coarse.yaml world_bound_scale
    for name, r in (("mask_96^3", 96), ("mask_256^3", 256)):
        hip, ref, sdf_h, sdf_t = mask_paths(mc, b_h[0] - shift, b_h[1] + shift, r, dev)
        t, m_h, m_t = alternate(hip, ref, a.repeats)
        t.update(true_nodes=int(m_h.sum()), nodes_differ=int((m_h != m_t).sum()), sdf_equal=bool(torch.equal(sdf_h, sdf_t)))
        out["stages"][name] = with_bytes(t, 4 * n + r ** 3 + 4 * int((~m_h).sum()))
        del hip, ref, sdf_h, sdf_t, m_h, m_t
    print(json.dumps(out["stages"]), flush=True)

    # ---- progressive up-scale: 160^3 -> 256^3, SDF + three 6-channel grids ----
    r0, r1 = 160, 256
    ws = torch.tensor([r0, r0, r0])
    grids = []
    for ch in (1, 6, 6, 6):
        g = DenseGrid(ch, ws, lo, hi).to(dev)
        with torch.no_grad():
            g.grid.normal_()
        grids.append(g)
    size = (r1, r1, r1)
    hip_up = lambda: [resample_grid(g.device_view(), size) for g in grids]
    torch_up = lambda: [g._scale_volume_grid_torch(size) for g in grids]
    peaks = {}
    for name, fn in (("hip", hip_up), ("torch", torch_up)):
        fn()                                                        # warm-up (allocator, code objects)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        new = fn()
        torch.cuda.synchronize()
        peaks[name] = dict(peak_above_before_mb=round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1),
                           new_grids_mb=round(sum(v.numel() * 4 for v in new) / 2 ** 20, 1))
        del new
    t, u_h, u_t = alternate(hip_up, torch_up, a.repeats, warmup=1)
    worst = 0.0
    for g, h, tt in zip(grids, u_h, u_t):
        tt = tt[0, 0] if g.channels == 1 else tt.permute(0, 2, 3, 4, 1)[0]
        worst = max(worst, float((h - tt).abs().max()))
    t.update(memory=peaks, worst_abs_difference=worst)
    n_cells = 19 * (r0 ** 3 + r1 ** 3)
    out["stages"]["upscale_4_grids_160^3_256^3"] = with_bytes(t, 4 * n_cells)
    print(json.dumps(out["stages"]["upscale_4_grids_160^3_256^3"]), flush=True)

    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
