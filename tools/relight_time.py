"""Stage times of selecting and labelling one re-lighting view's edit rays on the device (esr_nerf_amd/relight.py).

    python tools/relight_time.py [--rays 20000000] [--size 800] [--march-rays 1048576] [--repeats 10] [--out FILE]

Event-timed after a warm-up, on a realistic case (an 800 x 800 view, three conditions, tens of millions of training rays):
the dilation, the label launch (with its compulsory bytes: 12 B read and 21 B written per ray, and the rate they give),
the sampler bookkeeping (``attach_edit_labels``: three full-length arrays, the group filter), and the once-per-checkpoint
``eval_esp`` cache on ``--march-rays`` rays of the C2 slab scene (per-ray time; the reference pays it per VIEW).  Beside
them a torch-on-device restatement of the reference's per-view lines (app/fine/pdra.py:945-1044) on the same card and the
same case, WITHOUT its march (``eval_esp`` per chunk is the same kernel either way): the dilation as a padded max-pool, then
per ``eval.batch_size`` chunk the two matmuls, the bound test, ``grid_sample`` and the chain of masked assignments.  Its
labels are compared with the kernel's.  For the streaming yardstick run tools/hbm_read_rate.py on the same card.
One JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, repeats, warmup=2):
    """median / min milliseconds of fn() by device events"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return round(float(np.median(ms)), 4), round(float(np.min(ms)), 4)


def torch_dilate(masks, ks):
    a, b = ks // 2, ks - 1 - ks // 2
    return F.max_pool2d(F.pad(masks[:, None], (a, b, a, b), value=float("-inf")), ks, stride=1)[:, 0]


def torch_reference_view(esp, pose, f, w, h, em_masks, ks, modes_c, inten_c, col_c, bs):
    """pdra.py:945-1028 on device tensors, chunk by chunk (the march left out)"""
    dev = esp.device
    w2c = torch.inverse(pose).to(dev)
    K = torch.tensor([[-f, 0.0, w / 2.0 - 0.5], [0.0, f, h / 2.0 - 0.5], [0.0, 0.0, 1.0]]).to(dev, dtype=torch.float32)
    masks = torch_dilate(em_masks, ks).view(-1, 1, h, w)
    n = len(esp)
    keep = torch.zeros(n, dtype=torch.bool, device=dev)
    modes = torch.ones(n, dtype=torch.long, device=dev)
    colors = torch.zeros(n, 2, device=dev)
    intens = torch.zeros(n, device=dev)
    for idx in torch.arange(n, device=dev).split(bs):
        p = esp[idx]
        p = torch.concat([p, torch.ones_like(p[..., :1])], dim=-1).T
        xyz = w2c @ p
        cam = xyz[:3] / xyz[-1:]
        xyz = K @ cam
        ic = (xyz[:2] / xyz[-1:]).T
        ob = (ic < 0) | (ic > (h - 1)) | (ic > (w - 1))
        inb = (ob[..., 0] | ob[..., 1]).bitwise_not()
        ic = ic[inb]
        ic[..., 0] = ic[..., 0] / (w - 1) * 2 - 1
        ic[..., 1] = ic[..., 1] / (h - 1) * 2 - 1
        ic = ic.view(1, 1, -1, 2).repeat(len(masks), 1, 1, 1)
        m = (F.grid_sample(masks, ic, align_corners=True, mode="bilinear") > 0).view(len(masks), -1)
        keep[idx[inb]] = torch.sum(m, dim=0) > 0
        for i in range(len(masks)):
            _m, md = m[i], int(modes_c[i])
            modes[idx[inb][_m]] = md
            if md == 0:
                intens[idx[inb][_m]] = 0
            if md in (2, 4):
                intens[idx[inb][_m]] = inten_c[i].to(dev)
            if md in (3, 4):
                colors[idx[inb][_m]] = col_c[i][:2].to(dev)
    return keep, modes, colors, intens


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=20_000_000)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--march-rays", type=int, default=1 << 20)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--coherent", action="store_true",
                    help="label launch only, on points laid out row-major over the view (neighbouring lanes read neighbouring "
                         "mask pixels) instead of shuffled ones: separates the mask gathers from the streaming bytes")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("relight_time.py measures on the GPU; none is visible")
    from esr_nerf_amd import relight
    from esr_nerf_amd.config import AttrDict, lts_cfg
    from esr_nerf_amd.data import RayGroupManager

    dev, S, n, ks = torch.device("cuda:0"), a.size, a.rays, 10
    g = torch.Generator(device=dev).manual_seed(0)
    # a camera 4 units from a unit cloud of surface points; about 60 % of them project into the view
    pose = torch.eye(4)
    pose[:3, 3] = torch.tensor([0.3, -0.2, 4.0])
    f = 1.2 * S
    esp = (torch.rand(n, 3, generator=g, device=dev) - 0.5) * torch.tensor([3.4, 3.4, 1.0], device=dev)
    yy, xx = torch.meshgrid(torch.arange(S, device=dev), torch.arange(S, device=dev), indexing="ij")
    disc = lambda cy, cx, r: (((yy - cy) ** 2 + (xx - cx) ** 2) <= r * r).float()
    em_masks = torch.stack([disc(0.3 * S, 0.35 * S, 0.09 * S), disc(0.55 * S, 0.6 * S, 0.12 * S) * 0.5, disc(0.5 * S, 0.5 * S, 0.05 * S)])
    modes_c, inten_c, col_c = torch.tensor([2, 3, 0]), torch.tensor([1.5, 0.5, 2.0]), torch.tensor([[0.1, 0.9, 0.5], [0.6, 0.3, 0.5], [0.8, 0.8, 0.5]])

    if a.coherent:
        side = int(np.ceil(np.sqrt(n)))
        i = torch.arange(n, device=dev)
        esp[:, 0] = ((i % side).float() / side - 0.5) * 3.4
        esp[:, 1] = ((i // side).float() / side - 0.5) * 3.4
    st = {}
    ms = {"dilate": timed(lambda: st.__setitem__("masks", relight.dilate_masks(em_masks, ks)), a.repeats)}
    ms["label"] = timed(lambda: st.__setitem__("lab", relight.label_edit_rays(esp, pose, f, S, S, st["masks"], modes_c, inten_c, col_c)),
                        a.repeats)
    lab = st["lab"]
    label_bytes = n * (12 + 21)
    label_rate = label_bytes / (ms["label"][0] * 1e-3) / 1e12
    if a.coherent:
        print(json.dumps(dict(rays=n, size=S, coherent=True, kept=int(lab["keep"].sum()), ms_median_min=ms, label_bytes=label_bytes,
                              label_tb_per_s=round(label_rate, 3), device=torch.cuda.get_device_name(0))), flush=True)
        return

    cfg = AttrDict(system=dict(device="cuda:0", data_preload="cuda"))
    data = dict(rays_o=torch.zeros(n, 3, device=dev), em_modes=torch.ones(n, dtype=torch.long, device=dev))
    samp = RayGroupManager(cfg, data, ["rays_o", "em_modes"], 4096, 4096, uncert_data_idxs=torch.randperm(n, device=dev))
    base = samp.uncert_data_idxs

    def bookkeeping():
        samp.uncert_data_idxs, samp.cert_data_idxs = base, base[:0]
        samp.keys[:] = ["rays_o", "em_modes"]
        relight.attach_edit_labels(samp, lab["keep"], lab["em_modes"], lab["em_colors"], lab["em_intensities"])

    ms["sampler_attach_and_filter"] = timed(bookkeeping, max(3, a.repeats // 2))
    per_view = round(ms["dilate"][0] + ms["label"][0] + ms["sampler_attach_and_filter"][0], 3)

    # the torch restatement of the reference's per-view lines, once warm, once timed (seconds, not milliseconds)
    args = (esp, pose, f, S, S, em_masks, ks, modes_c, inten_c, col_c, a.batch)
    torch_reference_view(esp[: 64 * a.batch], *args[1:])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ref = torch_reference_view(*args)
    torch.cuda.synchronize()
    torch_ms = (time.perf_counter() - t0) * 1e3
    agree = {k: float((r == lab[k]).reshape(n, -1).all(1).float().mean()) for k, r in zip(("keep", "em_modes", "em_colors", "em_intensities"), ref)}
    del ref

    # the once-per-checkpoint cache: eval_esp in chunks on the C2 slab scene
    march = None
    if a.march_rays > 0:
        from esr_nerf_amd.esrnerf import ESRNeRF
        from esr_nerf_amd.synthetic import init_slab_model, slab_scene
        sc = slab_scene("C2", s_val=60.0, oblique=True, n_rays=a.march_rays)
        torch.manual_seed(0)
        np.random.seed(0)
        mcfg = lts_cfg("cuda:0")
        mcfg.system["data_preload"] = "cuda"
        m = init_slab_model(ESRNeRF(mcfg, sc.near, sc.far, sc.xyz_min, sc.xyz_max, sc.mask_xyz_min, sc.mask_xyz_max,
                                    sc.mask_alpha_init, sc.mask_density, sc.s_val, sc.num_voxels), sc)
        m.s_val = sc.s_val
        m.eval()
        s2 = RayGroupManager(mcfg, {k: sc.batch[k] for k in ("rays_o", "rays_d", "viewdirs", "em_modes")},
                             ["rays_o", "rays_d", "viewdirs", "em_modes"], 4096, 4096)
        t = timed(lambda: relight.EditRaySelector(m, s2, f, (S, S), ks, a.batch), 3, warmup=1)
        march = dict(rays=a.march_rays, batch=a.batch, ms_median_min=t, ns_per_ray=round(t[0] * 1e6 / a.march_rays, 2),
                     ms_scaled_to_rays=round(t[0] * n / a.march_rays, 1))

    out = dict(rays=n, size=S, conditions=3, ks=ks, repeats=a.repeats, kept=int(lab["keep"].sum()), ms_median_min=ms,
               label_bytes=label_bytes, label_tb_per_s=round(label_rate, 3), per_view_ms_new=per_view,
               per_view_ms_torch_restatement_without_march=round(torch_ms, 1), torch_chunk=a.batch,
               rows_equal_to_torch_restatement=agree, esp_cache=march, device=torch.cuda.get_device_name(0))
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
