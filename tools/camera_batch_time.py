"""Camera-defined ray sets against per-ray arrays at production scale (esr_nerf_amd/camera.py):

    python tools/camera_batch_time.py [--views 100] [--size 800] [--batch 8192] [--repeats 20] [--out FILE]

Workload: ``--views`` pinhole cameras of ``--size`` x ``--size`` pixels on a sphere of radius 4 around the box
(-1,-1,-1)..(1,1,1) (focal 1111 at 800 pixels, near 2, far 6), random RGBA8 images, and the renderer of
tools/ray_filter_time.py (fine, 256^3, a blob mask at 100^3).  Measured, one process:

  sample        ``sample()`` at ``--batch`` rays for ``BatchSampler`` on the materialised arrays against ``CameraBatchSampler``:
                device time (events around a run of calls) and host time (wall clock of the calls alone, the queue drained
                before and after), per call
  resident      bytes each form keeps on the device (arithmetic on the tensors actually held)
  filter        ``filter_rays`` on the materialised rays against ``filter_camera_rays``, both sampling modes; the flags must be equal
  bbox          ``frustum_bbox`` against the reference's torch loop over the materialised rays (app/coarse/alphamask.py:108-122)

No speed gate: the numbers are recorded whichever way they fall.  One JSON line.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def sphere_poses(views, seed=0):
    """float32 [views, 3, 4] camera-to-world (x right, y down, z forward) on a sphere of radius 4, looking at the origin"""
    import camera_ref as CR
    g = np.random.default_rng(seed)
    out = []
    for _ in range(views):
        az, el = g.random() * 2 * math.pi, math.radians(5 + 70 * g.random())
        out.append(CR.look_at_cv((4 * math.cos(el) * math.cos(az), 4 * math.cos(el) * math.sin(az), 4 * math.sin(el)), (0, 0, 0)))
    return np.stack(out)


def device_and_host_us(fn, calls, repeats):
    """(device microseconds, host microseconds) per call of fn: medians over `repeats` runs of `calls` calls"""
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    dev, host = [], []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        t1 = time.perf_counter()
        e1.record()
        e1.synchronize()
        dev.append(e0.elapsed_time(e1) * 1e3 / calls)
        host.append((t1 - t0) * 1e6 / calls)
    return round(float(np.median(dev)), 2), round(float(np.median(host)), 2)


def event_ms(fn, repeats, warmup=2):
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
    return round(float(np.median(ms)), 3)


def torch_bbox(ro, vd, near, far, chunk):
    """alphamask.py:108-122"""
    lo = torch.full((3,), float("inf"), device=ro.device)
    hi = -lo
    for o, v in zip(ro.split(chunk, 0), vd.split(chunk, 0)):
        pts = torch.stack([o + v * near, o + v * far])
        lo, hi = torch.minimum(lo, pts.amin((0, 1))), torch.maximum(hi, pts.amax((0, 1)))
    return lo, hi


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--calls", type=int, default=50, help="sample() calls per timed run")
    ap.add_argument("--chunk", type=int, default=16384, help="the torch bbox loop's chunk (the configs' eval batch size)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("camera_batch_time.py measures on the GPU; none is visible")
    from esr_nerf_amd.camera import CameraBatchSampler, Cameras, camera_batch, camera_rays, filter_camera_rays, frustum_bbox
    from esr_nerf_amd.config import AttrDict, fine_cfg
    from esr_nerf_amd.data import BatchSampler
    from esr_nerf_amd.rayfilter import filter_rays
    from esr_nerf_amd.voxurff import VoxurfF
    from ray_filter_time import blob_density

    dev = torch.device("cuda:0")
    hw = a.size * a.size
    K = np.array([[1111.0 * a.size / 800.0, 0, a.size * 0.5], [0, 1111.0 * a.size / 800.0, a.size * 0.5], [0, 0, 1.0]])
    cams = Cameras.from_intrinsics(sphere_poses(a.views), K, a.size, a.size, device=dev)
    g = torch.Generator(device=dev).manual_seed(1)
    rgba = torch.randint(0, 256, (cams.n_rays, 4), dtype=torch.uint8, device=dev, generator=g)
    modes = (torch.arange(a.views, device=dev) % 2).long()
    keys = ["rgbs", "rays_o", "rays_d", "viewdirs", "em_modes"]
    cfg = AttrDict(system=dict(device="cuda:0", data_preload="cuda"), data=dict(white_bg=True))
    out = dict(views=a.views, size=a.size, rays=cams.n_rays, batch=a.batch, device=torch.cuda.get_device_name(0))

    # the materialised form, made by the kernels themselves: dense rays, colours in view-sized batches
    ro, rd, vd = camera_rays(cams)
    rgbs = torch.cat([camera_batch(cams, rgba, modes, torch.arange(v * hw, (v + 1) * hw, device=dev), True, check_rows=False)["rgbs"]
                      for v in range(a.views)])
    data = dict(rays_o=ro, rays_d=rd, viewdirs=vd, rgbs=rgbs, em_modes=modes.repeat_interleave(hw))
    out["resident_bytes"] = dict(
        arrays=int(sum(t.numel() * t.element_size() for t in data.values())),
        cameras=int(cams.poses.numel() * 4 + rgba.numel() + modes.numel() * 8),
        index_vector=int(cams.n_rays * 8))

    torch.manual_seed(0)
    arr = BatchSampler(cfg, data, keys, a.batch)
    torch.manual_seed(0)
    cam = CameraBatchSampler(cfg, cams, rgba, modes, keys, a.batch)
    for s in (arr, cam):
        s.shuffle()
    x, y = arr.sample(), cam.sample()
    assert all(torch.equal(x[k], y[k]) for k in keys), "the two samplers' batches differ"
    out["sample_us"] = {}
    for name, s in (("arrays", arr), ("cameras", cam)):
        d, h = device_and_host_us(s.sample, a.calls, a.repeats)
        out["sample_us"][name] = dict(device=d, host=h)
    print("sample", json.dumps(out["sample_us"]), flush=True)

    lo, hi = torch.tensor([-1.0, -1.0, -1.0]), torch.tensor([1.0, 1.0, 1.0])
    torch.manual_seed(0)
    np.random.seed(0)
    m = VoxurfF(fine_cfg("cuda:0"), 2.0, 6.0, lo, hi, lo.clone(), hi.clone(), 1e-6, blob_density(100, dev), 20.0, 256 ** 3)
    out["filter_ms"] = {}
    for name, fixed in (("march", False), ("fixed", True)):
        m.sdf_random_init = fixed
        assert torch.equal(filter_rays(m, ro, rd, fixed), filter_camera_rays(m, cams, fixed)), name
        out["filter_ms"][name] = dict(arrays=event_ms(lambda: filter_rays(m, ro, rd, fixed), 5),
                                      cameras=event_ms(lambda: filter_camera_rays(m, cams, fixed), 5))
    print("filter", json.dumps(out["filter_ms"]), flush=True)

    blo, bhi = frustum_bbox(cams, 2.0, 6.0)
    tlo, thi = torch_bbox(ro, vd, 2.0, 6.0, a.chunk)
    assert float((blo - tlo).abs().max()) <= 1e-5 and float((bhi - thi).abs().max()) <= 1e-5
    out["bbox_ms"] = dict(kernel=event_ms(lambda: frustum_bbox(cams, 2.0, 6.0), 5),
                          torch_loop=event_ms(lambda: torch_bbox(ro, vd, 2.0, 6.0, a.chunk), 3, warmup=1))
    out["dense_rays_ms"] = event_ms(lambda: camera_rays(cams), 5)
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
