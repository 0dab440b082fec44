"""Stage times of evaluating one 800 x 800 test view on the device (esr_nerf_amd/evaluate.py, esr_nerf_amd/metrics.py).

    python tools/eval_time.py [--size 800] [--batch 8192] [--repeats 20] [--host]

Event-timed after a warm-up: the render (VoxurfF on the C2 slab scene through ``render_view``; 3 repetitions, it is the
long stage), the post-processing of every result key (with the fused squared-error sums), one SSIM of the 800 x 800 x 3
pair (called twice per view), the stand-alone squared-error sum, and the whole metric side of a view (post-process +
``view_metrics``: 2 x SSIM + the MSEs, with their read-backs) by a host clock around a synchronise.  Beside the SSIM time,
with ``--host``, the wall time of the float64 numpy restatement (tests/metrics_ref.py) on the same box with the thread
count it was given.  The SSIM kernel's compulsory work is printed from the shapes: bytes read once and float64 FMAs.
One JSON line per group.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, repeats, warmup=3):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--host", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("eval_time.py measures on the GPU; none is visible")
    from esr_nerf_amd import evaluate, metrics
    from esr_nerf_amd.config import fine_cfg
    from esr_nerf_amd.synthetic import init_slab_model, slab_scene
    from esr_nerf_amd.voxurff import VoxurfF
    import metrics_ref

    S = args.size
    sc = slab_scene("C2", s_val=60.0, oblique=True, n_rays=S * S)
    torch.manual_seed(0)
    np.random.seed(0)
    m = VoxurfF(fine_cfg("cuda:0"), sc.near, sc.far, sc.xyz_min, sc.xyz_max, sc.mask_xyz_min, sc.mask_xyz_max,
                sc.mask_alpha_init, sc.mask_density, sc.s_val, sc.num_voxels)
    init_slab_model(m, sc)
    m.s_val = sc.s_val
    m.eval()
    b = {k: sc.batch[k].cuda() for k in ("rays_o", "rays_d", "viewdirs")}
    pos = torch.eye(3).cuda()
    a_host, b_host = metrics_ref.image_pair("smooth", S, S, seed=8)
    rgbs, hdrs = torch.from_numpy(b_host).cuda(), torch.from_numpy(a_host).cuda() * 1.5
    state = {}

    def render():
        state["raw"] = evaluate.render_view(m, b["rays_o"], b["rays_d"], b["viewdirs"], 1, pos, S, S, args.batch)

    def post():
        state["post"] = evaluate.postprocess_view(state["raw"], True, rgbs=rgbs, hdrs=hdrs)

    def metric_side():
        p = evaluate.postprocess_view(state["raw"], True, rgbs=rgbs, hdrs=hdrs)
        state["metrics"] = evaluate.view_metrics(p, rgbs, hdrs=hdrs, em_mode=1)

    ms = {"render": timed(render, 3, warmup=1)}
    ms["postprocess"] = timed(post, args.repeats)
    img = state["post"]["srgb/rgb"]
    scratch = {}
    ms["ssim"] = timed(lambda: scratch.__setitem__("m", metrics.rgb_ssim(img, rgbs, 1, return_map=True)), args.repeats)
    ms["ssim_with_readback"] = timed(lambda: metrics.rgb_ssim(img, rgbs, 1), args.repeats)
    ms["sqerr_sum"] = timed(lambda: metrics.sqerr_sum(img, rgbs), args.repeats)
    wall = []
    for _ in range(args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        metric_side()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    ms["metric_side_wall"] = (round(float(np.median(wall)), 4), round(float(np.min(wall)), 4))
    out = S - 10
    work = dict(bytes_read=2 * S * S * 3 * 4, map_bytes_written=out * out * 3 * 8, f64_fma=out * out * 3 * 5 * 2 * 11,
                f64_fma_with_halo=int(out * out * 3 * 5 * 11 * (1 + 42 / 32)))
    print(json.dumps(dict(size=S, batch=args.batch, keys=len(state["raw"]), repeats=args.repeats, ms_median_min=ms, ssim_work=work,
                          metrics=state["metrics"], metric_side_faster_than_render=ms["metric_side_wall"][0] < ms["render"][0],
                          device=torch.cuda.get_device_name(0))), flush=True)
    if args.host:
        x, y = img.cpu().numpy(), b_host
        t0 = time.perf_counter()
        v = metrics_ref.rgb_ssim(x, y, 1)
        s = time.perf_counter() - t0
        print(json.dumps(dict(host_numpy_ssim_s=round(s, 3), threads=torch.get_num_threads(),
                              omp_num_threads=os.environ.get("OMP_NUM_THREADS"), value=float(v),
                              device_value=metrics.rgb_ssim(img, rgbs, 1))), flush=True)


if __name__ == "__main__":
    main()
