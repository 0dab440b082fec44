"""Times of the LPIPS (AlexNet) metric (esr_nerf_amd/lpips.py, csrc/lpips.hip) on the device.

    python tools/lpips_time.py [--size 800] [--repeats 10] [--rounds 3] [--inner 10] [--cpu-repeats 2] [--out profiles/lpips_time.json]

Seeded random weights of the exact shapes (``LpipsAlex.random(0)``) and seeded images in [0, 1]; per batch size (a pair,
and the batch of three of ``evaluate.view_metrics``):
  (a) every launch of the HIP path alone -- the five convolutions, the two pools, the five layer distances -- ``--inner``
      launches between two device events, with the convolution's FLOP (2 M K Cout) over its time and that rate as a
      fraction of the 157.3 TFLOP/s f32 matrix peak
  (b) the whole HIP path: ``features`` + ``distance`` (two distances for the batch of three), host time included
  (c) the same network as ``F.conv2d`` / ``F.max_pool2d`` in float32 on the same device (NCHW, what the ``lpips`` package
      runs), with the same normalisation and distance in torch: the BASELINE the HIP path must not be slower than
  (d) the same torch network on the CPU (host clock, ``--cpu-repeats`` runs after one warm-up)
One warm-up of every variant, then ``--rounds`` rounds that alternate (b) and (c), ``--repeats`` runs each; the figure is the
median of the rounds' medians, the spread that of the rounds' medians.  The two device paths' distances are compared.  One
JSON line; ``hip_not_slower_than_torch`` is the pass condition on time, and when it is false ``slower_by`` and the
slowest layer say by how much and where.
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

PEAK_F32_MATRIX = 157.3e12


def run_ms(fn, inner=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def summary(per_round):
    med = [float(np.median(r)) for r in per_round]
    m = float(np.median(med))
    return dict(ms=round(m, 4), ms_round_medians=[round(v, 4) for v in med], spread=round((max(med) - min(med)) / m, 4))


def torch_lpips(images, wts, pairs):
    """the network of the `lpips` package in torch ops on images [N,H,W,3]; [len(pairs)] distances (float64 on the host side
    of the caller), on the images' device"""
    from esr_nerf_amd.lpips import LAYERS
    x = images.permute(0, 3, 1, 2)
    x = (2 * x - 1 - wts["shift"].view(1, 3, 1, 1)) / wts["scale"].view(1, 3, 1, 1)
    total = [0.0 for _ in pairs]
    for l, (_, _, _, stride, pad, pooled) in enumerate(LAYERS):
        if pooled:
            x = F.max_pool2d(x, 3, 2)
        x = F.relu(F.conv2d(x, wts["conv_w"][l], wts["conv_b"][l], stride=stride, padding=pad))
        n = x / (x.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
        for q, (i, j) in enumerate(pairs):
            total[q] = total[q] + ((n[i] - n[j]).pow(2) * wts["lin"][l].view(-1, 1, 1)).sum(0).mean()
    return torch.stack(total)


def on(wts, device):
    return {k: ([t.to(device) for t in v] if isinstance(v, list) else v.to(device)) for k, v in wts.items()}


def layer_section(model, images, inner, repeats):
    """(a): each launch of the HIP path alone on the path's own intermediates"""
    from esr_nerf_amd import _lib
    from esr_nerf_amd.lpips import LAYERS, POOL_K, POOL_STRIDE, conv_out
    L, dev = _lib.lib(), model.device
    st, p = _lib.stream_ptr(dev), _lib.ptr
    N, H, W = images.shape[:3]
    feats = model.features(images)
    out, x = {}, images
    scratch = torch.empty(1025, dtype=torch.float64, device=dev)
    for l, (cin, cout, k, stride, pad, pooled) in enumerate(LAYERS):
        if pooled:
            Hp, Wp = conv_out(H, POOL_K, POOL_STRIDE, 0), conv_out(W, POOL_K, POOL_STRIDE, 0)
            y = torch.empty(N, Hp, Wp, cin, dtype=torch.float32, device=dev)
            fn = lambda x=x, y=y, H=H, W=W, cin=cin: L.esr_maxpool_nhwc(p(x), N, H, W, cin, POOL_K, POOL_STRIDE, p(y), st)
            fn()
            out[f"pool{l}"] = dict(ms=round(float(np.median([run_ms(fn, inner) for _ in range(repeats)])), 4))
            x, H, W = y, Hp, Wp
        Ho, Wo = conv_out(H, k, stride, pad), conv_out(W, k, stride, pad)
        y = torch.empty(N, Ho, Wo, cout, dtype=torch.float32, device=dev)
        aff = model._affine if l == 0 else None
        fn = lambda x=x, y=y, H=H, W=W, l=l, cin=cin, cout=cout, k=k, stride=stride, pad=pad, aff=aff: L.esr_conv_relu(
            p(x), N, H, W, cin, p(model._packed[l]), p(model._bias[l]), cout, k, k, stride, pad, p(aff), p(y), st)
        fn()
        ms = float(np.median([run_ms(fn, inner) for _ in range(repeats)]))
        flop = 2.0 * N * Ho * Wo * cin * k * k * cout
        out[f"conv{l + 1}"] = dict(ms=round(ms, 4), gflop=round(flop / 1e9, 3), tflops=round(flop / ms / 1e9, 2),
                                   fraction_of_f32_matrix_peak=round(flop / (ms * 1e-3) / PEAK_F32_MATRIX, 4),
                                   pixels=N * Ho * Wo, K=cin * k * k, Cout=cout)
        assert torch.equal(y, feats[l])
        x, H, W = y, Ho, Wo
        f = feats[l]
        fn = lambda f=f, l=l: L.esr_lpips_layer(p(f[0]), p(f[1]), f.shape[1] * f.shape[2], f.shape[3], p(model._lin[l]), p(scratch),
                                                 p(scratch[1024:]), st)
        fn()
        out[f"dist{l + 1}"] = dict(ms=round(float(np.median([run_ms(fn, inner) for _ in range(repeats)])), 4))
    out["sum_of_launches_ms"] = round(sum(v["ms"] for v in out.values()), 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--cpu-repeats", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lpips_time.py measures on the GPU; none is visible")
    from esr_nerf_amd.lpips import LpipsAlex
    dev = torch.device("cuda:0")
    model = LpipsAlex.random(0, dev)
    wts_dev, wts_cpu = on(model.weights, dev), model.weights
    g = torch.Generator().manual_seed(11)
    out = dict(size=a.size, repeats=a.repeats, rounds=a.rounds, inner=a.inner, device=torch.cuda.get_device_name(0),
               weights="LpipsAlex.random(0)", f32_matrix_peak_tflops=PEAK_F32_MATRIX / 1e12)
    for N in (2, 3):
        images_cpu = torch.rand(N, a.size, a.size, 3, generator=g)
        images = images_cpu.to(dev)
        pairs = [(0, j) for j in range(1, N)]

        def hip():
            feats = model.features(images)
            return torch.stack([model.distance(feats, i, j) for i, j in pairs])

        def tch():
            return torch_lpips(images, wts_dev, pairs)

        d_hip, d_torch = hip().tolist(), tch().double().tolist()               # warm-up of both, and their agreement
        torch.cuda.synchronize()
        times = {"hip": [], "torch_device": []}
        for _ in range(a.rounds):
            for name, fn in (("hip", hip), ("torch_device", tch)):
                times[name].append([run_ms(fn, a.inner) for _ in range(a.repeats)])
        sec = {k: summary(v) for k, v in times.items()}
        with torch.no_grad():
            torch_lpips(images_cpu, wts_cpu, pairs)
            cpu = []
            for _ in range(a.cpu_repeats):
                t0 = time.perf_counter()
                d_cpu = torch_lpips(images_cpu, wts_cpu, pairs)
                cpu.append((time.perf_counter() - t0) * 1e3)
        sec["torch_cpu"] = dict(ms=round(float(np.median(cpu)), 2), threads=torch.get_num_threads())
        sec["distances"] = dict(hip=d_hip, torch_device=d_torch, torch_cpu=d_cpu.double().tolist(),
                                worst_relative_difference_hip_torch_device=max(abs(x - y) / abs(y) for x, y in zip(d_hip, d_torch)))
        sec["launches"] = layer_section(model, images, a.inner, a.repeats)
        ok = sec["hip"]["ms"] <= sec["torch_device"]["ms"]
        sec["hip_not_slower_than_torch"] = bool(ok)
        sec["hip_over_torch_device"] = round(sec["hip"]["ms"] / sec["torch_device"]["ms"], 4)
        if not ok:
            convs = {k: v for k, v in sec["launches"].items() if k.startswith("conv")}
            worst = min(convs, key=lambda k: convs[k]["fraction_of_f32_matrix_peak"])
            sec["slower_by"] = dict(ms=round(sec["hip"]["ms"] - sec["torch_device"]["ms"], 4), slowest_layer=max(convs, key=lambda k: convs[k]["ms"]),
                                    lowest_fraction_of_peak=worst)
        out[f"batch_{N}"] = sec
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
