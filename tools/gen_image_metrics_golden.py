"""Write tests/golden/image_metrics.npz: the reference's own utils2.metric.rgb_ssim / IoU / loss2psnr and
utils2.image.apply_gamma_curve on small seeded inputs.

    python tools/gen_image_metrics_golden.py            (CPU host with the reference tree and scipy)

The reference modules are loaded by path with lpips / trimesh / sklearn / wandb stubbed (tools/gen_dtu_cd_golden.py's
``load_metric``).  The inputs come from tests/metrics_ref.py (``image_pair``, ``gamma_inputs``); only data goes into the
file: per pair the two float32 images, the float64 map and mean; the gamma inputs and outputs; a mask pair with its
counts; a few losses with their PSNR.  The tests only read the .npz.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
OUT = os.path.join(ROOT, "tests", "golden", "image_metrics.npz")

# name -> (kind, H, W, seed, filter_size, filter_sigma)
PAIRS = {
    "noisy": ("noisy", 40, 52, 1, 11, 1.5),
    "smooth": ("smooth", 72, 64, 2, 11, 1.5),
    "negative": ("negative", 33, 47, 3, 11, 1.5),
    "fs7": ("noisy", 50, 45, 4, 7, 1.0),
}


def main():
    import gen_dtu_cd_golden as g
    import metrics_ref
    sys.modules.setdefault("sklearn", types.ModuleType("sklearn"))
    sys.modules.setdefault("sklearn.neighbors", types.ModuleType("sklearn.neighbors"))
    metric = g.load_metric()
    spec = importlib.util.spec_from_file_location("ref_image", os.path.join(g.REF_ROOT, "utils2", "image.py"))
    image = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(image)

    out = {}
    for name, (kind, H, W, seed, fs, sigma) in PAIRS.items():
        a, b = metrics_ref.image_pair(kind, H, W, seed)
        ta, tb = torch.from_numpy(a), torch.from_numpy(b)       # float32 tensors, as evaluate() passes them
        out[f"{name}/img0"], out[f"{name}/img1"] = a, b
        out[f"{name}/filter"] = np.array([fs, sigma], np.float64)
        out[f"{name}/map"] = np.asarray(metric.rgb_ssim(ta, tb, 1, filter_size=fs, filter_sigma=sigma, return_map=True), np.float64)
        out[f"{name}/mean"] = np.float64(metric.rgb_ssim(ta, tb, 1, filter_size=fs, filter_sigma=sigma))
    x = metrics_ref.gamma_inputs()
    out["gamma/x"] = x
    out["gamma/y"] = image.apply_gamma_curve(torch.from_numpy(x)).numpy()
    rng = np.random.default_rng(5)
    m1, m2 = rng.random((37, 41)) > 0.6, rng.random((37, 41)) > 0.5
    ratio, inter, union = metric.IoU(torch.from_numpy(m1), torch.from_numpy(m2))
    out["iou/mask1"], out["iou/mask2"] = m1, m2
    out["iou/result"] = np.array([ratio, inter, union], np.float64)
    loss = np.array([1e-4, 3.7e-3, 0.25, 1.0], np.float64)
    out["psnr/loss"], out["psnr/psnr"] = loss, np.array([metric.loss2psnr(float(v)) for v in loss], np.float64)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} B): " + ", ".join(f"{n} {float(out[n + '/mean']):.6f}" for n in PAIRS))


if __name__ == "__main__":
    main()
