"""The image metrics' CPU side: the float64 numpy restatement tests/metrics_ref.py against the reference's own output
(tests/golden/image_metrics.npz, tools/gen_image_metrics_golden.py) and, where the reference tree and scipy exist, live
against the imported reference function.  This pins the yardstick the GPU tests use; it also checks the module's host
logic (the filter taps, argument errors, no fallback without a device)."""
import os
import sys

import numpy as np
import pytest

import metrics_ref
from conftest import ROOT, load_npz

PAIRS = ("noisy", "smooth", "negative", "fs7")
# both sides are float64 evaluations of the same window sums in a different order (at most 121 products of relative
# rounding 1e-16, the variance cancellation divided by c2 = 9e-4: ~1e-12 per entry)
MAP_TOL = 1e-10


@pytest.mark.parametrize("name", PAIRS)
def test_restatement_matches_the_reference_golden(name):
    z = load_npz("image_metrics.npz")
    fs, sigma = int(z[f"{name}/filter"][0]), float(z[f"{name}/filter"][1])
    got = metrics_ref.rgb_ssim(z[f"{name}/img0"], z[f"{name}/img1"], 1, filter_size=fs, filter_sigma=sigma, return_map=True)
    want = z[f"{name}/map"]
    assert got.shape == want.shape == (z[f"{name}/img0"].shape[0] - fs + 1, z[f"{name}/img0"].shape[1] - fs + 1, 3)
    err = float(np.abs(got - want).max())
    print(f"{name}: max |restatement - reference| per map entry {err:.3e}")
    assert err <= MAP_TOL
    mean = metrics_ref.rgb_ssim(z[f"{name}/img0"], z[f"{name}/img1"], 1, filter_size=fs, filter_sigma=sigma)
    assert abs(mean - float(z[f"{name}/mean"])) <= MAP_TOL


def test_golden_covers_a_negative_covariance_and_a_non_default_filter():
    z = load_npz("image_metrics.npz")
    assert float(z["negative/mean"]) < -0.5 and float(z["negative/map"].min()) < 0
    assert tuple(z["fs7/filter"]) == (7.0, 1.0) and tuple(z["noisy/filter"]) == (11.0, 1.5)


def test_restatement_gamma_iou_psnr_match_the_reference_golden():
    z = load_npz("image_metrics.npz")
    x, y = z["gamma/x"], z["gamma/y"]
    got = metrics_ref.apply_gamma_curve(x)
    assert np.all(np.isfinite(y))                             # negatives take the linear branch
    # the reference evaluates in float32: a few float32 roundings (the product, powf, the sum) of values up to ~2.5
    rel = np.abs(got - y) / np.maximum(np.abs(got), 1e-30)
    print(f"gamma: reference float32 against float64, worst relative error {float(rel.max()):.3e}")
    assert float(rel.max()) < 8 * 2.0 ** -24
    low = x <= np.float32(0.0031308)
    assert np.array_equal(np.float32(12.92) * x[low], y[low])
    ratio, inter, union = metrics_ref.iou(z["iou/mask1"], z["iou/mask2"])
    assert [ratio, inter, union] == list(z["iou/result"])
    assert np.array_equal(metrics_ref.loss2psnr(z["psnr/loss"]), z["psnr/psnr"])


def test_restatement_live_against_the_reference_function():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_dtu_cd_golden as g
    if not os.path.exists(os.path.join(g.REF_ROOT, "utils2", "metric.py")):
        pytest.skip("no reference tree on this host")
    pytest.importorskip("scipy.signal")
    import torch
    metric = g.load_metric()
    a, b = metrics_ref.image_pair("smooth", 45, 61, seed=11)
    for kw in (dict(), dict(filter_size=8, filter_sigma=2.0)):
        want = metric.rgb_ssim(torch.from_numpy(a), torch.from_numpy(b), 1, return_map=True, **kw)
        got = metrics_ref.rgb_ssim(a, b, 1, return_map=True, **kw)
        assert float(np.abs(got - np.asarray(want)).max()) <= MAP_TOL


def test_identical_and_constant_images_give_exactly_one_in_the_restatement():
    for kind in ("identical", "constant"):
        a, b = metrics_ref.image_pair(kind, 30, 26, seed=3)
        assert np.all(metrics_ref.rgb_ssim(a, b, 1, return_map=True) == 1.0)


def test_module_taps_equal_the_restatements_and_sum_to_one():
    from esr_nerf_amd import metrics
    for fs, sigma in ((11, 1.5), (7, 1.0), (8, 2.0), (33, 4.0)):
        t = metrics.gaussian_taps(fs, sigma)
        assert t.dtype == np.float64 and np.array_equal(t, metrics_ref.gaussian_taps(fs, sigma))
        assert abs(t.sum() - 1.0) < 1e-15 and np.array_equal(t, t[::-1])
    assert float(metrics.loss2psnr(0.01)) == 20.0


def test_argument_errors_come_before_any_device_work():
    from esr_nerf_amd import metrics
    a = np.zeros((10, 40, 3), np.float32)
    with pytest.raises(ValueError):
        metrics.rgb_ssim(a, a, 1)                            # H < filter_size, as scipy's "valid" mode refuses it
    with pytest.raises(ValueError):
        metrics.rgb_ssim(np.zeros((40, 10, 3), np.float32), np.zeros((40, 10, 3), np.float32), 1)
    with pytest.raises(ValueError):
        metrics.rgb_ssim(np.zeros((40, 40, 3), np.float32), np.zeros((40, 41, 3), np.float32), 1)
    with pytest.raises(ValueError):
        metrics.rgb_ssim(np.zeros((40, 40, 3), np.float32), np.zeros((40, 40, 3), np.float32), 1, filter_size=35)
    with pytest.raises(ValueError):
        metrics.IoU(np.zeros(4, np.float32), np.zeros(4, np.float32))


def test_no_cpu_fallback_for_cpu_resident_view_images():
    import torch
    from esr_nerf_amd import metrics
    with pytest.raises(ValueError):
        metrics.post_image(torch.zeros(4, 3))               # the view loop's images live on the device
