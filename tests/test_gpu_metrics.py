"""The image metrics on the MI355X (esr_nerf_amd/metrics.py over csrc/metrics.hip) against the float64 numpy
restatement tests/metrics_ref.py and the reference's own output in tests/golden/image_metrics.npz.

Bars.  SSIM: 1e-9 absolute per map entry, 1e-10 on the mean -- both sides sum at most 121 float64 products per window
(relative rounding ~1e-15), the variance cancellation leaves ~1e-15 absolute, divided by c2 = 9e-4 that is ~1e-12 per
entry; a float32 accumulation misses by up to 4.6e-4, so the bar also guards the float64 decision.  Identical and constant
images: exactly 1.0.  Background add and clamps: bit-exact against torch on the same device tensors.  Gamma twin: 4x the
worst relative error of torch-CPU float32 apply_gamma_curve against float64 on the same inputs (measured in the test).
uint8: equal to (x * 255).astype(uint8) of the kernel's own float output.  Squared-error sum: relative 1e-12."""
import numpy as np
import pytest
import torch

import metrics_ref
from conftest import load_npz

pytestmark = pytest.mark.gpu

MAP_TOL, MEAN_TOL = 1e-9, 1e-10
GOLDEN_PAIRS = ("noisy", "smooth", "negative", "fs7")


def _check_pair(a, b, what, **kw):
    from esr_nerf_amd import metrics
    want = metrics_ref.rgb_ssim(a, b, 1, return_map=True, **kw)
    got = metrics.rgb_ssim(a, b, 1, return_map=True, **kw)
    assert got.dtype == torch.float64 and got.is_cuda and tuple(got.shape) == want.shape, what
    err = float(np.abs(got.cpu().numpy() - want).max())
    mean = metrics.rgb_ssim(a, b, 1, **kw)
    assert isinstance(mean, float)
    merr = abs(mean - float(np.mean(want)))
    print(f"{what}: map err {err:.3e}, mean err {merr:.3e}, mean {mean:.6f}")
    assert err <= MAP_TOL, (what, err)
    assert merr <= MEAN_TOL, (what, merr)
    return got, mean


@pytest.mark.parametrize("name", GOLDEN_PAIRS)
def test_ssim_matches_the_reference_golden(name):
    from esr_nerf_amd import metrics
    z = load_npz("image_metrics.npz")
    fs, sigma = int(z[f"{name}/filter"][0]), float(z[f"{name}/filter"][1])
    got = metrics.rgb_ssim(z[f"{name}/img0"], z[f"{name}/img1"], 1, filter_size=fs, filter_sigma=sigma, return_map=True)
    assert tuple(got.shape) == z[f"{name}/map"].shape
    err = float(np.abs(got.cpu().numpy() - z[f"{name}/map"]).max())
    mean = metrics.rgb_ssim(z[f"{name}/img0"], z[f"{name}/img1"], 1, filter_size=fs, filter_sigma=sigma)
    print(f"{name}: map err {err:.3e}, mean err {abs(mean - float(z[name + '/mean'])):.3e}")
    assert err <= MAP_TOL
    assert abs(mean - float(z[f"{name}/mean"])) <= MEAN_TOL


@pytest.mark.parametrize("kind,H,W", [("noisy", 11, 11), ("noisy", 43, 75), ("smooth", 64, 64), ("noisy", 65, 97),
                                      ("smooth", 200, 200), ("negative", 52, 29), ("noisy", 11, 40), ("noisy", 90, 11)])
def test_ssim_sizes_and_content(kind, H, W):
    a, b = metrics_ref.image_pair(kind, H, W, seed=H * 131 + W)
    got, _ = _check_pair(a, b, f"{kind} {H}x{W}")
    assert tuple(got.shape) == (H - 10, W - 10, 3)
    if kind == "negative":
        assert float(got.min()) < 0                          # the sign of sigma01 survived the clip


def test_ssim_800x800():
    a, b = metrics_ref.image_pair("smooth", 800, 800, seed=8)
    _check_pair(a, b, "smooth 800x800")


@pytest.mark.parametrize("fs,sigma", [(7, 1.0), (8, 2.0), (1, 1.5), (33, 5.0)])
def test_ssim_other_filters(fs, sigma):
    a, b = metrics_ref.image_pair("smooth", 70, 83, seed=fs)
    got, _ = _check_pair(a, b, f"filter {fs}/{sigma}", filter_size=fs, filter_sigma=sigma)
    assert tuple(got.shape) == (70 - fs + 1, 83 - fs + 1, 3)


@pytest.mark.parametrize("kind", ["identical", "constant"])
def test_ssim_identical_and_constant_images_are_exactly_one(kind):
    from esr_nerf_amd import metrics
    a, b = metrics_ref.image_pair(kind, 75, 58, seed=5)
    m = metrics.rgb_ssim(a, b, 1, return_map=True)
    assert bool((m == 1.0).all())
    assert metrics.rgb_ssim(a, b, 1) == 1.0


def test_ssim_is_deterministic_and_takes_every_input_form():
    from esr_nerf_amd import metrics
    a, b = metrics_ref.image_pair("noisy", 130, 117, seed=9)
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    m0, m1 = metrics.rgb_ssim(da, db, 1, return_map=True), metrics.rgb_ssim(da, db, 1, return_map=True)
    assert torch.equal(m0, m1)
    means = [metrics.rgb_ssim(da, db, 1), metrics.rgb_ssim(da, db, 1), metrics.rgb_ssim(a, b, 1),
             metrics.rgb_ssim(torch.from_numpy(a), torch.from_numpy(b), 1), metrics.rgb_ssim(da, b, 1)]
    assert all(np.float64(v).tobytes() == np.float64(means[0]).tobytes() for v in means)
    assert torch.equal(metrics.rgb_ssim(a, torch.from_numpy(b), 1, return_map=True), m0)
    with pytest.raises(ValueError):
        metrics.rgb_ssim(da[:10], db[:10], 1)


def test_ssim_entry_point_refuses_what_the_kernel_cannot_do():
    import ctypes as C
    from esr_nerf_amd import _lib, metrics
    L = _lib.lib()
    a = torch.zeros(40, 40, 3, device="cuda")
    scratch = torch.zeros(1025, dtype=torch.float64, device="cuda")

    def call(H, W, fs):
        taps = metrics.gaussian_taps(fs, 1.5)
        return L.esr_ssim(_lib.ptr(a), _lib.ptr(a), H, W, taps.ctypes.data_as(C.c_void_p), fs, C.c_double(1e-4),
                          C.c_double(9e-4), None, _lib.ptr(scratch), C.c_void_p(scratch.data_ptr() + 8192), None)
    assert call(10, 40, 11) == -1 and call(40, 10, 11) == -1          # ESR_EINVAL
    assert call(40, 40, 34) == -2                                     # ESR_ECAP
    assert call(40, 40, 11) == 0
    torch.cuda.synchronize()


def _post_case(C, seed=0, n=5000):
    g = torch.Generator().manual_seed(seed)
    v = (torch.rand(n, C, generator=g) * 1.6 - 0.3)
    v[::7] = 0.0
    v[1::11] = 1.0
    wbg = torch.rand(n, generator=g)
    wbg[::5] = 0.0
    wbg[3::9] = 1.0
    return (v if C > 1 else v[:, 0]).contiguous(), wbg


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("white_bg", [1.0, 0.0])
def test_post_image_background_and_clamps_are_bit_exact(C, white_bg):
    from esr_nerf_amd import metrics
    v, wbg = _post_case(C, seed=C)
    dv, dw = v.cuda(), wbg.cuda()
    w = dw * white_bg
    s = dv + (w.unsqueeze(-1) if C > 1 else w)
    r = metrics.post_image(dv, dw, white_bg)
    assert torch.equal(r["out"], s.clamp(min=0.0, max=1.0)) and "gamma" not in r
    r = metrics.post_image(dv, dw, white_bg, lin=True, want_u8=True)
    assert torch.equal(r["out"], s.clamp(min=0.0))
    c01 = s.clamp(min=0.0, max=1.0)
    want = metrics_ref.apply_gamma_curve(c01.cpu().numpy())
    bar = _gamma_bar(c01.cpu())
    rel = np.abs(r["gamma"].cpu().numpy() - want) / np.maximum(np.abs(want), 1e-30)
    print(f"gamma twin: worst relative error {float(rel.max()):.3e} (bar {bar:.3e})")
    assert float(rel.max()) <= bar
    # uint8 images: one multiply and a truncation of the kernel's own float output, no tolerance
    for f in ("out", "gamma"):
        own = r[f].cpu().numpy()
        assert np.array_equal(r[f + "_u8"].cpu().numpy(), (np.clip(own, 0, 1) * np.float32(255)).astype("uint8")), f
    only = metrics.post_image(dw)                              # etc/white_bg itself: clamped only
    assert torch.equal(only["out"], dw.clamp(min=0.0, max=1.0))


def _torch_cpu_gamma(x):
    """utils2/image.py:14-26 as the reference runs it: float32 on the CPU"""
    rst = torch.empty_like(x)
    low = x <= 0.0031308
    rst[low] = 12.92 * x[low]
    rst[~low] = 1.055 * torch.pow(x[~low], 1 / 2.4) - 0.055
    return rst


def _gamma_bar(x_cpu):
    """4 x the worst relative error of torch-CPU float32 apply_gamma_curve against float64 on these inputs"""
    want = metrics_ref.apply_gamma_curve(x_cpu.numpy())
    got = _torch_cpu_gamma(x_cpu).numpy()
    worst = float((np.abs(got - want) / np.maximum(np.abs(want), 1e-30)).max())
    print(f"torch-CPU float32 gamma against float64: worst relative error {worst:.3e}")
    return 4 * worst


def test_gamma_curve_on_the_edge_inputs():
    from esr_nerf_amd import metrics
    x = torch.from_numpy(metrics_ref.gamma_inputs())
    want = metrics_ref.apply_gamma_curve(x.numpy())
    bar = _gamma_bar(x)
    got = metrics.apply_gamma_curve(x.cuda()).cpu().numpy()
    rel = np.abs(got - want) / np.maximum(np.abs(want), 1e-30)
    print(f"device gamma against float64: worst relative error {float(rel.max()):.3e} (bar {bar:.3e})")
    assert float(rel.max()) <= bar
    low = x.numpy() <= np.float32(0.0031308)
    assert np.array_equal(got[low], np.float32(12.92) * x.numpy()[low])      # the linear branch is one float32 product
    assert got[0] == 0.0 and got[1] == pytest.approx(1.0, rel=bar)
    z = load_npz("image_metrics.npz")
    rel = np.abs(metrics.apply_gamma_curve(z["gamma/x"]).cpu().numpy() - z["gamma/y"]) / np.maximum(np.abs(z["gamma/y"]), 1e-30)
    assert float(rel.max()) <= 2 * bar                        # two float32 evaluations, each within the bar of float64


@pytest.mark.parametrize("n", [1, 1000, 800 * 800 * 3])
def test_squared_error_sums(n):
    from esr_nerf_amd import metrics
    g = torch.Generator().manual_seed(n)
    a, b = torch.rand(n, generator=g), torch.rand(n, generator=g)
    want = metrics_ref.sqerr_sum(a.numpy(), b.numpy())
    da, db = a.cuda(), b.cuda()
    got = metrics.sqerr_sum(da, db)
    assert got.dtype == torch.float64 and got.shape == (1,)
    print(f"n {n}: sum {float(got):.15e}, relative error {abs(float(got) - want) / want:.3e}")
    assert abs(float(got) - want) <= 1e-12 * want
    assert torch.equal(got, metrics.sqerr_sum(da, db))         # deterministic
    mse = float(got) / n
    assert float(metrics.loss2psnr(mse)) == pytest.approx(metrics_ref.loss2psnr(want / n), abs=1e-10)


def test_post_image_fused_squared_errors():
    from esr_nerf_amd import metrics
    v, wbg = _post_case(3, seed=4, n=48 * 40)
    g = torch.Generator().manual_seed(1)
    rgbs, hdrs = torch.rand(48 * 40, 3, generator=g), torch.rand(48 * 40, 3, generator=g) * 2
    r = metrics.post_image(v.cuda(), wbg.cuda(), 1.0, lin=True, target=hdrs.cuda(), target_gamma=rgbs.cuda())
    for key, img, tgt in (("sqerr", r["out"], hdrs), ("sqerr_gamma", r["gamma"], rgbs)):
        want = metrics_ref.sqerr_sum(img.cpu().numpy(), tgt.numpy())
        assert abs(float(r[key]) - want) <= 1e-12 * want, key
        assert torch.equal(r[key], metrics.sqerr_sum(img, tgt.cuda())), key
    r = metrics.post_image(v.cuda(), wbg.cuda(), 1.0, target=rgbs.cuda())
    want = metrics_ref.sqerr_sum(r["out"].cpu().numpy(), rgbs.numpy())
    assert abs(float(r["sqerr"]) - want) <= 1e-12 * want


def test_iou_counts_are_exact():
    from esr_nerf_amd import metrics
    z = load_npz("image_metrics.npz")
    assert list(metrics.IoU(z["iou/mask1"], z["iou/mask2"])) == list(z["iou/result"])
    rng = np.random.default_rng(0)
    m1, m2 = rng.random((800, 800)) > 0.7, rng.random((800, 800)) > 0.4
    want = metrics_ref.iou(m1, m2)
    assert metrics.IoU(torch.from_numpy(m1).cuda(), torch.from_numpy(m2).cuda()) == want
    assert metrics.IoU(m1.astype(np.uint8), torch.from_numpy(m2)) == want
    none = np.zeros((33, 7), bool)
    assert metrics.IoU(none, none) == (0.0, 0, 1)
    assert metrics.IoU(m1, m1) == (1.0, int(m1.sum()), int(m1.sum()))
