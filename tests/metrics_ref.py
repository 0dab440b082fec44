"""Float64, numpy-only restatement of the image-level evaluation metrics (no scipy, no torch): the yardstick of
tests/test_gpu_metrics.py and tests/test_gpu_evaluate.py, itself pinned to the reference's own output by
tests/test_metrics_host.py.

``rgb_ssim``          utils2/metric.py:31-88.  The reference squares float32 tensors (the three products are rounded to
                      float32) and scipy promotes everything behind them to float64 against the float64 filter.
``apply_gamma_curve`` utils2/image.py:14-26, evaluated in float64 on the float32 inputs
``post_image``        app/fine/fine.py:572-587 for one key, float32 operations as torch performs them
``to_u8``             (clamp01(x) * 255).astype(uint8), fine.py:611-617
``iou``               utils2/metric.py:95-98
"""
import numpy as np


def gaussian_taps(filter_size, filter_sigma):
    hw = filter_size // 2
    shift = (2 * hw - filter_size + 1) / 2
    f_i = ((np.arange(filter_size) - hw + shift) / filter_sigma) ** 2
    filt = np.exp(-0.5 * f_i)
    filt /= np.sum(filt)
    return filt


def _valid_filter(z, f):
    """convolve2d(convolve2d(z, f[:, None], "valid"), f[None, :], "valid") for z [H, W, C] float64: a convolution flips f"""
    n, (H, W) = len(f), z.shape[:2]
    v = np.zeros((H - n + 1,) + z.shape[1:])
    for k in range(n):
        v += f[k] * z[n - 1 - k:H - k]
    out = np.zeros((H - n + 1, W - n + 1) + z.shape[2:])
    for k in range(n):
        out += f[k] * v[:, n - 1 - k:W - k]
    return out


def rgb_ssim(img0, img1, max_val, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03, return_map=False):
    img0, img1 = np.asarray(img0, np.float32), np.asarray(img1, np.float32)
    assert img0.ndim == 3 and img0.shape[-1] == 3 and img0.shape == img1.shape
    if img0.shape[0] < filter_size or img0.shape[1] < filter_size:
        raise ValueError("image smaller than the filter")
    filt = gaussian_taps(filter_size, filter_sigma)
    f64 = lambda a: np.asarray(a, np.float64)
    mu0, mu1 = _valid_filter(f64(img0), filt), _valid_filter(f64(img1), filt)
    mu00, mu11, mu01 = mu0 * mu0, mu1 * mu1, mu0 * mu1
    sigma00 = _valid_filter(f64(img0 * img0), filt) - mu00          # float32 products, as img0**2 of a float32 tensor
    sigma11 = _valid_filter(f64(img1 * img1), filt) - mu11
    sigma01 = _valid_filter(f64(img0 * img1), filt) - mu01
    sigma00 = np.maximum(0.0, sigma00)
    sigma11 = np.maximum(0.0, sigma11)
    sigma01 = np.sign(sigma01) * np.minimum(np.sqrt(sigma00 * sigma11), np.abs(sigma01))
    c1, c2 = (k1 * max_val) ** 2, (k2 * max_val) ** 2
    numer = (2 * mu01 + c1) * (2 * sigma01 + c2)
    denom = (mu00 + mu11 + c1) * (sigma00 + sigma11 + c2)
    ssim_map = numer / denom
    return ssim_map if return_map else np.mean(ssim_map)


def apply_gamma_curve(image):
    x = np.asarray(image, np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(x <= np.float64(np.float32(0.0031308)), 12.92 * x, 1.055 * np.power(np.maximum(x, 0.0), 1 / 2.4) - 0.055)


def post_image(v, wbg=None, white_bg=1.0, lin=False):
    """(out, clamp01(v + wbg) or None): float32, each operation rounded once as torch rounds it; the gamma twin of a lin/
    key is apply_gamma_curve of the second value"""
    v = np.asarray(v, np.float32)
    if wbg is not None:
        w = np.asarray(wbg, np.float32) * np.float32(white_bg)
        v = v + (w[..., None] if v.ndim == w.ndim + 1 else w.reshape(v.shape))
    c01 = np.clip(v, np.float32(0), np.float32(1))
    return (np.maximum(v, np.float32(0)), c01) if lin else (c01, None)


def to_u8(x):
    return (np.clip(np.asarray(x, np.float32), np.float32(0), np.float32(1)) * np.float32(255)).astype("uint8")


def sqerr_sum(a, b):
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return float(np.sum(d * d))


def loss2psnr(loss):
    return -10 * np.log10(loss)


def iou(mask1, mask2):
    m1, m2 = np.asarray(mask1).astype(bool), np.asarray(mask2).astype(bool)
    inter = int((m1 & m2).sum())
    union = max(1, int((m1 | m2).sum()))
    return inter / union, inter, union


# ----------------------------------------------------------------------------------------------------------------------
# seeded inputs shared by the golden generator and the tests


def image_pair(kind, H, W, seed=0):
    """[H, W, 3] float32 pairs: ``noisy`` uniform noise and a perturbed copy; ``smooth`` sines plus noise of 0.01 (low
    variance: where E[x^2] - mu^2 cancels); ``negative`` the second image is the inverted first (negative covariance:
    the sign / clip of sigma01); ``identical``; ``constant``"""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    if kind == "noisy":
        a = rng.random((H, W, 3))
        b = np.clip(a + 0.1 * rng.standard_normal((H, W, 3)), 0, 1)
    elif kind == "smooth":
        base = np.stack([0.5 + 0.3 * np.sin(xx / (7.0 + c)) * np.cos(yy / (11.0 - c)) for c in range(3)], -1)
        a = base + 0.01 * rng.standard_normal((H, W, 3))
        b = base + 0.01 * rng.standard_normal((H, W, 3))
    elif kind == "negative":
        a = rng.random((H, W, 3))
        b = 1.0 - a + 0.05 * rng.standard_normal((H, W, 3))
    elif kind == "identical":
        a = rng.random((H, W, 3))
        b = a.copy()
    elif kind == "constant":
        a = np.full((H, W, 3), 0.3)
        b = a.copy()
    else:
        raise ValueError(kind)
    return a.astype(np.float32), b.astype(np.float32)


def gamma_inputs(seed=0):
    """float32 inputs of the gamma curve: exact 0 and 1, the threshold 0.0031308 and its float32 neighbours, negatives,
    values above 1, a dense sweep of [0, 1] and of the neighbourhood of the threshold"""
    rng = np.random.default_rng(seed)
    t = np.float32(0.0031308)
    special = np.array([0.0, 1.0, t, np.nextafter(t, np.float32(0)), np.nextafter(t, np.float32(1)), -0.25, -1e-6, 1.5, 7.0,
                        1e-8, 1e-4, 0.5], np.float32)
    return np.concatenate([special, rng.random(4000).astype(np.float32), (rng.random(500) * 0.01).astype(np.float32),
                           np.linspace(0, 1, 1001, dtype=np.float32)])
