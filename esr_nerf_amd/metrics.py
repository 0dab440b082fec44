"""Image-level evaluation metrics on the device: the reference's ``utils2.metric.rgb_ssim`` / ``IoU`` / ``loss2psnr``
and ``utils2.image.apply_gamma_curve`` over libesr_hip.so's kernels (esr_nerf_amd/csrc/metrics.hip).

``rgb_ssim``           the reference's signature; float (or the float64 map as a device tensor with ``return_map``)
``rgb_lpips``          the reference's signature (AlexNet only), on the model ``set_lpips`` was given (lpips.py)
``IoU``                (ratio, intersection, union) of two bool / uint8 masks
``loss2psnr``          -10 log10(loss)
``apply_gamma_curve``  the sRGB curve in float32
``sqerr_sum``          float64 sum of squared differences of two float32 images (MSE = sum / numel on the host)
``post_image``         one result image of a view: background, clamps, gamma twin, uint8 images, squared-error sums

Inputs may be device tensors (used in place), CPU tensors or numpy arrays (uploaded to the current device).  There is
no scipy and no CPU path: without the library every call raises.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib

MAX_FILTER_SIZE = _lib.SSIM_MAX_TAPS
_BLOCKS = _lib.METRICS_BLOCKS


def _dev(device=None):
    return torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())


def _on_device(x, dtype, device=None) -> torch.Tensor:
    """x as a contiguous ``dtype`` tensor on the device: a device tensor of that dtype and layout is returned as is"""
    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(np.ascontiguousarray(x))
    dev = x.device if x.is_cuda else _dev(device)
    return x.to(device=dev, dtype=dtype).contiguous()


def _same_device(*tensors):
    dev = tensors[0].device
    if any(t.device != dev for t in tensors):
        raise ValueError("metrics: the inputs live on different devices")
    return dev


def gaussian_taps(filter_size: int, filter_sigma: float) -> np.ndarray:
    """The reference's 1-D filter (utils2/metric.py:47-51), float64"""
    hw = filter_size // 2
    shift = (2 * hw - filter_size + 1) / 2
    f_i = ((np.arange(filter_size) - hw + shift) / filter_sigma) ** 2
    filt = np.exp(-0.5 * f_i)
    filt /= np.sum(filt)
    return filt


def rgb_ssim(img0, img1, max_val, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03, return_map=False):
    """utils2/metric.py:31-88.  img0, img1 [H, W, 3]; returns the mean SSIM as a float, or with ``return_map`` the map
    [H-fs+1, W-fs+1, 3] (float64, on the device)."""
    if len(img0.shape) != 3 or img0.shape[-1] != 3 or tuple(img0.shape) != tuple(img1.shape):
        raise ValueError(f"rgb_ssim: expected two [H, W, 3] images, got {tuple(img0.shape)} and {tuple(img1.shape)}")
    filter_size = int(filter_size)
    H, W = int(img0.shape[0]), int(img0.shape[1])
    if filter_size < 1 or H < filter_size or W < filter_size:
        raise ValueError(f"rgb_ssim: a {H} x {W} image is smaller than the {filter_size}-tap filter")
    if filter_size > MAX_FILTER_SIZE:
        raise ValueError(f"rgb_ssim: filter_size {filter_size} exceeds the kernel's {MAX_FILTER_SIZE} taps")
    a = _on_device(img0, torch.float32)
    b = _on_device(img1, torch.float32, a.device)
    dev = _same_device(a, b)
    taps = gaussian_taps(filter_size, filter_sigma)
    c1, c2 = (k1 * max_val) ** 2, (k2 * max_val) ** 2
    with torch.cuda.device(dev):
        ssim_map = torch.empty(H - filter_size + 1, W - filter_size + 1, 3, dtype=torch.float64, device=dev) if return_map else None
        scratch = torch.empty(_BLOCKS + 1, dtype=torch.float64, device=dev)
        _lib.check(_lib.lib().esr_ssim(_lib.ptr(a), _lib.ptr(b), H, W, taps.ctypes.data_as(C.c_void_p), filter_size,
                                       c1, c2, _lib.ptr(ssim_map), _lib.ptr(scratch),
                                       C.c_void_p(scratch.data_ptr() + 8 * _BLOCKS), _lib.stream_ptr(dev)), "esr_ssim")
        return ssim_map if return_map else float(scratch[_BLOCKS])


_LPIPS = {}                   # net_name -> lpips.LpipsAlex (the reference's __LPIPS__, utils2/metric.py:12)


def set_lpips(model_or_path, backbone_path=None, device=None):
    """Give ``rgb_lpips`` its model: an ``lpips.LpipsAlex``, or the path of a state-dict file (``LpipsAlex.from_file``; with
    ``backbone_path`` the pair of the package's ``alex.pth`` and torchvision's AlexNet).  ``None`` removes it.  Returns the
    model."""
    from .lpips import LpipsAlex
    if model_or_path is None:
        _LPIPS.pop("alex", None)
        return None
    model = model_or_path if isinstance(model_or_path, LpipsAlex) else LpipsAlex.from_file(model_or_path, backbone_path, device)
    _LPIPS["alex"] = model
    return model


def rgb_lpips(np_gt, np_im, net_name="alex", device=None):
    """utils2/metric.py:21-28: the LPIPS distance of two [H, W, 3] images in [0, 1] (numpy or tensors), as a float.
    ``net_name`` "alex" only.  The trained weights are the user's to supply, once, through ``set_lpips``."""
    if net_name == "vgg":
        raise NotImplementedError("rgb_lpips: the VGG backbone is not provided, only net_name='alex'")
    if net_name != "alex":
        raise ValueError(f"rgb_lpips: unknown net_name {net_name!r}")
    model = _LPIPS.get("alex")
    if model is None:
        raise RuntimeError("rgb_lpips: no LPIPS model is set.  No trained weights travel with this package: call "
                           "metrics.set_lpips(path) with the state dict of lpips.LPIPS(net='alex') saved by torch.save "
                           "(or set_lpips(alex_pth, backbone_path=torchvision_alexnet_pth)), or pass an lpips.LpipsAlex")
    if device is not None and torch.device(device).type == "cuda" and torch.device(device).index not in (None, model.device.index):
        raise ValueError(f"rgb_lpips: the model lives on {model.device}, not on {device}")
    return model(np_gt, np_im)


def loss2psnr(loss: float):
    return -10 * np.log10(loss)


def IoU(mask1, mask2):
    """utils2/metric.py:95-98: (intersection / max(1, union), intersection, max(1, union)) as Python numbers"""
    m1, m2 = _mask(mask1), _mask(mask2, getattr(mask1, "device", None) if getattr(mask1, "is_cuda", False) else None)
    if m1.shape != m2.shape:
        raise ValueError(f"IoU: mask shapes differ, {tuple(m1.shape)} and {tuple(m2.shape)}")
    dev = _same_device(m1, m2)
    with torch.cuda.device(dev):
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        _lib.check(_lib.lib().esr_mask_iou(_lib.ptr(m1), _lib.ptr(m2), m1.numel(), _lib.ptr(counts), _lib.stream_ptr(dev)),
                   "esr_mask_iou")
        inter, union = counts.tolist()
    union = max(1, union)
    return inter / union, inter, union


def _mask(m, device=None) -> torch.Tensor:
    if not isinstance(m, torch.Tensor):
        m = torch.from_numpy(np.ascontiguousarray(m))
    if m.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"IoU: masks are bool or uint8, got {m.dtype}")
    dev = m.device if m.is_cuda else _dev(device)
    return m.to(dev).contiguous()


def apply_gamma_curve(image):
    """utils2/image.py:14-26 in float32; the result is a device tensor of the input's shape"""
    x = _on_device(image, torch.float32)
    y = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().esr_gamma_curve(_lib.ptr(x), x.numel(), _lib.ptr(y), _lib.stream_ptr(x.device)), "esr_gamma_curve")
    return y


def sqerr_sum(a, b) -> torch.Tensor:
    """[1] float64 device tensor: the sum of ((double)a - (double)b)^2 over all elements, the same bits on every call"""
    a = _on_device(a, torch.float32)
    b = _on_device(b, torch.float32, a.device)
    if a.shape != b.shape:
        raise ValueError(f"sqerr_sum: shapes differ, {tuple(a.shape)} and {tuple(b.shape)}")
    dev = _same_device(a, b)
    with torch.cuda.device(dev):
        scratch = torch.empty(_BLOCKS + 1, dtype=torch.float64, device=dev)
        _lib.check(_lib.lib().esr_sqerr_sum(_lib.ptr(a), _lib.ptr(b), a.numel(), _lib.ptr(scratch),
                                            C.c_void_p(scratch.data_ptr() + 8 * _BLOCKS), _lib.stream_ptr(dev)), "esr_sqerr_sum")
    return scratch[_BLOCKS:]


def post_image(v: torch.Tensor, wbg=None, white_bg=1.0, lin=False, want_u8=False, target=None, target_gamma=None):
    """One result image of a view (app/fine/fine.py:572-587 and :611-617) in one launch.  v [..., C] or [...] float32 on
    the device, wbg (or None) the white-background weight per pixel.  Returns a dict: ``out`` (clamped to [0, 1], or to
    [0, inf) with ``lin``), ``gamma`` (with ``lin``), ``out_u8`` / ``gamma_u8`` (with ``want_u8``) and, against the given
    targets, ``sqerr`` / ``sqerr_gamma``: [1] float64 device tensors."""
    if not (isinstance(v, torch.Tensor) and v.is_cuda and v.dtype == torch.float32):
        raise ValueError("post_image: a float32 device tensor is expected")
    v = v.contiguous()
    dev = v.device
    channels = 1
    if wbg is not None:
        wbg = wbg.contiguous()
        if wbg.numel() == 0 or v.numel() % wbg.numel() or v.numel() // wbg.numel() not in (1, 3):
            raise ValueError(f"post_image: image {tuple(v.shape)} against background weights {tuple(wbg.shape)}")
        channels = v.numel() // wbg.numel()
    if target_gamma is not None and not lin:
        raise ValueError("post_image: target_gamma needs lin=True")
    job, res = _lib.EsrViewPost(), {}
    with torch.cuda.device(dev):
        res["out"] = torch.empty_like(v)
        if lin:
            res["gamma"] = torch.empty_like(v)
        if want_u8:
            res["out_u8"] = torch.empty(v.shape, dtype=torch.uint8, device=dev)
            if lin:
                res["gamma_u8"] = torch.empty(v.shape, dtype=torch.uint8, device=dev)
        tgt = {}
        for name, t in (("target_out", target), ("target_gamma", target_gamma)):
            if t is not None:
                tgt[name] = _on_device(t, torch.float32, dev)
                if tgt[name].numel() != v.numel():
                    raise ValueError(f"post_image: target {tuple(t.shape)} against image {tuple(v.shape)}")
        if tgt:
            scratch = torch.empty(2 * _BLOCKS + 2, dtype=torch.float64, device=dev)
            job.partials, job.sqerr = scratch.data_ptr(), scratch.data_ptr() + 16 * _BLOCKS
            if target is not None:
                res["sqerr"] = scratch[2 * _BLOCKS:2 * _BLOCKS + 1]
            if target_gamma is not None:
                res["sqerr_gamma"] = scratch[2 * _BLOCKS + 1:]
        job.v, job.wbg, job.wbg_scale, job.lin = v.data_ptr(), None if wbg is None else wbg.data_ptr(), float(white_bg), int(lin)
        job.n, job.channels = v.numel() // channels, channels
        job.out = res["out"].data_ptr()
        for f in ("gamma", "out_u8", "gamma_u8"):
            setattr(job, f, res[f].data_ptr() if f in res else None)
        for f, t in tgt.items():
            setattr(job, f, t.data_ptr())
        _lib.check(_lib.lib().esr_view_post(C.byref(job), _lib.stream_ptr(dev)), "esr_view_post")
    return res
