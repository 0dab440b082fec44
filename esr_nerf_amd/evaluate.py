"""Test-view evaluation on the device: the image level of the reference trainers' ``evaluate()``
(app/fine/fine.py:500-623, app/fine/pdra.py:600-762; the same loop in coarse.py / lts.py) without file writing and
logging.  LPIPS is opt-in: ``view_metrics`` / ``evaluate_views`` add ``*/LPIPS_ALEX`` when they are handed an
``lpips.LpipsAlex`` (the trained weights are the user's to supply).

``render_camera_view``  one view of a camera set (camera.py): its rays made on the device, then ``render_view``
``render_view``       the chunk loop (fine.py:553-570): every chunk's outputs go straight into one set of [H*W, C] buffers
``postprocess_view``  background, clamps, the ``lin/*_gamma`` twins (fine.py:572-587), optionally the uint8 images and the
                      squared-error sums against the targets in the same launches
``view_metrics``      the metric lines (fine.py:596-609, pdra.py:710-739) under the reference's names
``evaluate_views``    the loop over views: per-view lists, their means, PDRA's pooled ``etc/IoU``

Everything stays on the device; a view costs one read-back of its squared-error sums, one per SSIM and one for the IoU
counts (and the uint8 images when they are asked for); with LPIPS, one more for its two distances.
"""
from __future__ import annotations

from typing import Dict, Iterable, List, Optional

import numpy as np
import torch

from . import metrics as M

LIGHT_MODES = {"off": 0, "on": 1}          # utils2/utils.py:32-35, the two modes evaluate() scores


@torch.no_grad()
def render_view(renderer, rays_o, rays_d, viewdirs, em_mode, pos_rt, height, width, batch_size, **extra):
    """Render ``height * width`` rays in chunks of ``batch_size`` through ``renderer(**chunk)`` (a model in eval mode:
    DVGO, VoxurfC, VoxurfF, ESRNeRF -- ``extra`` carries ``render_pbr`` / ``chunk_sz`` for the last).  Returns the result
    dict reshaped as the reference's ``reshape(height, width, -1).squeeze(-1)``, on the device."""
    n = int(height) * int(width)
    if rays_o.shape[0] != n:
        raise ValueError(f"render_view: {rays_o.shape[0]} rays for a {height} x {width} view")
    if batch_size < 1:
        raise ValueError("render_view: batch_size must be positive")
    bufs: Dict[str, torch.Tensor] = {}
    for s in range(0, n, int(batch_size)):
        e = min(n, s + int(batch_size))
        out = renderer(rays_o=rays_o[s:e], rays_d=rays_d[s:e], viewdirs=viewdirs[s:e], em_modes=em_mode, pos_rt=pos_rt,
                       **extra)
        if not bufs:
            bufs = {k: torch.empty((n, *v.shape[1:]), dtype=v.dtype, device=v.device) for k, v in out.items()}
        if set(out) != set(bufs):
            raise RuntimeError(f"render_view: the renderer's result keys changed between chunks: {sorted(set(out) ^ set(bufs))}")
        for k, v in out.items():
            bufs[k][s:e].copy_(v)
        del out                                     # one chunk's outputs at a time beside the buffers
    return {k: v.reshape(height, width, -1).squeeze(-1) for k, v in bufs.items()}


@torch.no_grad()
def render_camera_view(renderer, cams, view, em_mode, pos_rt, batch_size, **extra):
    """``render_view`` of view ``view`` of the camera set ``cams`` (camera.Cameras): the view's rays come from one launch of
    the ray kernel instead of a loader's arrays (the test phases' ``pose2ray``, data/esrnerf/esrnerf.py:237-238)."""
    from .camera import camera_rays
    rays_o, rays_d, viewdirs = camera_rays(cams, int(view))
    return render_view(renderer, rays_o, rays_d, viewdirs, em_mode, pos_rt, cams.height, cams.width, batch_size, **extra)


class ViewImages(dict):
    """The post-processed result images of a view, plus what the same launches produced beside them: ``sqerr`` (key ->
    [1] float64 device tensor, the squared-error sum against the view's target) and ``u8`` (key -> uint8 image)."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.sqerr: Dict[str, torch.Tensor] = {}
        self.u8: Dict[str, torch.Tensor] = {}


@torch.no_grad()
def postprocess_view(results, white_bg, rgbs=None, hdrs=None, want_u8=False) -> ViewImages:
    """fine.py:572-587 over every key, in the reference's order: ``v + etc/white_bg * white_bg`` clamped to [0, 1]; the
    ``lin/`` keys clamped to [0, inf) with a ``*_gamma`` twin; ``etc/white_bg`` only clamped.  With ``rgbs`` / ``hdrs``
    ([H, W, 3]) the launches of ``srgb/rgb`` and ``lin/rgb`` also sum the squared errors ``view_metrics`` needs."""
    out = ViewImages()
    wbg = results["etc/white_bg"]
    for k, v in results.items():
        if k == "etc/white_bg":
            r = M.post_image(v, want_u8=want_u8)
            wbg = r["out"]                         # the keys behind it read the clamped weights, as in the reference
        else:
            lin = k.startswith("lin/")
            tgt = dict(target=rgbs) if k == "srgb/rgb" else dict(target=hdrs, target_gamma=rgbs) if k == "lin/rgb" else {}
            r = M.post_image(v, wbg, float(white_bg), lin=lin, want_u8=want_u8, **tgt)
        out[k] = r["out"]
        if "gamma" in r:
            out[f"{k}_gamma"] = r["gamma"]
        for src, name in (("out", k), ("gamma", f"{k}_gamma")):
            if f"{src}_u8" in r:
                out.u8[name] = r[f"{src}_u8"]
        if "sqerr" in r:
            out.sqerr[k] = r["sqerr"]
        if "sqerr_gamma" in r:
            out.sqerr[f"{k}_gamma"] = r["sqerr_gamma"]
    return out


@torch.no_grad()
def view_metrics(results, rgbs, hdrs=None, em_mode=None, masks=None, areas=None, lpips=None) -> Dict[str, Optional[float]]:
    """The metric lines of fine.py:596-609 / pdra.py:710-739, from post-processed ``results``: ``lin/MSE``,
    ``lin/PSNR``, ``lin/SSIM``; ``srgb/*`` when the view has an ``srgb/rgb`` image; ``lin/MSE_EXR_off|on`` with ``hdrs``
    and ``em_mode`` (None for the mode the view was not rendered in); ``etc/IoU_I``, ``etc/IoU_U`` with ``masks`` and
    ``areas``.  MSE is the float64 sum of squared differences over the element count.  With ``lpips`` (an
    ``lpips.LpipsAlex``): ``lin/LPIPS_ALEX`` and, when the view has an ``srgb/rgb`` image, ``srgb/LPIPS_ALEX``
    (pdra.py:615-742) -- the target and the images go through the network as one batch, the target's features are computed
    once.  Without it the returned keys and values are what they were."""
    sqerr = getattr(results, "sqerr", {})
    pairs = {"lin/MSE": ("lin/rgb_gamma", rgbs)}
    if "srgb/rgb" in results:
        pairs["srgb/MSE"] = ("srgb/rgb", rgbs)
    if hdrs is not None:
        if em_mode is None:
            raise ValueError("view_metrics: hdrs need the view's em_mode")
        em_mode = int(em_mode.reshape(-1)[0]) if torch.is_tensor(em_mode) else int(em_mode)
        pairs["lin/MSE_EXR"] = ("lin/rgb", hdrs)
    sums = [sqerr[key] if key in sqerr else M.sqerr_sum(results[key], tgt.reshape(results[key].shape))
            for key, tgt in pairs.values()]
    host = torch.cat(sums).tolist()                                    # the view's one read-back of its error sums
    mse = {name: s / results[key].numel() for (name, (key, _)), s in zip(pairs.items(), host)}
    m: Dict[str, Optional[float]] = {}
    if hdrs is not None:
        for mode, code in LIGHT_MODES.items():
            m[f"lin/MSE_EXR_{mode}"] = mse["lin/MSE_EXR"] if code == em_mode else None
    for space, key in (("srgb", "srgb/rgb"), ("lin", "lin/rgb_gamma")):
        if f"{space}/MSE" in mse:
            m[f"{space}/MSE"] = mse[f"{space}/MSE"]
            m[f"{space}/PSNR"] = float(M.loss2psnr(mse[f"{space}/MSE"]))
            m[f"{space}/SSIM"] = M.rgb_ssim(results[key], rgbs.reshape(results[key].shape), 1)
    if masks is not None and areas is not None:
        _, m["etc/IoU_I"], m["etc/IoU_U"] = M.IoU(masks, areas.reshape(masks.shape))
    if lpips is not None:
        spaces = [(space, key) for space, key in (("lin", "lin/rgb_gamma"), ("srgb", "srgb/rgb")) if key in results]
        shape = results["lin/rgb_gamma"].shape
        batch = torch.stack([rgbs.reshape(shape).to(torch.float32)] + [results[key].reshape(shape) for _, key in spaces])
        feats = lpips.features(batch)
        host = torch.stack([lpips.distance(feats, 0, 1 + i) for i in range(len(spaces))]).tolist()
        for (space, _), d in zip(spaces, host):
            m[f"{space}/LPIPS_ALEX"] = d
    return m


def _to(x, device, dtype=None):
    x = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    return x.to(device=device, dtype=dtype or x.dtype)


@torch.no_grad()
def evaluate_views(renderer, views: Iterable[dict], batch_size, white_bg, height, width, k_val=None, return_images=False,
                   device=None, lpips=None, **extra):
    """The view loop of ``evaluate()``.  A view is a dict: ``rays_o``, ``rays_d``, ``viewdirs`` [H*W, 3], ``em_mode``
    (scalar), ``pos_rt`` [3, 3], ``rgbs`` [H*W, 3] and optionally ``hdrs`` [H*W, 3] and ``areas`` [H*W] (bool; with
    ``k_val``: PDRA's emission mask ``any(lin/emit > k_val)`` is applied to ``lin/emit`` and scored against it).
    Returns ``{"metrics": name -> per-view list, "mean": name -> mean over the views that have it, "scene": {"etc/IoU"}
    when masks were scored, "images": key -> list of uint8 [H, W(, 3)] host arrays with return_images}``.  ``lpips``: an
    ``lpips.LpipsAlex`` adds the ``*/LPIPS_ALEX`` lines of ``view_metrics``."""
    device = torch.device(device) if device is not None else next(renderer.parameters()).device
    metrics: Dict[str, List[Optional[float]]] = {}
    images: Dict[str, list] = {}
    n_views = 0
    for view in views:
        rays = {k: _to(view[k], device, torch.float32) for k in ("rays_o", "rays_d", "viewdirs")}
        results = render_view(renderer, rays["rays_o"], rays["rays_d"], rays["viewdirs"], view["em_mode"],
                              _to(view["pos_rt"], device, torch.float32), height, width, batch_size, **extra)
        masks = None
        if k_val is not None and "lin/emit" in results:                # pdra.py:686-688
            masks = torch.any(results["lin/emit"] > k_val, dim=-1)
            results["lin/emit"] = results["lin/emit"] * masks.unsqueeze(-1)
        rgbs = _to(view["rgbs"], device, torch.float32).reshape(height, width, 3)
        hdrs = _to(view["hdrs"], device, torch.float32).reshape(height, width, 3) if view.get("hdrs") is not None else None
        areas = _to(view["areas"], device).reshape(height, width) if view.get("areas") is not None else None
        post = postprocess_view(results, white_bg, rgbs=rgbs, hdrs=hdrs, want_u8=return_images)
        m = view_metrics(post, rgbs, hdrs=hdrs, em_mode=view["em_mode"], masks=masks if areas is not None else None,
                         areas=areas, lpips=lpips)
        for k in set(metrics) | set(m):
            metrics.setdefault(k, [None] * n_views).append(m.get(k))
        n_views += 1
        if return_images:
            images.setdefault("target", []).append((rgbs.cpu().numpy() * 255).astype("uint8"))
            for k, v in post.u8.items():
                images.setdefault(k, []).append(v.cpu().numpy())
    out = {"metrics": metrics, "scene": {}}
    if "etc/IoU_I" in metrics:                                         # pdra.py:758-762
        inter, union = (sum(v for v in metrics.pop(k) if v is not None) for k in ("etc/IoU_I", "etc/IoU_U"))
        out["scene"]["etc/IoU"] = inter / max(1, union)
    out["mean"] = {k: (float(np.mean([x for x in v if x is not None])) if any(x is not None for x in v) else None)
                   for k, v in metrics.items()}
    if return_images:
        out["images"] = images
    return out
