"""Re-lighting: which training rays see an edited emissive source, their edit labels, and the fine-tune on them -- the
``filter_edit_rays`` / ``finetune_radiance`` pair of the reference's PDRA trainer (app/fine/pdra.py:934-1109) over
libesr_hip.so's kernels (esr_nerf_amd/csrc/relight.hip).

``dilate_masks``        the view's emissive-source masks dilated by a ks x ks box (cv2.dilate's definition)
``label_edit_rays``     per ray: keep flag, ``em_modes``, ``em_colors``, ``em_intensities`` from its expected surface point
``attach_edit_labels``  the labels put on a ``RayGroupManager`` and its uncertain group filtered by the keep flags
``EditRaySelector``     the expected surface points of the uncertain group, marched ONCE per checkpoint; ``apply(view)``
                        does per view what ``filter_edit_rays`` does
``finetune_radiance``   the fine-tune loop on ``trainer.FinetuneStep`` and the package's Adam

The reference marches every uncertain ray again for every test view; ``eval_esp`` depends on the SDF grid, the mask cache,
``s_val`` and the rays -- nothing the fine-tune trains and nothing of the view -- and the checkpoint is reloaded before every
view, so the points are the same each time.  There is no CPU path: without the library the launchers raise.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional

import numpy as np
import torch

from . import _lib

LIGHT_MODES = {"off": 0, "on": 1, "i_change": 2, "c_change": 3, "ic_change": 4}      # utils2/utils.py:32-38
MAX_CONDITIONS = _lib.RELIGHT_MAX_COND
EDIT_KEYS = ("em_colors", "em_intensities")


def _device_f32(x, device=None) -> torch.Tensor:
    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(np.ascontiguousarray(x))
    dev = x.device if x.is_cuda else (torch.device(device) if device is not None
                                      else torch.device("cuda", torch.cuda.current_device()))
    return x.to(device=dev, dtype=torch.float32).contiguous()


def _host(x, dtype, shape) -> Optional[np.ndarray]:
    """A per-condition array as contiguous host memory (the conditions travel as kernel arguments)"""
    if x is None:
        return None
    x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return np.ascontiguousarray(x.astype(dtype, copy=False).reshape(shape))


def dilate_masks(em_masks, ks: int) -> torch.Tensor:
    """``cv2.dilate(em_masks, np.ones((ks, ks)), iterations=1)`` per mask (pdra.py:945-962): em_masks [n_cond, h, w] ->
    a new float32 device tensor of that shape.  The box is anchored at ``ks // 2``: the window is
    ``-(ks // 2) .. ks - 1 - ks // 2``, not symmetric for an even ``ks``."""
    m = _device_f32(em_masks)
    if m.dim() != 3:
        raise ValueError(f"dilate_masks: masks are [n_cond, h, w], got {tuple(m.shape)}")
    n_cond, h, w = (int(s) for s in m.shape)
    out = torch.empty_like(m)
    with torch.cuda.device(m.device):
        _lib.check(_lib.lib().esr_mask_dilate(_lib.ptr(m), n_cond, h, w, int(ks), _lib.ptr(out), _lib.stream_ptr(m.device)),
                   "esr_mask_dilate")
    return out


@torch.no_grad()
def edit_emission(emit, modes, intensities, colors) -> torch.Tensor:
    """The emission edit of the re-lighting fine-tune (esrnerf.py:427-441) on any emission values: ``emit`` float32 [n, 3],
    ``modes`` int64 [n] (``LIGHT_MODES``: 0 off, 1 unchanged, 2 scaled by ``intensities`` [n], 3 hue and saturation
    replaced by ``colors`` [n, 2] with the value kept, 4 both) -> a new float32 [n, 3] device tensor (``esr_emit_edit``, the
    kernel the light-transport engine runs on its own points)."""
    e = _device_f32(emit).clone()
    if e.dim() != 2 or e.shape[1] != 3:
        raise ValueError(f"edit_emission: emit is [n, 3], got {tuple(e.shape)}")
    n, dev = int(e.shape[0]), e.device
    if n >= 2 ** 31:
        raise ValueError(f"edit_emission: {n} values exceed the kernel's 31-bit count")
    if not isinstance(modes, torch.Tensor) or modes.dtype != torch.int64 or modes.shape != (n,) or modes.device != dev:
        raise ValueError("edit_emission: modes is an int64 [n] tensor on the device of emit")
    k, c = _device_f32(intensities, dev), _device_f32(colors, dev)
    if k.shape != (n,) or c.shape != (n, 2) or k.device != dev or c.device != dev:
        raise ValueError("edit_emission: intensities is [n] and colors [n, 2] (hue, saturation), on the device of emit")
    if n:
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().esr_emit_edit(_lib.ptr(e), _lib.ptr(modes.contiguous()), _lib.ptr(k), _lib.ptr(c), n,
                                                _lib.stream_ptr(dev)), "esr_emit_edit")
    return e


def label_edit_rays(esp, pose, focal, width, height, masks, em_modes, em_intensities=None, em_colors=None,
                    return_uv=False) -> Dict[str, torch.Tensor]:
    """pdra.py:988-1028 for all rays in one launch.  esp [n, 3] (``eval_esp``), pose [4, 4] camera-to-world (inverted on
    the host in float32, as the reference does), masks [n_cond, height, width] the DILATED masks, em_modes [n_cond],
    em_intensities [n_cond], em_colors [n_cond, >= 2] (the first two are used; None = zeros).  Returns device tensors
    ``keep`` [n] bool, ``em_modes`` [n] int64, ``em_colors`` [n, 2], ``em_intensities`` [n] (and ``uv`` [n, 2], the
    projected pixel coordinates, with ``return_uv``)."""
    esp = _device_f32(esp)
    dev = esp.device
    masks = _device_f32(masks, dev)
    if esp.dim() != 2 or esp.shape[1] != 3:
        raise ValueError(f"label_edit_rays: esp is [n, 3], got {tuple(esp.shape)}")
    n_cond = int(masks.shape[0]) if masks.dim() == 3 else -1
    if n_cond < 0 or tuple(masks.shape[1:]) != (int(height), int(width)) or masks.device != dev:
        raise ValueError(f"label_edit_rays: masks {tuple(masks.shape)} on {masks.device} for a {height} x {width} view on {dev}")
    pose = pose.detach() if isinstance(pose, torch.Tensor) else torch.from_numpy(np.asarray(pose))
    w2c = torch.inverse(pose.reshape(4, 4).to(device="cpu", dtype=torch.float32)).contiguous().numpy()
    modes = _host(em_modes, np.int64, (-1,))
    if modes.shape[0] != n_cond:
        raise ValueError(f"label_edit_rays: {modes.shape[0]} modes for {n_cond} masks")
    inten = _host(em_intensities, np.float32, (n_cond,))
    cols = None if em_colors is None else np.ascontiguousarray(_host(em_colors, np.float32, (n_cond, -1))[:, :2])
    n = int(esp.shape[0])
    hp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    with torch.cuda.device(dev):
        out = dict(keep=torch.empty(n, dtype=torch.uint8, device=dev), em_modes=torch.empty(n, dtype=torch.int64, device=dev),
                   em_colors=torch.empty(n, 2, dtype=torch.float32, device=dev),
                   em_intensities=torch.empty(n, dtype=torch.float32, device=dev))
        if return_uv:
            out["uv"] = torch.empty(n, 2, dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().esr_edit_label(_lib.ptr(esp), n, hp(w2c), float(focal), int(width), int(height), _lib.ptr(masks),
                                             n_cond, hp(modes), hp(inten), hp(cols), _lib.ptr(out["keep"]),
                                             _lib.ptr(out["em_modes"]), _lib.ptr(out["em_colors"]),
                                             _lib.ptr(out["em_intensities"]), _lib.ptr(out.get("uv")), _lib.stream_ptr(dev)),
                   "esr_edit_label")
    out["keep"] = out["keep"].view(torch.bool)
    return out


def attach_edit_labels(sampler, keep, em_modes, em_colors, em_intensities):
    """pdra.py:1030-1044 on this package's ``RayGroupManager``.  The labels are aligned with the uncertain group's
    current order.  The reference stores per-group arrays in current order; ours keeps every array at its original rows
    (data.py), so the labels go into NEW full-length arrays indexed by original row: the uncertain rows get the labels,
    every other row (the certain group) mode 0, colour 0, intensity 0.  ``sampler.data["em_modes"]`` may be the dataset's
    own array and is replaced, not written.  Then the group is filtered by ``keep`` and the two edit keys join
    ``sampler.keys``.  Works on any device (no kernel)."""
    rows = sampler.uncert_data_idxs
    if not (len(keep) == len(em_modes) == len(em_colors) == len(em_intensities) == len(rows)):
        raise ValueError("attach_edit_labels: the labels are not aligned with the uncertain group")
    sampler.set_rows("em_modes", rows, em_modes.to(torch.int64), fill=0)
    sampler.set_rows("em_colors", rows, em_colors.to(torch.float32), fill=0)
    sampler.set_rows("em_intensities", rows, em_intensities.to(torch.float32), fill=0)
    sampler.keys.extend(k for k in EDIT_KEYS if k not in sampler.keys)
    sampler.filter(keep.to(torch.bool))
    return sampler


class EditRaySelector:
    """``filter_edit_rays`` with the march taken out of the per-view loop.

    Construction computes ``renderer.eval_esp`` of the sampler's uncertain group once, in chunks of ``batch_size`` written
    straight into one [n, 3] buffer, with the renderer in ``eval()`` for the duration (its mode is restored).  The points
    are kept beside the ORIGINAL row of each ray (``rows``), so they do not depend on what the sampler's index vectors look
    like later.  ``apply(test_data)`` first puts the sampler back into the state it was built on (the reference builds a
    new sampler from the checkpoint for every view), then dilates the view's masks, labels the rays, attaches the labels
    and filters the uncertain group: two launches and the index bookkeeping per view.

    test_data: ``poses`` [4, 4], ``em_masks`` (n_cond * h * w values), ``em_modes`` [n_cond], ``em_intensities`` [n_cond],
    ``em_colors`` [n_cond, 3]."""

    def __init__(self, renderer, sampler, focal, image_size, mask_dilation_ks, batch_size):
        self.renderer, self.sampler = renderer, sampler
        self.focal = float(focal)
        self.width, self.height = int(image_size[0]), int(image_size[1])     # the datasets' (w, h)
        self.ks, self.batch_size = int(mask_dilation_ks), int(batch_size)
        if self.batch_size < 1:
            raise ValueError("EditRaySelector: batch_size must be positive")
        self._base = dict(uncert=sampler.uncert_data_idxs.clone(), cert=sampler.cert_data_idxs.clone(),
                          st=(sampler.uncert_batch_st, sampler.cert_batch_st), keys=list(sampler.keys),
                          data={k: sampler.data.get(k) for k in ("em_modes",) + EDIT_KEYS})
        self.rows = self._base["uncert"]
        self.esp = self._march()
        self.labels: Optional[Dict[str, torch.Tensor]] = None            # of the last view applied

    @torch.no_grad()
    def _march(self) -> torch.Tensor:
        s, dev = self.sampler, torch.device(self.sampler.device)
        n = len(self.rows)
        esp = torch.empty(n, 3, dtype=torch.float32, device=dev)
        was_training = self.renderer.training
        finetune = was_training and getattr(self.renderer, "forward", None) == getattr(self.renderer, "forward_finetune", None)
        self.renderer.eval()
        try:
            for a in range(0, n, self.batch_size):
                rows = self.rows[a:a + self.batch_size]
                chunk = {k: s.data[k][rows].to(dev, non_blocking=True) for k in ("rays_o", "rays_d", "viewdirs")}
                esp[a:a + len(rows)].copy_(self.renderer.eval_esp(**chunk))
        finally:
            if was_training:
                self.renderer.train(True, finetune=True) if finetune else self.renderer.train(True)
        return esp

    def reset(self):
        """The sampler as it was when the selector was built"""
        s, b = self.sampler, self._base
        s.uncert_data_idxs, s.cert_data_idxs = b["uncert"].clone(), b["cert"].clone()
        s.uncert_batch_st, s.cert_batch_st = b["st"]
        s.keys[:] = b["keys"]
        for k, v in b["data"].items():
            if v is None:
                s.data.pop(k, None)
            else:
                s.data[k] = v
        return s

    @torch.no_grad()
    def apply(self, test_data):
        s = self.reset()
        dev = self.esp.device
        masks = _device_f32(test_data["em_masks"], dev).reshape(-1, self.height, self.width)
        masks = dilate_masks(masks, self.ks)
        lab = label_edit_rays(self.esp, test_data["poses"], self.focal, self.width, self.height, masks, test_data["em_modes"],
                              test_data.get("em_intensities"), test_data.get("em_colors"))
        self.labels = lab
        return attach_edit_labels(s, lab["keep"], lab["em_modes"], lab["em_colors"], lab["em_intensities"])


def finetune_radiance(renderer, selector_or_sampler, test_data, n_iters, lrs, weight_lts, state=None) -> List[float]:
    """pdra.py:1047-1109: fine-tune ``emo_color`` / ``emo_rgbnet`` towards one edited view and return the per-step losses
    (``weight_lts * mse(lin/pbr/emo, lin/pbr/emo_hat)``).  ``state`` (a ``state_dict``) is restored first when given -- the
    reference reloads the checkpoint before every view.  An ``EditRaySelector`` is applied to ``test_data``; a sampler is
    taken as already labelled.  Only the two emission parameters get a learning rate (``lrs``: emo_color, emo_rgbnet);
    the renderer is put in fine-tune mode before the loop and in ``eval()`` after it.  One read-back, at the end."""
    from .optimizer import create_optimizer_or_freeze_model
    from .trainer import FinetuneStep
    if state is not None:
        renderer.load_state_dict(state, strict=False)
    sampler = selector_or_sampler.apply(test_data) if isinstance(selector_or_sampler, EditRaySelector) else selector_or_sampler
    for p in renderer.parameters():
        p.requires_grad_(False)
    for p in list(renderer.emo_color.parameters()) + list(renderer.emo_rgbnet.parameters()):
        p.requires_grad_(True)
    optimizer = create_optimizer_or_freeze_model(renderer, **{k: lrs[k] for k in ("emo_color", "emo_rgbnet") if k in lrs})
    renderer.train(True, finetune=True)
    params = dict(renderer.named_parameters())
    losses = []
    try:
        step = FinetuneStep(renderer, weight=float(weight_lts))
        for _ in range(int(n_iters)):
            batch = sampler.sample()
            optimizer.zero_grad(set_to_none=True)
            loss, grads = step.forward_loss_backward(batch, renderer.s_val)
            for name, g in grads.items():
                params[name].grad = g
            optimizer.step()
            losses.append(loss.clone())
    finally:
        renderer.eval()
    return torch.cat(losses).tolist() if losses else []
