"""LPIPS with the AlexNet backbone (version 0.1, ``normalize=True``, eval mode) on libesr_hip.so's kernels
(esr_nerf_amd/csrc/lpips.hip): the reference's ``utils2.metric.rgb_lpips`` (utils2/metric.py:15-28) without the ``lpips``
package, torchvision or a vendor convolution library.

Per image [H, W, 3] in [0, 1]: ``s = ((2 x - 1) - shift) / scale``, five taps of AlexNet's feature stack (each behind its
ReLU), and per tap the mean over pixels of ``sum_c w_c (n0_c - n1_c)^2`` with ``n = f / (|f| + 1e-10)``; the distance is the
sum over the taps.  Activations are channels-last, so an image needs no permutation.

``LpipsAlex(weights, device)``     the model: packed convolution weights and a grow-only workspace on ``device``
``LpipsAlex.random(seed, device)`` a Kaiming-scaled model of the exact shapes (tests, tools/lpips_time.py)
``LpipsAlex.from_state_dict``      trained weights, the user's to supply: an ``lpips.LPIPS(net="alex").state_dict()``, or the
                                   package's ``alex.pth`` together with torchvision's AlexNet state dict
``LpipsAlex.from_file``            the same from files (``torch.load(..., weights_only=True)``)

No trained weights travel with this package, VGG is not provided, and there is no CPU path: without the library every
call raises.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List

import numpy as np
import torch

from . import _lib

# (Cin, Cout, kernel, stride, pad, pooled): the five taps; `pooled`: a 3x3 stride-2 max pool in front of the convolution
LAYERS = ((3, 64, 11, 4, 2, False), (64, 192, 5, 1, 2, True), (192, 384, 3, 1, 1, True), (384, 256, 3, 1, 1, False),
          (256, 256, 3, 1, 1, False))
SHIFT = (-0.030, -0.088, -0.188)            # the scaling layer of lpips 0.1
SCALE = (0.458, 0.448, 0.450)
FEATURE_INDEX = (0, 3, 6, 8, 10)            # the convolutions' positions in torchvision's alexnet().features
MIN_SIZE = 31                               # the smallest image side for which every tap is non-empty
POOL_K, POOL_STRIDE = 3, 2
_BLOCKS = _lib.METRICS_BLOCKS


def conv_out(size: int, k: int, stride: int, pad: int) -> int:
    return (size + 2 * pad - k) // stride + 1


def tap_sizes(H: int, W: int) -> List[tuple]:
    """[(Ho, Wo)] of the five taps of an H x W image"""
    out = []
    for _, _, k, s, p, pooled in LAYERS:
        if pooled:
            H, W = conv_out(H, POOL_K, POOL_STRIDE, 0), conv_out(W, POOL_K, POOL_STRIDE, 0)
        H, W = conv_out(H, k, s, p), conv_out(W, k, s, p)
        out.append((H, W))
    return out


def _shape_check(name, t, shape):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"LpipsAlex: '{name}' is not a tensor")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"LpipsAlex: '{name}' has shape {tuple(t.shape)}, expected {tuple(shape)}")
    return t.detach().to(device="cpu", dtype=torch.float32).contiguous()


def _take(sd, key, shape, what):
    if key not in sd:
        raise KeyError(f"LpipsAlex: the {what} has no key '{key}'")
    return _shape_check(key, sd[key], shape)


def check_weights(weights) -> Dict[str, object]:
    """``weights`` as float32 CPU tensors, every shape checked against ``LAYERS``; a missing or mis-sized part is named"""
    missing = {"conv_w", "conv_b", "lin", "shift", "scale"} - set(weights)
    if missing:
        raise KeyError(f"LpipsAlex: weights lack {sorted(missing)}")
    for part in ("conv_w", "conv_b", "lin"):
        if len(weights[part]) != len(LAYERS):
            raise ValueError(f"LpipsAlex: '{part}' has {len(weights[part])} entries, expected {len(LAYERS)}")
    w = {"conv_w": [], "conv_b": [], "lin": []}
    for l, (cin, cout, k, _, _, _) in enumerate(LAYERS):
        w["conv_w"].append(_shape_check(f"conv_w[{l}]", weights["conv_w"][l], (cout, cin, k, k)))
        w["conv_b"].append(_shape_check(f"conv_b[{l}]", weights["conv_b"][l], (cout,)))
        w["lin"].append(_shape_check(f"lin[{l}]", weights["lin"][l], (cout,)))
    w["shift"] = _shape_check("shift", weights["shift"], (3,))
    w["scale"] = _shape_check("scale", weights["scale"], (3,))
    if not bool((w["scale"] != 0).all()):
        raise ValueError("LpipsAlex: 'scale' holds a zero")
    return w


def random_weights(seed: int = 0) -> Dict[str, object]:
    """Seeded stand-in weights: convolutions N(0, 2 / fan_in), biases U(-0.1, 0.1), ``lin`` U[0, 0.1), the published shift
    and scale"""
    g = torch.Generator().manual_seed(int(seed))
    w = {"conv_w": [], "conv_b": [], "lin": [], "shift": torch.tensor(SHIFT), "scale": torch.tensor(SCALE)}
    for cin, cout, k, _, _, _ in LAYERS:
        w["conv_w"].append(torch.randn(cout, cin, k, k, generator=g) * float(np.sqrt(2.0 / (cin * k * k))))
        w["conv_b"].append(torch.rand(cout, generator=g) * 0.2 - 0.1)
        w["lin"].append(torch.rand(cout, generator=g) * 0.1)
    return w


def weights_from_state_dict(sd, backbone_sd=None) -> Dict[str, object]:
    """The weights of ``LpipsAlex.from_state_dict``'s two forms as a ``check_weights`` dict (host only)"""
    w = {"conv_w": [], "conv_b": [], "lin": []}
    for l, (cin, cout, k, _, _, _) in enumerate(LAYERS):
        if backbone_sd is None:
            stem, src, what = f"net.slice{l + 1}.{FEATURE_INDEX[l]}", sd, "LPIPS state dict"
        else:
            stem, src, what = f"features.{FEATURE_INDEX[l]}", backbone_sd, "AlexNet state dict"
        w["conv_w"].append(_take(src, f"{stem}.weight", (cout, cin, k, k), what))
        w["conv_b"].append(_take(src, f"{stem}.bias", (cout,), what))
        w["lin"].append(_take(sd, f"lin{l}.model.1.weight", (1, cout, 1, 1), "LPIPS state dict").reshape(cout))
    for name, const in (("shift", SHIFT), ("scale", SCALE)):
        key = f"scaling_layer.{name}"
        if backbone_sd is not None and key not in sd:
            w[name] = torch.tensor(const)
        else:
            w[name] = _take(sd, key, (1, 3, 1, 1), "LPIPS state dict").reshape(3)
    return check_weights(w)


class LpipsAlex:
    """``weights``: ``conv_w`` [5] ([Cout, Cin, k, k]), ``conv_b`` [5] ([Cout]), ``lin`` [5] ([Cout]), ``shift`` [3], ``scale``
    [3], float32 tensors of the shapes of ``LAYERS``.  They are kept (on the host, ``self.weights``) as given."""

    def __init__(self, weights: Dict[str, object], device=None):
        w = check_weights(weights)
        self.weights = w
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        L = _lib.lib()
        with torch.cuda.device(self.device):
            st = _lib.stream_ptr(self.device)
            self._packed, self._bias, self._lin = [], [], []
            for l, (cin, cout, k, _, _, _) in enumerate(LAYERS):
                src = w["conv_w"][l].to(self.device)
                dst = torch.empty(L.esr_conv_packed_floats(cout, cin, k, k), dtype=torch.float32, device=self.device)
                _lib.check(L.esr_conv_pack(_lib.ptr(src), cout, cin, k, k, _lib.ptr(dst), st), "esr_conv_pack")
                self._packed.append(dst)
                self._bias.append(w["conv_b"][l].to(self.device))
                self._lin.append(w["lin"][l].to(self.device))
            self._affine = torch.cat([w["shift"], w["scale"]]).to(self.device)
            self._scratch = torch.empty(_BLOCKS, dtype=torch.float64, device=self.device)
            torch.cuda.current_stream(self.device).synchronize()          # the host copies `src` may go
        self._work: Dict[str, torch.Tensor] = {}

    # ---- construction ------------------------------------------------------------------------------------------------
    @classmethod
    def random(cls, seed: int = 0, device=None) -> "LpipsAlex":
        """A model on ``random_weights(seed)``"""
        return cls(random_weights(seed), device)

    @classmethod
    def from_state_dict(cls, sd, backbone_sd=None, device=None) -> "LpipsAlex":
        """``sd`` alone: an ``lpips.LPIPS(net="alex").state_dict()`` (``net.slice{i}.{n}.weight|bias``,
        ``lin{i}.model.1.weight``, ``scaling_layer.shift|scale``; the duplicate ``lins.*`` keys are ignored).  With
        ``backbone_sd``: ``sd`` is the package's ``alex.pth`` (``lin{i}.model.1.weight`` only) and ``backbone_sd``
        torchvision's AlexNet (``features.{n}.weight|bias``); the scaling layer is then the published constant unless ``sd``
        carries one.  Every shape is checked, a missing or mis-sized key is named; nothing is guessed."""
        return cls(weights_from_state_dict(sd, backbone_sd), device)

    @classmethod
    def from_file(cls, path, backbone_path=None, device=None) -> "LpipsAlex":
        sd = torch.load(path, map_location="cpu", weights_only=True)
        bb = torch.load(backbone_path, map_location="cpu", weights_only=True) if backbone_path is not None else None
        return cls.from_state_dict(sd, bb, device)

    # ---- evaluation --------------------------------------------------------------------------------------------------
    def _buffer(self, name: str, numel: int) -> torch.Tensor:
        """``numel`` floats of the grow-only workspace slot ``name``"""
        buf = self._work.get(name)
        if buf is None or buf.numel() < numel:
            buf = self._work[name] = torch.empty(numel, dtype=torch.float32, device=self.device)
        return buf[:numel]

    @torch.no_grad()
    def features(self, images) -> List[torch.Tensor]:
        """images [N, H, W, 3] (or [H, W, 3]) float32 in [0, 1] -> the five taps, [N, Ho, Wo, C] device tensors"""
        x = images if isinstance(images, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(images))
        if x.dim() == 3:
            x = x.unsqueeze(0)
        if x.dim() != 4 or x.shape[-1] != 3:
            raise ValueError(f"LpipsAlex: expected images [N, H, W, 3], got {tuple(x.shape)}")
        N, H, W = int(x.shape[0]), int(x.shape[1]), int(x.shape[2])
        if N < 1 or min(H, W) < MIN_SIZE:
            raise ValueError(f"LpipsAlex: {N} images of {H} x {W}; the smallest image with five non-empty taps is "
                             f"{MIN_SIZE} x {MIN_SIZE}")
        x = x.to(device=self.device, dtype=torch.float32).contiguous()
        L, taps = _lib.lib(), []
        with torch.cuda.device(self.device):
            st = _lib.stream_ptr(self.device)
            for l, (cin, cout, k, stride, pad, pooled) in enumerate(LAYERS):
                if pooled:
                    Hp, Wp = conv_out(H, POOL_K, POOL_STRIDE, 0), conv_out(W, POOL_K, POOL_STRIDE, 0)
                    pool = self._buffer(f"pool{l}", N * Hp * Wp * cin)
                    _lib.check(L.esr_maxpool_nhwc(_lib.ptr(x), N, H, W, cin, POOL_K, POOL_STRIDE, _lib.ptr(pool), st),
                               "esr_maxpool_nhwc")
                    x, H, W = pool, Hp, Wp
                Ho, Wo = conv_out(H, k, stride, pad), conv_out(W, k, stride, pad)
                y = torch.empty(N, Ho, Wo, cout, dtype=torch.float32, device=self.device)
                _lib.check(L.esr_conv_relu(_lib.ptr(x), N, H, W, cin, _lib.ptr(self._packed[l]), _lib.ptr(self._bias[l]), cout,
                                           k, k, stride, pad, _lib.ptr(self._affine if l == 0 else None), _lib.ptr(y), st),
                           "esr_conv_relu")
                taps.append(y)
                x, H, W = y, Ho, Wo
        return taps

    @torch.no_grad()
    def layers(self, feats, i: int = 0, j: int = 1) -> torch.Tensor:
        """[5] float64 device tensor: the per-tap terms d_l between images ``i`` and ``j`` of ``features``' batch"""
        if len(feats) != len(LAYERS):
            raise ValueError(f"LpipsAlex: {len(feats)} taps, expected {len(LAYERS)}")
        L = _lib.lib()
        with torch.cuda.device(self.device):
            st = _lib.stream_ptr(self.device)
            out = torch.empty(len(LAYERS), dtype=torch.float64, device=self.device)
            for l, f in enumerate(feats):
                if f.dim() != 4 or f.shape[-1] != LAYERS[l][1] or f.dtype != torch.float32 or not f.is_contiguous():
                    raise ValueError(f"LpipsAlex: tap {l} is not a contiguous float32 [N, H, W, {LAYERS[l][1]}] tensor")
                npix, Cl = int(f.shape[1]) * int(f.shape[2]), int(f.shape[3])
                _lib.check(L.esr_lpips_layer(_lib.ptr(f[i]), _lib.ptr(f[j]), npix, Cl, _lib.ptr(self._lin[l]),
                                             _lib.ptr(self._scratch), C.c_void_p(out.data_ptr() + 8 * l), st),
                           "esr_lpips_layer")
        return out

    @torch.no_grad()
    def distance(self, feats, i: int = 0, j: int = 1) -> torch.Tensor:
        """float64 device scalar: the LPIPS distance between images ``i`` and ``j``, the taps added in their order"""
        d = self.layers(feats, i, j)
        return (((d[0] + d[1]) + d[2]) + d[3]) + d[4]

    def __call__(self, img0, img1) -> float:
        """The distance of two [H, W, 3] images in [0, 1] (numpy, CPU or device tensors); one read-back"""
        a, b = (t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t)) for t in (img0, img1))
        if a.dim() != 3 or tuple(a.shape) != tuple(b.shape):
            raise ValueError(f"LpipsAlex: expected two [H, W, 3] images, got {tuple(a.shape)} and {tuple(b.shape)}")
        pair = torch.stack([a.to(device=self.device, dtype=torch.float32), b.to(device=self.device, dtype=torch.float32)])
        return float(self.distance(self.features(pair), 0, 1))
