"""CPU side of the LPIPS metric (esr_nerf_amd/lpips.py, csrc/lpips.hip): the float64 restatement tests/lpips_ref64.py against
independent forms of its own parts, its binary32 emulation inside every bound the GPU test uses, ten mutants of the
definition rejected, the state-dict loader's two forms and its refusals, and the C ABI's declarations and argument codes."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lpips_ref64 as R
from esr_nerf_amd import _lib, lpips, metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("esr_conv_packed_floats", "esr_conv_pack", "esr_conv_relu", "esr_maxpool_nhwc", "esr_lpips_layer")
SMALL = [c for c in R.CONV_CASES if c[0] != "tiles-2x200x203"]


# ---- the restatement against independent forms ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SMALL, ids=[c[0] for c in SMALL])
def test_restated_convolution_equals_unfold_and_matmul(case):
    _, N, H, W, Cin, Cout, k, stride, pad, _ = case
    x, w, b, aff = R.case_tensors(case)
    y, absref = R.conv_relu64(x, w, b, stride, pad, aff)
    A, (n, Ho, Wo) = R.im2col(R.affine64(x, aff).numpy(), k, stride, pad)
    B = R.weight_matrix(w.double().numpy())
    z = A @ B + b.double().numpy()
    assert (n, Ho, Wo) == tuple(y.shape[:3]) and Ho == R.conv_out(H, k, stride, pad)
    assert np.allclose(y.numpy().reshape(-1, Cout), np.maximum(z, 0), rtol=1e-12, atol=1e-13)
    assert np.allclose(absref.numpy().reshape(-1, Cout), np.abs(A) @ np.abs(B) + np.abs(b.double().numpy()), rtol=1e-12, atol=0)
    # torch's own unfold agrees on the patches (its column order is (c, ky, kx))
    u = F.unfold(R.affine64(x, aff).permute(0, 3, 1, 2), k, padding=pad, stride=stride)
    u = u.reshape(N, Cin, k * k, -1).permute(0, 3, 2, 1).reshape(-1, k * k * Cin)
    assert np.array_equal(u.numpy(), A)


@pytest.mark.parametrize("shape", R.POOL_CASES + ((1, 8, 11, 3),))
def test_restated_pool_equals_a_loop(shape):
    N, H, W, C = shape
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(H)) - 0.5
    y = R.maxpool(x)
    Ho, Wo = (H - 3) // 2 + 1, (W - 3) // 2 + 1
    assert tuple(y.shape) == (N, Ho, Wo, C)
    for n in range(N):
        for i in range(Ho):
            for j in range(Wo):
                assert torch.equal(y[n, i, j], x[n, 2 * i:2 * i + 3, 2 * j:2 * j + 3].reshape(9, C).max(0)[0])


@pytest.mark.parametrize("C_,npix", R.DIST_CASES)
def test_restated_distance_equals_a_direct_form(C_, npix):
    f0, f1, w = R.dist_features(C_, npix)
    a, b, ww = f0.double().numpy(), f1.double().numpy(), w.double().numpy()
    assert not a[0].any() and b[0].any() and not b[1].any() and not a[2].any() and not b[2].any()
    total = 0.0
    for p in range(npix):
        n0 = a[p] / (np.sqrt((a[p] ** 2).sum()) + 1e-10)
        n1 = b[p] / (np.sqrt((b[p] ** 2).sum()) + 1e-10)
        total += float((ww * (n0 - n1) ** 2).sum())
    d = R.layer_dist64(f0, f1, w)
    assert np.isfinite(d) and d == pytest.approx(total / npix, rel=1e-13)
    assert R.layer_dist64(f0, f0, w) == 0.0 and R.layer_dist64(f1, f0, w) == d
    assert R.layer_dist32(f0, f0, w) == 0.0 and R.layer_dist32(f1, f0, w) == R.layer_dist32(f0, f1, w)


def test_tap_sizes_and_the_smallest_image():
    assert lpips.tap_sizes(31, 31) == [(7, 7), (3, 3), (1, 1), (1, 1), (1, 1)]
    assert min(min(s) for s in lpips.tap_sizes(30, 31)) == 0
    assert lpips.LAYERS == R.LAYERS and lpips.SHIFT == R.SHIFT and lpips.SCALE == R.SCALE and lpips.MIN_SIZE == 31
    taps = R.features64(torch.rand(1, 35, 47, 3), R.random_weights(0))
    assert [tuple(t.shape[1:3]) for t in taps] == lpips.tap_sizes(35, 47)
    assert [t.shape[-1] for t in taps] == [l[1] for l in R.LAYERS]


# ---- the emulation inside the GPU test's bounds ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CONV_CASES, ids=[c[0] for c in R.CONV_CASES])
def test_binary32_emulation_of_the_convolution_is_inside_k_conv(case):
    name, _, _, _, _, _, _, stride, pad, _ = case
    x, w, b, aff = R.case_tensors(case)
    ref, absref = R.conv_relu64(x, w, b, stride, pad, aff)
    assert R.conv_ratio(R.conv_relu32(x, w, b, stride, pad, aff), ref, absref) <= R.K_CONV
    if name in R.CHAIN_CASES:
        assert R.conv_ratio(R.conv_relu_chain32(x, w, b, stride, pad, aff), ref, absref) <= R.K_CONV


def test_binary32_emulation_of_the_distances_is_inside_k_dist_and_k_e2e():
    assert R.K_CONV <= 8 and R.K_E2E <= 1e-4
    for C_, npix in R.DIST_CASES:
        f0, f1, w = R.dist_features(C_, npix)
        assert R.rel_err(R.layer_dist32(f0, f1, w), R.layer_dist64(f0, f1, w)) <= R.K_DIST
    wts = R.random_weights(0)
    aff = torch.stack([wts["shift"], wts["scale"]])
    for H, W in R.E2E_SIZES:
        a, b = R.image_pair(H, W)
        assert 0.0 <= float(a.min()) and float(a.max()) <= 1.0 and not torch.equal(a, b)
        d_ref, _ = R.lpips64(a, b, wts)
        taps = R.features32(torch.stack([a, b]), wts, conv=R.conv_relu_chain32)
        d32 = sum(R.layer_dist32(t[0], t[1], wts["lin"][l]) for l, t in enumerate(taps))
        assert R.rel_err(d32, d_ref) <= R.K_E2E
        x = torch.stack([a, b])
        for l, (_, _, k, stride, pad, pooled) in enumerate(R.LAYERS):          # chained, as the GPU test checks the layers
            if pooled:
                x = R.maxpool(x)
            ref, absref = R.conv_relu64(x, wts["conv_w"][l], wts["conv_b"][l], stride, pad, aff if l == 0 else None)
            assert R.conv_ratio(taps[l], ref, absref) <= R.K_CONV
            x = taps[l]


# ---- mutants of the definition ----------------------------------------------------------------------------------------------
def _mutant_lpips(img0, img1, wts, mutant):
    """the definition in float64 with one deliberate mistake"""
    shift, scale = wts["shift"].double(), wts["scale"].double()
    x = torch.stack([img0, img1]).double().permute(0, 3, 1, 2)

    def affine(t):
        s = shift if mutant != "shift_sign" else -shift
        return ((2.0 * t - 1.0) - s.view(1, 3, 1, 1)) / scale.view(1, 3, 1, 1)

    total = 0.0
    for l, (_, _, k, stride, pad, pooled) in enumerate(R.LAYERS):
        w, b = wts["conv_w"][l].double(), wts["conv_b"][l].double()
        if mutant == "transposed_taps":
            w = w.transpose(2, 3)
        if pooled:
            x = F.max_pool2d(x, 3, 3 if mutant == "pool_stride_3" else 2, ceil_mode=mutant == "ceil_pool")
        if l == 0 and mutant == "pad_before_affine":
            x, p = affine(F.pad(x, (pad, pad, pad, pad))), 0
        else:
            x, p = (affine(x) if l == 0 else x), pad
        if mutant == "no_bias":
            x = F.relu(F.conv2d(x, w, None, stride=stride, padding=p))
        elif mutant == "relu_before_bias":
            x = F.relu(F.conv2d(x, w, None, stride=stride, padding=p)) + b.view(1, -1, 1, 1)
        else:
            x = F.relu(F.conv2d(x, w, b, stride=stride, padding=p))
        f = x.permute(0, 2, 3, 1).reshape(2, -1, x.shape[1])
        total += _mutant_dist(f[0], f[1], wts["lin"][l].double(), mutant)
    return total


def _mutant_dist(f0, f1, w, mutant):
    eps = 0.0 if mutant == "no_eps" else R.EPS
    n0 = f0 / (f0.pow(2).sum(-1, keepdim=True).sqrt() + eps)
    n1 = f1 / (f1.pow(2).sum(-1, keepdim=True).sqrt() + eps)
    t = ((n0 - n1) * w).pow(2) if mutant == "w_inside_square" else (n0 - n1).pow(2) * w
    return float(t.sum(-1).sum() if mutant == "sum_not_mean" else t.sum(-1).mean())


MUTANTS = ("pad_before_affine", "shift_sign", "no_eps", "w_inside_square", "sum_not_mean", "ceil_pool", "pool_stride_3",
           "transposed_taps", "no_bias", "relu_before_bias")


def test_the_unmutated_form_is_the_restatement():
    wts = R.random_weights(0)
    a, b = R.image_pair(35, 47)
    assert _mutant_lpips(a, b, wts, None) == pytest.approx(R.lpips64(a, b, wts)[0], rel=1e-13)
    f0, f1, w = R.dist_features(64, 49)
    assert _mutant_dist(f0.double(), f1.double(), w.double(), None) == pytest.approx(R.layer_dist64(f0, f1, w), rel=1e-13)


@pytest.mark.parametrize("mutant", MUTANTS)
def test_mutants_of_the_definition_are_rejected(mutant):
    """each mistake moves the result outside the bound the GPU test holds the kernels to (or makes it NaN)"""
    if mutant == "no_eps":                       # only visible where a pixel's features are all zero
        f0, f1, w = R.dist_features(64, 49)
        got, ref, bound = _mutant_dist(f0.double(), f1.double(), w.double(), mutant), R.layer_dist64(f0, f1, w), R.K_DIST
    else:
        wts = R.random_weights(0)
        a, b = R.image_pair(97, 131)                # large enough for the stride-3 pools to leave a pixel
        got, ref, bound = _mutant_lpips(a, b, wts, mutant), R.lpips64(a, b, wts)[0], R.K_E2E
    assert not (R.rel_err(got, ref) <= bound)


# ---- the loader ----------------------------------------------------------------------------------------------------------
def _state_dicts(seed=3):
    wts = R.random_weights(seed)
    full, lin_only, backbone = {}, {}, {}
    for l in range(5):
        n = lpips.FEATURE_INDEX[l]
        full[f"net.slice{l + 1}.{n}.weight"] = backbone[f"features.{n}.weight"] = wts["conv_w"][l]
        full[f"net.slice{l + 1}.{n}.bias"] = backbone[f"features.{n}.bias"] = wts["conv_b"][l]
        full[f"lin{l}.model.1.weight"] = lin_only[f"lin{l}.model.1.weight"] = wts["lin"][l].reshape(1, -1, 1, 1)
        full[f"lins.{l}.model.1.weight"] = full[f"lin{l}.model.1.weight"]                # the duplicates: ignored
    full["scaling_layer.shift"] = wts["shift"].reshape(1, 3, 1, 1)
    full["scaling_layer.scale"] = wts["scale"].reshape(1, 3, 1, 1)
    backbone["classifier.1.weight"] = torch.zeros(8, 8)                                 # what else torchvision's dict holds
    return wts, full, lin_only, backbone


def _same(a, b):
    return all(torch.equal(x, y) for part in ("conv_w", "conv_b", "lin") for x, y in zip(a[part], b[part])) and \
        torch.equal(a["shift"], b["shift"]) and torch.equal(a["scale"], b["scale"])


def test_state_dicts_load_in_both_forms():
    wts, full, lin_only, backbone = _state_dicts()
    assert _same(lpips.weights_from_state_dict(full), wts)
    assert _same(lpips.weights_from_state_dict(lin_only, backbone), wts)
    assert _same(lpips.check_weights(lpips.random_weights(3)), wts)


def test_renamed_or_missized_keys_are_refused_by_name():
    _, full, lin_only, backbone = _state_dicts()
    for key in ("net.slice3.6.weight", "net.slice1.0.bias", "lin4.model.1.weight", "scaling_layer.scale"):
        sd = {(k + "_x" if k == key else k): v for k, v in full.items()}
        with pytest.raises(KeyError, match=re.escape(key)):
            lpips.weights_from_state_dict(sd)
    with pytest.raises(KeyError, match=re.escape("features.8.bias")):
        lpips.weights_from_state_dict(lin_only, {k: v for k, v in backbone.items() if k != "features.8.bias"})
    with pytest.raises(KeyError, match=re.escape("lin2.model.1.weight")):
        lpips.weights_from_state_dict({k: v for k, v in lin_only.items() if k != "lin2.model.1.weight"}, backbone)
    with pytest.raises(KeyError, match=re.escape("net.slice1.0.weight")):               # a bare alex.pth without the backbone
        lpips.weights_from_state_dict(lin_only)
    for key, bad in (("net.slice2.3.weight", torch.zeros(192, 64, 3, 3)), ("lin0.model.1.weight", torch.zeros(64)),
                     ("net.slice5.10.bias", torch.zeros(384)), ("scaling_layer.shift", torch.zeros(3))):
        with pytest.raises(ValueError, match=re.escape(key)):
            lpips.weights_from_state_dict({**full, key: bad})
    with pytest.raises(ValueError, match=re.escape("features.0.weight")):
        lpips.weights_from_state_dict(lin_only, {**backbone, "features.0.weight": torch.zeros(64, 3, 7, 7)})
    with pytest.raises(KeyError, match="lin"):
        lpips.check_weights({k: v for k, v in lpips.random_weights(0).items() if k != "lin"})


def test_rgb_lpips_refuses_without_weights_and_for_vgg():
    metrics.set_lpips(None)
    img = np.zeros((31, 31, 3), np.float32)
    with pytest.raises(RuntimeError, match="set_lpips"):
        metrics.rgb_lpips(img, img, "alex")
    with pytest.raises(NotImplementedError, match="VGG"):
        metrics.rgb_lpips(img, img, "vgg")
    with pytest.raises(ValueError):
        metrics.rgb_lpips(img, img, "squeeze")


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
def test_header_declares_the_lpips_entry_points_and_ctypes_agrees():
    header = open(os.path.join(ROOT, "include", "esr_hip.h")).read()
    # the names only: tests/test_host.py checks every entry's restype and argument types against the header text
    assert set(ENTRIES) <= set(_lib.EXPORTS)
    assert int(re.search(r"#define ESR_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == _lib.lib().esr_abi_version()
    assert int(re.search(r"#define ESR_CONV_KC (\d+)", header).group(1)) == 32
    assert int(re.search(r"#define ESR_METRICS_BLOCKS (\d+)", header).group(1)) == lpips._BLOCKS
    assert "utils2/metric.py:15-28" in header


def test_entry_points_check_their_arguments_before_any_launch():
    """Every code here is returned by the host-side checks: no pointer is read and nothing is launched"""
    L = _lib.lib()
    null, p = ctypes.c_void_p(0), ctypes.c_void_p(0x1000)                              # never dereferenced
    assert L.esr_conv_packed_floats(64, 3, 11, 11) == 384 * 64 and L.esr_conv_packed_floats(32, 5, 5, 5) == 128 * 32
    assert L.esr_conv_packed_floats(256, 384, 3, 3) == 3456 * 256 and L.esr_conv_packed_floats(0, 3, 3, 3) == -1
    assert L.esr_conv_pack(null, 32, 3, 3, 3, p, null) == -1 and L.esr_conv_pack(p, 32, 0, 3, 3, p, null) == -1
    assert L.esr_conv_pack(p, 1 << 20, 1 << 10, 3, 3, p, null) == -2

    def conv(N=1, H=8, W=8, Cin=4, Cout=32, k=3, stride=1, pad=1, x=p, packed=p, bias=p, y=p):
        return L.esr_conv_relu(x, N, H, W, Cin, packed, bias, Cout, k, k, stride, pad, null, y, null)

    for kw in (dict(Cout=48), dict(Cout=0), dict(N=0), dict(H=0), dict(W=-1), dict(Cin=0), dict(k=0), dict(stride=0), dict(pad=-1),
               dict(H=2, k=5, pad=1), dict(W=1, k=3, pad=0), dict(x=null), dict(packed=null), dict(bias=null), dict(y=null),
               dict(packed=ctypes.c_void_p(0x1004))):
        assert conv(**kw) == -1, kw
    for kw in (dict(N=1 << 10, H=1 << 10, W=1 << 10), dict(N=2, H=1 << 13, W=1 << 13, Cin=1, Cout=32),
               dict(Cin=1 << 15, Cout=1 << 15, k=3)):
        assert conv(**kw) == -2, kw
    for args, code in (((p, 1, 2, 8, 4, 3, 2, p, null), -1), ((p, 1, 8, 8, 4, 0, 2, p, null), -1), ((p, 1, 8, 8, 4, 3, 0, p, null), -1),
                       ((null, 1, 8, 8, 4, 3, 2, p, null), -1), ((p, 0, 8, 8, 4, 3, 2, p, null), -1),
                       ((p, 1 << 10, 1 << 10, 1 << 10, 4, 3, 2, p, null), -2)):
        assert L.esr_maxpool_nhwc(*args) == code, args
    for args, code in (((p, p, 0, 64, p, p, p, null), -1), ((p, p, 5, 0, p, p, p, null), -1), ((null, p, 5, 64, p, p, p, null), -1),
                       ((p, p, 5, 64, p, null, p, null), -1), ((p, p, 1 << 30, 64, p, p, p, null), -2)):
        assert L.esr_lpips_layer(*args) == code, args
