"""The LPIPS kernels (esr_nerf_amd/csrc/lpips.hip) on the device against the float64 restatement tests/lpips_ref64.py:
the convolution per value through the C ABI, the pool bit for bit against torch, a layer's distance, the whole metric on
the real AlexNet shapes with seeded weights, and the wiring into evaluate.view_metrics / metrics.rgb_lpips.  Every
figure a bound is held against is printed before the assertion (pytest -s shows them)."""
import ctypes as C

import numpy as np
import pytest
import torch

import lpips_ref64 as R
from esr_nerf_amd import _lib

pytestmark = pytest.mark.gpu

GUARD = 64                       # guard floats in front of and behind every buffer
SENTINEL = -12345.5              # what guards and untouched outputs hold


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


class Guarded:
    """A device copy of `t` (or `numel` sentinel floats) with GUARD sentinel floats on either side, its data optionally
    16 bytes further into the allocation"""

    def __init__(self, t=None, numel=None, shift16=False, dtype=torch.float32):
        n = t.numel() if t is not None else numel
        off = GUARD + (16 // torch.empty(0, dtype=dtype).element_size() if shift16 else 0)
        self.buf = torch.full((off + n + GUARD,), SENTINEL, dtype=dtype, device=_dev())
        self.data = self.buf[off:off + n]
        if t is not None:
            self.data.copy_(t.reshape(-1).to(dtype))
        self.lo, self.hi = self.buf[:off], self.buf[off + n:]
        self.saved = self.data.clone()

    @property
    def ptr(self):
        return C.c_void_p(self.data.data_ptr())

    def guards_intact(self):
        return bool((self.lo == SENTINEL).all()) and bool((self.hi == SENTINEL).all())

    def unchanged(self):
        return torch.equal(self.data.view(torch.int32), self.saved.view(torch.int32))


def _st():
    return _lib.stream_ptr(_dev())


def run_conv(x, w, b, aff, stride, pad, shift16=False):
    """(y [N,Ho,Wo,Cout] on the host, every buffer of the call) of esr_conv_relu on channels-last x"""
    L = _lib.lib()
    N, H, W, Cin = x.shape
    Cout, _, kh, kw = w.shape
    gx, gw, gb = Guarded(x, shift16=shift16), Guarded(w), Guarded(b, shift16=shift16)
    ga = Guarded(aff, shift16=shift16) if aff is not None else None
    gp = Guarded(numel=L.esr_conv_packed_floats(Cout, Cin, kh, kw), shift16=shift16)
    _lib.check(L.esr_conv_pack(gw.ptr, Cout, Cin, kh, kw, gp.ptr, _st()), "esr_conv_pack")
    torch.cuda.synchronize()
    gp.saved = gp.data.clone()
    Ho, Wo = R.conv_out(H, kh, stride, pad), R.conv_out(W, kw, stride, pad)
    gy = Guarded(numel=N * Ho * Wo * Cout, shift16=shift16)
    _lib.check(L.esr_conv_relu(gx.ptr, N, H, W, Cin, gp.ptr, gb.ptr, Cout, kh, kw, stride, pad,
                               ga.ptr if ga is not None else C.c_void_p(0), gy.ptr, _st()), "esr_conv_relu")
    torch.cuda.synchronize()
    bufs = {n: g for n, g in (("x", gx), ("w", gw), ("bias", gb), ("affine", ga), ("packed", gp), ("y", gy)) if g is not None}
    return gy.data.cpu().reshape(N, Ho, Wo, Cout), bufs


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("case", R.CONV_CASES, ids=[c[0] for c in R.CONV_CASES])
def test_convolution_per_value_against_float64(case):
    name, N, H, W, Cin, Cout, k, stride, pad, _ = case
    x, w, b, aff = R.case_tensors(case)
    ref, absref = R.conv_relu64(x, w, b, stride, pad, aff)
    y, bufs = run_conv(x, w, b, aff, stride, pad)
    ratio = R.conv_ratio(y, ref, absref)
    print(f"\nlpips conv {name}: worst |gpu - ref64| / (2^-24 absref) = {ratio:.3f}  (K_CONV {R.K_CONV})")
    assert tuple(y.shape) == tuple(ref.shape) and bool(torch.isfinite(y).all())
    assert ratio <= R.K_CONV
    # the packed weight: the documented order, the zero rows exact
    packed = bufs["packed"].data.cpu().numpy().reshape(-1, Cout)
    K = Cin * k * k
    assert packed.shape[0] % 32 == 0 and packed.shape[0] - K < 32
    assert np.array_equal(packed[:K], R.weight_matrix(w.numpy())) and not packed[K:].any()
    # nothing outside the buffers is written, the inputs are left bit for bit
    assert all(g.guards_intact() for g in bufs.values())
    assert all(g.unchanged() for n, g in bufs.items() if n != "y")
    # a second call, and a call on pointers 16 bytes further on, give the same bits
    y2, _ = run_conv(x, w, b, aff, stride, pad)
    y3, bufs3 = run_conv(x, w, b, aff, stride, pad, shift16=True)
    assert torch.equal(_bits(y), _bits(y2)) and torch.equal(_bits(y), _bits(y3))
    assert all(g.guards_intact() for g in bufs3.values()) and all(g.unchanged() for n, g in bufs3.items() if n != "y")
    if name in R.CHAIN_CASES:
        # the documented order: one k-ascending chain of fused multiply-adds per value, bias and ReLU behind it
        chain = R.conv_relu_chain32(x, w, b, stride, pad, aff)
        differ = int((_bits(y) != _bits(chain)).sum())
        print(f"lpips conv {name}: {differ} of {y.numel()} values differ in bits from the k-ordered chain")
        assert differ == 0


@pytest.mark.parametrize("name", ["first-35x47", "conv2-11x15"])
def test_an_image_gives_the_same_bits_in_either_slot_of_a_batch(name):
    case = next(c for c in R.CONV_CASES if c[0] == name)
    _, _, _, _, _, _, _, stride, pad, _ = case
    x, w, b, aff = R.case_tensors(case)
    other = R.case_tensors(case, seed=1)[0]
    alone, _ = run_conv(x, w, b, aff, stride, pad)
    first, _ = run_conv(torch.cat([x, other]), w, b, aff, stride, pad)
    second, _ = run_conv(torch.cat([other, x]), w, b, aff, stride, pad)
    assert torch.equal(_bits(alone[0]), _bits(first[0])) and torch.equal(_bits(alone[0]), _bits(second[1]))
    assert torch.equal(_bits(first[1]), _bits(second[0]))


def test_a_channel_count_off_the_tile_is_refused_and_nothing_is_written():
    L = _lib.lib()
    x, w, b = torch.randn(1, 6, 6, 4), torch.randn(48, 4, 3, 3), torch.randn(48)
    gx, gw, gb = Guarded(x), Guarded(w), Guarded(b)
    gp = Guarded(numel=L.esr_conv_packed_floats(48, 4, 3, 3))
    _lib.check(L.esr_conv_pack(gw.ptr, 48, 4, 3, 3, gp.ptr, _st()), "esr_conv_pack")
    gy = Guarded(numel=6 * 6 * 48)
    null = C.c_void_p(0)
    assert L.esr_conv_relu(gx.ptr, 1, 6, 6, 4, gp.ptr, gb.ptr, 48, 3, 3, 1, 1, null, gy.ptr, _st()) == -1
    assert L.esr_conv_relu(gx.ptr, 1, 6, 6, 4, gp.ptr, gb.ptr, 32, 9, 3, 1, 1, null, gy.ptr, _st()) == -1      # empty output
    torch.cuda.synchronize()
    assert bool((gy.buf == SENTINEL).all())


@pytest.mark.parametrize("shape", R.POOL_CASES, ids=["7to3", "3to1", "8x11to3x5"])
def test_pool_is_bit_equal_to_torch(shape):
    L = _lib.lib()
    N, H, W, Cc = shape
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(H * W)) - 0.5
    x[0, 0, 0, 0] = -0.0
    want = R.maxpool(x)
    assert bool((want < 0).any())
    gx, gy = Guarded(x, shift16=True), Guarded(numel=want.numel())
    _lib.check(L.esr_maxpool_nhwc(gx.ptr, N, H, W, Cc, 3, 2, gy.ptr, _st()), "esr_maxpool_nhwc")
    torch.cuda.synchronize()
    assert tuple(want.shape[1:3]) == (R.conv_out(H, 3, 2, 0), R.conv_out(W, 3, 2, 0))
    assert torch.equal(_bits(gy.data.cpu().reshape(want.shape)), _bits(want))
    assert gx.guards_intact() and gy.guards_intact() and gx.unchanged()


def run_layer(f0, f1, w):
    L = _lib.lib()
    g0, g1, gw = Guarded(f0), Guarded(f1), Guarded(w)
    part = Guarded(numel=1024, dtype=torch.float64)
    out = Guarded(numel=1, dtype=torch.float64)
    _lib.check(L.esr_lpips_layer(g0.ptr, g1.ptr, f0.shape[0], f0.shape[1], gw.ptr, part.ptr, out.ptr, _st()), "esr_lpips_layer")
    torch.cuda.synchronize()
    assert all(g.guards_intact() for g in (g0, g1, gw, part, out)) and g0.unchanged() and g1.unchanged() and gw.unchanged()
    return float(out.data[0])


@pytest.mark.parametrize("C_,npix", R.DIST_CASES)
def test_layer_distance_against_float64(C_, npix):
    f0, f1, w = R.dist_features(C_, npix)
    ref = R.layer_dist64(f0, f1, w)
    got = run_layer(f0, f1, w)
    err = R.rel_err(got, ref)
    print(f"\nlpips layer C={C_} npix={npix}: relative error {err:.3e}  (K_DIST {R.K_DIST:.3e})")
    assert np.isfinite(got) and err <= R.K_DIST
    assert run_layer(f1, f0, w) == got == run_layer(f0, f1, w)
    assert run_layer(f0, f0, w) == 0.0 and run_layer(torch.zeros_like(f0), torch.zeros_like(f0), w) == 0.0


@pytest.fixture(scope="module")
def model():
    from esr_nerf_amd.lpips import LpipsAlex
    return LpipsAlex.random(0, _dev())


def test_random_model_is_the_restated_draw(model):
    want = R.random_weights(0)
    for part in ("conv_w", "conv_b", "lin"):
        assert all(torch.equal(a, b) for a, b in zip(model.weights[part], want[part]))
    assert torch.equal(model.weights["shift"], want["shift"]) and torch.equal(model.weights["scale"], want["scale"])


@pytest.mark.parametrize("H,W", R.E2E_SIZES)
def test_whole_metric_on_the_alexnet_shapes(model, H, W):
    from esr_nerf_amd.lpips import tap_sizes
    a, b = R.image_pair(H, W)
    c = R.image_pair(H, W, seed=1)[1]
    wts = model.weights
    feats = model.features(torch.stack([a, b]))
    assert [tuple(f.shape[1:3]) for f in feats] == tap_sizes(H, W)
    aff = torch.stack([wts["shift"], wts["scale"]])
    x = torch.stack([a, b])
    for l, (_, _, k, stride, pad, pooled) in enumerate(R.LAYERS):            # each layer on the device's own previous output
        if pooled:
            x = R.maxpool(x)
        ref, absref = R.conv_relu64(x, wts["conv_w"][l], wts["conv_b"][l], stride, pad, aff if l == 0 else None)
        x = feats[l].cpu()
        ratio = R.conv_ratio(x, ref, absref)
        print(f"\nlpips e2e {H}x{W} layer {l}: worst ratio {ratio:.3f}  (K_CONV {R.K_CONV})")
        assert ratio <= R.K_CONV
    d = model.distance(feats, 0, 1)
    assert d.dtype == torch.float64 and d.is_cuda
    d_ref, layers_ref = R.lpips64(a, b, wts)
    err = R.rel_err(d, d_ref)
    print(f"lpips e2e {H}x{W}: d = {float(d):.9g}, ref64 {d_ref:.9g}, relative error {err:.3e}  (K_E2E {R.K_E2E:.3e})")
    assert d_ref > 0 and err <= R.K_E2E
    per_layer = model.layers(feats, 0, 1).tolist()
    assert len(per_layer) == len(layers_ref) == 5 and (((per_layer[0] + per_layer[1]) + per_layer[2]) + per_layer[3]) + per_layer[4] == float(d)
    assert float(d) == model(a, b) == model(b, a) == float(model.distance(feats, 1, 0))
    assert model(a, a) == 0.0
    feats3 = model.features(torch.stack([a, b, c]))                          # the batch of three: the target's taps once
    assert float(model.distance(feats3, 0, 1)) == model(a, b) and float(model.distance(feats3, 0, 2)) == model(a, c)


def test_view_metrics_and_rgb_lpips_carry_the_metric(model):
    from esr_nerf_amd import evaluate, metrics
    H, W = 40, 33
    g = torch.Generator().manual_seed(5)
    rgbs = torch.rand(H, W, 3, generator=g).to(_dev())
    results = {k: (rgbs + 0.1 * torch.rand(H, W, 3, generator=g).to(_dev())).clamp(0, 1) for k in ("lin/rgb", "lin/rgb_gamma", "srgb/rgb")}
    plain = evaluate.view_metrics(results, rgbs)
    with_l = evaluate.view_metrics(results, rgbs, lpips=model)
    assert set(with_l) - set(plain) == {"lin/LPIPS_ALEX", "srgb/LPIPS_ALEX"} and set(plain) <= set(with_l)
    assert all(with_l[k] == v for k, v in plain.items())
    assert with_l["lin/LPIPS_ALEX"] == model(rgbs, results["lin/rgb_gamma"]) > 0
    assert with_l["srgb/LPIPS_ALEX"] == model(rgbs, results["srgb/rgb"]) > 0
    lin_only = evaluate.view_metrics({k: v for k, v in results.items() if k != "srgb/rgb"}, rgbs, lpips=model)
    assert "srgb/LPIPS_ALEX" not in lin_only and lin_only["lin/LPIPS_ALEX"] == with_l["lin/LPIPS_ALEX"]
    try:
        assert metrics.set_lpips(model) is model
        assert metrics.rgb_lpips(rgbs.cpu().numpy(), results["srgb/rgb"].cpu().numpy(), "alex") == with_l["srgb/LPIPS_ALEX"]
        assert metrics.rgb_lpips(rgbs, results["srgb/rgb"], "alex", _dev()) == with_l["srgb/LPIPS_ALEX"]
    finally:
        metrics.set_lpips(None)
