"""Float64 restatement of LPIPS-Alex (version 0.1, normalize=True, eval mode), written from the definition and not from
the kernels; the yardstick of tests/test_lpips_host.py and tests/test_gpu_lpips.py.

Definition.  Two images [H, W, 3] float32 in [0, 1].  Per image: t = 2 x - 1, s_c = (t - shift_c) / scale_c (zero padding
applies to s); five taps, each behind its ReLU: conv(3->64, k11, s4, p2); maxpool(3, 2) conv(64->192, k5, p2); maxpool(3, 2)
conv(192->384, k3, p1); conv(384->256, k3, p1); conv(256->256, k3, p1), all with bias, the pool in floor mode without
padding.  Per tap and pixel n = f / (sqrt(sum_c f_c^2) + 1e-10), d_l = mean_pixels sum_c w_c (n0_c - n1_c)^2; LPIPS = sum_l d_l.

Parts: the network through F.conv2d / F.max_pool2d in float64 on the CPU; absref = conv(|s|, |w|) + |b|, the scale of a
value's rounding error; a binary32 emulation (torch float32 ops, and the k-ordered fused-multiply-add chain the header
documents, for small cases); the case tables and the constants of the GPU test.

Everything here is channels-last ([N, H, W, C]) at its interface, as the kernels are.
"""
import numpy as np
import torch
import torch.nn.functional as F

LAYERS = ((3, 64, 11, 4, 2, False), (64, 192, 5, 1, 2, True), (192, 384, 3, 1, 1, True), (384, 256, 3, 1, 1, False),
          (256, 256, 3, 1, 1, False))
SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
EPS = 1e-10
U = 2.0 ** -24                      # unit roundoff of binary32

# ---- the constants of tests/test_gpu_lpips.py ------------------------------------------------------------------------------
# Each is the next power of two above the worst ratio measured on an MI355X against this restatement (the project's
# convention, K_FAMILY of tests/mlp_ref64.py); the measured ratios stand beside them.
#   K_CONV   |gpu - ref64| <= K_CONV * 2^-24 * absref per value.  Known in advance: the f32 MFMA's error is 0.75 - 1.5e-7
#            sum|a b| for K <= 1024 and 3.5e-7 at K = 4096, i.e. 1.3 - 6 units; above 8 would be a bug, not a constant.
#   K_DIST   relative error of one layer's distance against float64 on the same float32 features
#   K_E2E    relative error of the whole distance; never above 1e-4, the project's fp32 parity bar
K_CONV = 8.0            # worst measured 5.333 (a K = 36 chain over 2.6 M values); the emulation gives the same 5.333
K_DIST = 2.0 ** -26     # 1.49e-8; worst measured 1.029e-8
K_E2E = 2.0 ** -20      # 9.54e-7; worst measured 6.406e-7
MEASURED = {            # one MI355X, tests/test_gpu_lpips.py, every case; the kernel's bits equalled the k-ordered chain's everywhere
    "conv": {"first-31x31": 2.320, "first-35x47": 2.203, "oddK-7x9": 2.632, "pad-1x1": 1.342, "pad-1x2": 2.069,
             "conv2-11x15": 4.205, "tiles-2x200x203": 5.333, "conv4-5x7": 3.313},
    "e2e_layers": {"31x31": (2.491, 2.198, 1.830, 2.188, 1.766), "35x47": (3.614, 2.853, 2.844, 3.052, 2.864),
                   "64x64": (2.971, 3.376, 3.659, 3.332, 3.135), "97x131": (4.318, 3.294, 3.321, 4.186, 3.076)},
    "dist": {64: 1.029e-8, 192: 7.934e-9, 384: 4.459e-9, 256: 2.690e-9},
    "e2e": {"31x31": 4.930e-7, "35x47": 1.378e-7, "64x64": 6.406e-7, "97x131": 4.561e-8},
}

# ---- case tables --------------------------------------------------------------------------------------------------------
# name, N, H, W, Cin, Cout, k, stride, pad, affine
CONV_CASES = (
    ("first-31x31", 1, 31, 31, 3, 32, 11, 4, 2, True),
    ("first-35x47", 1, 35, 47, 3, 32, 11, 4, 2, True),
    ("oddK-7x9", 1, 7, 9, 5, 32, 5, 1, 2, False),                  # K = 125: the zero rows of the packed weight
    ("pad-1x1", 1, 1, 1, 32, 64, 3, 1, 1, False),                  # all taps but one are padding
    ("pad-1x2", 1, 1, 2, 32, 64, 3, 1, 1, False),
    ("conv2-11x15", 1, 11, 15, 64, 192, 5, 1, 2, False),
    ("tiles-2x200x203", 2, 200, 203, 4, 32, 3, 1, 1, False),       # 1269 pixel tiles: more than one pass of the launcher
    ("conv4-5x7", 1, 5, 7, 384, 256, 3, 1, 1, False),              # K = 3456
)
CHAIN_CASES = tuple(c[0] for c in CONV_CASES)                  # all are small enough for the k-ordered chain
POOL_CASES = ((1, 7, 7, 64), (2, 3, 3, 192), (1, 8, 11, 5))        # N, H, W, C: 7 -> 3, 3 -> 1, 8 x 11 -> 3 x 5
DIST_CASES = ((64, 49), (192, 9), (384, 5), (256, 70))             # C, pixels
E2E_SIZES = ((31, 31), (35, 47), (64, 64), (97, 131))


def conv_out(size, k, stride, pad):
    return (size + 2 * pad - k) // stride + 1


def case_tensors(case, seed=0):
    """x [N,H,W,Cin] f32 (in [0, 1] under the affine, N(0, 1) otherwise), w [Cout,Cin,k,k], b [Cout], affine ([2,Cin] or None)"""
    name, N, H, W, Cin, Cout, k, stride, pad, affine = case
    g = torch.Generator().manual_seed(1000 + seed + sum(map(ord, name)))
    x = torch.rand(N, H, W, Cin, generator=g) if affine else torch.randn(N, H, W, Cin, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) * float(np.sqrt(2.0 / (Cin * k * k)))
    b = torch.rand(Cout, generator=g) * 0.2 - 0.1
    aff = torch.tensor([SHIFT, SCALE], dtype=torch.float32) if affine else None
    return x, w, b, aff


# ---- float64 ------------------------------------------------------------------------------------------------------------
def affine64(x, aff):
    """s = ((2 x - 1) - shift) / scale in float64, the float32 constants taken as they are"""
    x = x.double()
    return x if aff is None else ((2.0 * x - 1.0) - aff[0].double()) / aff[1].double()


def conv_relu64(x, w, b, stride, pad, aff=None):
    """(y, absref) [N,Ho,Wo,Cout] float64: y = relu(conv(s, w) + b), absref = conv(|s|, |w|) + |b|"""
    s = affine64(x, aff).permute(0, 3, 1, 2)
    y = F.relu(F.conv2d(s, w.double(), b.double(), stride=stride, padding=pad))
    a = F.conv2d(s.abs(), w.double().abs(), b.double().abs(), stride=stride, padding=pad)
    return y.permute(0, 2, 3, 1).contiguous(), a.permute(0, 2, 3, 1).contiguous()


def maxpool(x, k=3, stride=2):
    """F.max_pool2d (floor mode, no padding) of [N,H,W,C], any float dtype; exact"""
    return F.max_pool2d(x.permute(0, 3, 1, 2), k, stride).permute(0, 2, 3, 1).contiguous()


def features64(images, weights):
    """the five taps [N,Ho,Wo,C] float64 of images [N,H,W,3]"""
    aff = torch.stack([weights["shift"], weights["scale"]])
    x, taps = images, []
    for l, (_, _, k, stride, pad, pooled) in enumerate(LAYERS):
        if pooled:
            x = maxpool(x)
        x, _ = conv_relu64(x, weights["conv_w"][l], weights["conv_b"][l], stride, pad, aff if l == 0 else None)
        taps.append(x)
    return taps


def layer_dist64(f0, f1, w):
    """d_l of two taps [..., C] (any float dtype, taken as they are) and the lin weight [C], as a Python float"""
    f0, f1, w = f0.double().reshape(-1, f0.shape[-1]), f1.double().reshape(-1, f1.shape[-1]), w.double()
    n0 = f0 / (f0.pow(2).sum(-1, keepdim=True).sqrt() + EPS)
    n1 = f1 / (f1.pow(2).sum(-1, keepdim=True).sqrt() + EPS)
    return float(((n0 - n1).pow(2) * w).sum(-1).mean())


def lpips64(img0, img1, weights):
    """(distance, [d_l]) of two images [H,W,3]"""
    taps = features64(torch.stack([img0, img1]), weights)
    d = [layer_dist64(t[0], t[1], weights["lin"][l]) for l, t in enumerate(taps)]
    return sum(d), d


# ---- binary32 emulation -------------------------------------------------------------------------------------------------
def affine32(x, aff):
    """the kernel's input affine: 2 x - 1, minus shift, a correctly rounded division, each in binary32"""
    if aff is None:
        return x.float()
    return ((2.0 * x.float() - 1.0) - aff[0].float()) / aff[1].float()


def conv_relu32(x, w, b, stride, pad, aff=None):
    """torch's float32 convolution (its own summation order) behind the binary32 affine"""
    s = affine32(x, aff).permute(0, 3, 1, 2)
    return F.relu(F.conv2d(s, w.float(), b.float(), stride=stride, padding=pad)).permute(0, 2, 3, 1).contiguous()


def im2col(s, k, stride, pad):
    """[M, K] patches of s [N,H,W,C] (numpy) in the kernels' reduction order: column (ky k + kx) C + c"""
    N, H, W, C = s.shape
    Ho, Wo = conv_out(H, k, stride, pad), conv_out(W, k, stride, pad)
    p = np.zeros((N, H + 2 * pad, W + 2 * pad, C), s.dtype)
    p[:, pad:pad + H, pad:pad + W] = s
    cols = [p[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride] for ky in range(k) for kx in range(k)]
    return np.concatenate(cols, axis=-1).reshape(N * Ho * Wo, k * k * C), (N, Ho, Wo)


def weight_matrix(w):
    """[K, Cout] of w [Cout,Cin,k,k] (numpy) in the same order: row (ky k + kx) Cin + c"""
    return np.ascontiguousarray(w.transpose(2, 3, 1, 0).reshape(-1, w.shape[0]))


def conv_relu_chain32(x, w, b, stride, pad, aff=None):
    """The documented order: per value acc = +0, acc = fmaf(patch[k], w[k][n], acc) for k ascending, y = acc + b, ReLU.
    fmaf through float64: the product of two binary32 numbers is exact there, the sum is rounded to 53 and then to 24 bits."""
    A, (N, Ho, Wo) = im2col(affine32(x, aff).numpy(), w.shape[-1], stride, pad)
    B = weight_matrix(w.float().numpy())
    acc = np.zeros((A.shape[0], B.shape[1]), np.float32)
    A64, B64 = A.astype(np.float64), B.astype(np.float64)
    for kk in range(A.shape[1]):
        acc = (A64[:, kk:kk + 1] * B64[kk:kk + 1, :] + acc.astype(np.float64)).astype(np.float32)
    y = acc + b.float().numpy()[None, :]
    return torch.from_numpy(np.where(y > 0, y, np.float32(0)).astype(np.float32).reshape(N, Ho, Wo, -1))


def _norm_den32(f):
    """sqrtf(sum_c f_c^2) + 1e-10f per pixel in the documented order: lane l of 64 adds c = l, l + 64, ... (product and
    sum separately rounded), then a butterfly over the lanes (offsets 32, 16, ... 1)"""
    f = f.astype(np.float32)
    npix, C = f.shape
    padded = np.zeros((npix, (C + 63) // 64 * 64), np.float32)
    padded[:, :C] = f
    lanes = np.zeros((npix, 64), np.float32)
    for r in range(padded.shape[1] // 64):
        u = padded[:, 64 * r:64 * r + 64]
        lanes = np.where(np.arange(64)[None, :] + 64 * r < C, lanes + u * u, lanes).astype(np.float32)
    for off in (32, 16, 8, 4, 2, 1):
        lanes = (lanes + lanes[:, np.arange(64) ^ off]).astype(np.float32)
    return np.sqrt(lanes[:, 0]).astype(np.float32) + np.float32(EPS)


def layer_dist32(f0, f1, w):
    """the layer kernel's arithmetic: norms, quotients and their difference in binary32 in the documented order, float64
    from there (the order of the float64 sums is immaterial at these bounds)"""
    a, b = f0.float().reshape(-1, f0.shape[-1]).numpy(), f1.float().reshape(-1, f1.shape[-1]).numpy()
    d = (a / _norm_den32(a)[:, None]).astype(np.float32) - (b / _norm_den32(b)[:, None]).astype(np.float32)
    d = d.astype(np.float32).astype(np.float64)
    return float(((d * d) * w.double().numpy()[None, :]).sum(-1).mean())


def features32(images, weights, conv=conv_relu32):
    aff = torch.stack([weights["shift"], weights["scale"]])
    x, taps = images.float(), []
    for l, (_, _, k, stride, pad, pooled) in enumerate(LAYERS):
        if pooled:
            x = maxpool(x)
        x = conv(x, weights["conv_w"][l], weights["conv_b"][l], stride, pad, aff if l == 0 else None)
        taps.append(x)
    return taps


# ---- shared data and figures ----------------------------------------------------------------------------------------------
def random_weights(seed=0):
    """the draw of esr_nerf_amd.lpips.LpipsAlex.random, restated (CPU float32 tensors)"""
    g = torch.Generator().manual_seed(int(seed))
    w = {"conv_w": [], "conv_b": [], "lin": [], "shift": torch.tensor(SHIFT), "scale": torch.tensor(SCALE)}
    for cin, cout, k, _, _, _ in LAYERS:
        w["conv_w"].append(torch.randn(cout, cin, k, k, generator=g) * float(np.sqrt(2.0 / (cin * k * k))))
        w["conv_b"].append(torch.rand(cout, generator=g) * 0.2 - 0.1)
        w["lin"].append(torch.rand(cout, generator=g) * 0.1)
    return w


def image_pair(H, W, seed=0):
    """two related images [H,W,3] in [0, 1]: a smooth random field and a perturbed copy of it"""
    g = torch.Generator().manual_seed(77 + seed + 1000 * H + W)
    base = F.interpolate(torch.rand(1, 3, H // 4 + 2, W // 4 + 2, generator=g), size=(H, W), mode="bilinear", align_corners=False)[0]
    a = (base + 0.1 * torch.rand(3, H, W, generator=g)).clamp(0, 1).permute(1, 2, 0).contiguous()
    b = (base + 0.2 * torch.rand(3, H, W, generator=g) - 0.05).clamp(0, 1).permute(1, 2, 0).contiguous()
    return a, b


def dist_features(C, npix, seed=0):
    """f0, f1 [npix, C] float32 post-ReLU-like features with all-zero pixels in one image (pixel 0: f0, pixel 1: f1) and
    in both (pixel 2), and w [C] in [0, 0.1)"""
    g = torch.Generator().manual_seed(500 + seed + C)
    f0, f1 = torch.randn(npix, C, generator=g).clamp_min(0), torch.randn(npix, C, generator=g).clamp_min(0)
    f0[0] = 0
    f1[1] = 0
    f0[2] = 0
    f1[2] = 0
    return f0, f1, torch.rand(C, generator=g) * 0.1


def conv_ratio(got, ref, absref):
    """worst |got - ref| / (2^-24 absref) over all values"""
    return float(((got.double() - ref).abs() / (U * absref)).max())


def rel_err(got, ref):
    return abs(float(got) - float(ref)) / abs(float(ref))
