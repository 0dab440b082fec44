"""Float64 restatement of the tiny-MLP engine's f32 and split-fp16 entry points (csrc/mlp.hip, csrc/mlp_split.hip,
csrc/tone_wgrad.hip), with a binary32 emulation of each entry, the mask word decoder / encoder and the input builders shared by
tests/test_mlp_ref64_host.py and tests/test_gpu_mlp_ref64.py; never imported by the product path.

Written from what include/esr_hip.h and csrc/mlp_common.h document, not from the kernels' arithmetic:
  nets        radiance 85-192-192-192-3, tone mapper 33-192-3, BRDF 76-128-128-128-5, emission 76-128-128-128-3, coarse 57-128-128-3
              (net_desc); X is tile-major [tile][row][32]; row r of the tile feeds reference column in_colmap(kind, r) (none: the row
              contributes nothing); the first cw rows are read from the colour group at color_row0.
  forward     pre[l] = W_l h[l-1] + b_l, h[l] = relu(pre[l]), z = W_out h + b_out in rows 0 .. out_dim-1 of a [zrows][32] tile whose
              other rows are exactly 0; H[l] = h[l] and the mask bit (pre[l] > 0) are saved where the launch saves.
  masks       M[l] is [tile][word wd][lane]: bit b of word wd in lane s + 32 h is feature 32 (2 wd + (b >> 4)) + acc_row(b & 15, h) of
              sample s, acc_row(r, h) = (r & 3) + 8 (r >> 2) + 4 h.
  dgrad       dZ[last] = m (.) (W_out^T dz), dZ[l-1] = m (.) (W_l^T dZ[l]), dX = W_0^T dZ[0] on rows 0 .. written-1 (44 for the sample
              nets, 36 for the tone mapper, 32 for the coarse net); a written row without a reference column is exactly 0; the
              rows above keep their bits.  Given M this is linear: no decisions.
  wgrad       gw[l] += dZ[l] h[l-1]^T, gb[l] += sum dZ[l] in the reference's [out, in] layout (h[-1]: the input in reference order).
  tone wgrad  the same two layers from Xt, dzt, W0, b0, W1 with the hidden layer recomputed (mask: pre > 0).
  absmax      out = max(out, max |x|); amax of the split input gradients: max(amax, max |dz| x max(1, G / 16)) over the rows
              0 .. out_dim-1 of the launch's tiles, in binary32, G = max over the hidden layers of the running product of the layers'
              largest column sums of |W| (output layer first, first layer excluded) and 1 (`gain_bound`).

Every entry returns, per output, (value, absref, zero): a value is checked as |got - value| <= K * U * absref + FLOOR (shade_ref64's
`compare`); absref is first order, in the algebra of lts_ref64's `Q` (E >= |binary32 result - value| / U):
  dot product in fp32, n terms behind a bias      E = sum |w_k| E_{x_k} + (n + 1) (|b| + sum |w_k x_k|)                    (`lin`)
  ReLU                                           1-Lipschitz: E_h = E_pre where the unit is on or within DEC_K U E_pre of 0, else 0; the
                                                 forward's VALUES therefore need no decision handling, only the mask bits do.
  split-fp16 product w x -> w1 x1 + w1 x2 + w2 x1, x1 = fp16(x), x2 = fp16(x - x1), weights stored x 64:
      |x - x1 - x2| <= 2^-22 |x| = 4 U |x| while x2 is a normal fp16 number, else 2^-25 = U / 2 absolute; the same for 64 w
      (U / 128 absolute after the 1 / 64); the dropped w2 x2 <= 2^-11 |w| 2^-11 |x| = 4 U |w x|.  Per product
          E_split = |w| (4 |x| + f_x) + |x| (4 |w| + 1 / 128) + 4 |w x| = 12 |w x| + f_x |w| + |x| / 128,
      f_x = 1 / 2 for an unscaled operand (inputs, activations).
  split input gradients   the tile's chain runs times 2^k with G max |dz| 2^k in [2^14, 2^15), G rounded up to a power of two: f_x = (1 / 2) 2^-k <= G max|dz| 2^-14,
                          max |dz| that of the TILE -- an absolute term proportional to G max |dz| of the tile.
  split weight gradients  the gradient operand runs times s with B s in [2^7, 2^8), B = *amax: f = (1 / 2) / s <= B 2^-8 on the
                          gradient operand, 1 / 2 on the activation operand: per addend 12 |a b| + B 2^-8 |b| + |a| / 2.
  weight-gradient sums    Q's sum rule E = sum E_i + r sum |v_i| with r the roundings on an addend's path: the samples one workgroup
                          accumulates (32 per tile of its share; the launch's <= 256 workgroups are shared by <= 16 layer jobs), the
                          slab reduction (REDUCE_PG = 32 partial sums), one float atomic per group of partials -- `wg_rounds` --
                          and |prefill| + |total| for the atomics' magnitude.  The tone mapper's kernels: two tiles per workgroup and
                          trip, grid <= 256 (f32) / 512 (split) -- `tone_rounds`.
Mask bits are decisions: bit = (float64 pre-activation > 0); a differing bit is accepted only where |pre| < DEC_K U E_pre (an exact 0
or -0 with E = 0 must give 0), at most max(2, decisions / 20000) per case; flips are counted.  The tone mapper's weight gradient
recomputes its mask, so its cases are built with every |pre| outside that band (asserted by the builder; seeds in TONE_CASES).
Values with a subnormal binary32 magnitude are counted (`Ref.note`), not exempted; with the smallest dz at 1e-20 no case produces one.
What the first run on the MI355X showed: every documented edge held -- the padding rows of z, the written dX rows without a reference
column (coarse rows 12-23, tone mapper rows 33-35: exactly 0), tiles outside the range, `amax` over a non-zero prefill -- so neither
a kernel nor the header needed a correction; 8 of 1.5e8 mask bits differed from the float64 sign, all inside the band; in four
families the device's worst ratio equals the emulation's to three digits (few-term products of exact binary32 or fp16-plane
operands round the same way in either), and in none does it exceed four times the emulation's (K_FAMILY)."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from grid_ref64 import bits, same_bits  # noqa: F401  (same_bits: re-exported for the tests)
from lts_ref64 import Q  # noqa: F401  (the algebra `lin` applies in matrix form)
from shade_ref64 import DEC_K, FLOOR, U, Ref, compare

F32, F64, I32 = torch.float32, torch.float64, torch.int32
TINY = 2.0 ** -126
RADIANCE, TONEMAP, BRDF, EMIT, COARSE = range(5)
KIND_NAME = {RADIANCE: "radiance", TONEMAP: "tonemap", BRDF: "brdf", EMIT: "emit", COARSE: "coarse"}
ESR_EINVAL, ESR_ECAP = -1, -2
H_FILL, M_FILL = 9.0, 0x07070707
REDUCE_PG, WG_GRID, WG_MAX_JOBS = 32, 256, 16


def acc_row(r, h):
    return (r & 3) + 8 * (r >> 2) + 4 * h


def _sample_colmap(n_view):
    """colour6 | sdf | feat24 | normal12 | xyz3 sin15 cos15 [| view9] rows -> the reference's column order"""
    def f(row):
        if row < 6: return row
        base = 39 + n_view
        if row == 6: return base
        if row < 31: return base + 1 + (row - 7)
        if row < 43: return base + 25 + (row - 31)
        if row < 46: return 6 + (row - 43)
        if row < 61: return 9 + (row - 46)
        if row < 76: return 24 + (row - 61)
        if row < 76 + n_view: return 39 + (row - 76)
        return -1
    return f


def _coarse_colmap(row):
    if row < 12: return row
    if row < 24: return -1
    if row < 27: return 54 + (row - 24)
    if row < 30: return 12 + (row - 27)
    if row < 45: return 15 + (row - 30)
    if row < 60: return 30 + (row - 45)
    if row < 69: return 45 + (row - 60)
    return -1


class Net:
    def __init__(self, kind, dims, xrows, zrows, cw, written, colmap, crows):
        self.kind, self.dims, self.xrows, self.zrows, self.cw, self.written, self.crows = kind, dims, xrows, zrows, cw, written, crows
        self.nl, self.hid, self.out_dim, self.in_dim = len(dims) - 1, dims[1], dims[-1], dims[0]
        self.words = self.hid // 64
        self.colmap = [colmap(r) if r < xrows else -1 for r in range(max(xrows, 64))]
        cols = [c for c in self.colmap if c >= 0]
        assert sorted(cols) == list(range(self.in_dim)), kind


NETS = {
    RADIANCE: Net(RADIANCE, [85, 192, 192, 192, 3], 104, 4, 6, 44, _sample_colmap(9), (0, 88, 96)),
    TONEMAP: Net(TONEMAP, [33, 192, 3], 48, 4, 6, 36, lambda r: r if r < 33 else -1, (0,)),
    BRDF: Net(BRDF, [76, 128, 128, 128, 5], 104, 8, 6, 44, _sample_colmap(0), (0, 88, 96)),
    EMIT: Net(EMIT, [76, 128, 128, 128, 3], 104, 4, 6, 44, _sample_colmap(0), (0, 88, 96)),
    COARSE: Net(COARSE, [57, 128, 128, 3], 72, 4, 12, 32, _coarse_colmap, (0, 12)),
}


def rm(t):
    """tile-major [T, rows, 32] -> sample-major [T * 32, rows]"""
    return t.permute(0, 2, 1).reshape(t.shape[0] * 32, t.shape[1])


def tm(t, T):
    return t.reshape(T, 32, t.shape[-1]).permute(0, 2, 1).contiguous()


def x_ref(net, X, crow, mut=None):
    """the net's input in the reference's column order, [T * 32, in_dim], from the X tiles"""
    cmap = list(net.colmap)
    if mut == "sdf_and_first_stencil_row_swapped" and net.kind != TONEMAP and net.kind != COARSE:
        cmap[6], cmap[7] = cmap[7], cmap[6]
    if mut == "color_row0_ignored":
        crow = 0
    rows = [r for r in range(net.xrows) if cmap[r] >= 0]
    src = [r + crow if r < net.cw else r for r in rows]
    out = torch.zeros(X.shape[0] * 32, net.in_dim, dtype=X.dtype)
    out[:, [cmap[r] for r in rows]] = rm(X[:, src])
    return out


# ---- the mask words ---------------------------------------------------------------------------------------------------
def _mask_index(hid, swap_half=False):
    """feature of (word, lane, bit): [W, 64, 32]"""
    W = hid // 64
    f = torch.empty(W, 64, 32, dtype=torch.int64)
    for wd in range(W):
        for h in range(2):
            hh = 1 - h if swap_half else h
            for b in range(32):
                f[wd, 32 * h:32 * h + 32, b] = 32 * (2 * wd + (b >> 4)) + acc_row(b & 15, hh)
    return f


def mask_decode(M, hid):
    """M [T, W, 64] int32 words -> bool [T, hid, 32]"""
    T = M.shape[0]
    f = _mask_index(hid)
    w = M.reshape(T, hid // 64, 64).to(torch.int64) & 0xFFFFFFFF
    b = ((w[..., None] >> torch.arange(32)) & 1).bool()                 # [T, W, 64, 32 bits]
    out = torch.zeros(T, hid, 32, dtype=torch.bool)
    s = (torch.arange(64) % 32)[None, :, None].expand(hid // 64, 64, 32)
    out[:, f.reshape(-1), s.reshape(-1)] = b.reshape(T, -1)
    return out


def mask_encode(m, swap_half=False):
    """bool [T, hid, 32] -> int32 words [T, W, 64]"""
    T, hid = m.shape[0], m.shape[1]
    f = _mask_index(hid, swap_half)
    s = (torch.arange(64) % 32)[None, :, None].expand(hid // 64, 64, 32)
    b = m[:, f.reshape(-1), s.reshape(-1)].reshape(T, hid // 64, 64, 32).to(torch.int64)
    w = (b << torch.arange(32)).sum(-1)
    w = torch.where(w >= 2 ** 31, w - 2 ** 32, w)
    return w.to(I32)


# ---- arithmetic: (value, E) in float64, binary32, split planes ---------------------------------------------------------
def planes(x):
    x1 = x.half().float()
    return x1, (x - x1).half().float()


def lin(x, Ex, W, b, mode, split=False, fx=0.5, mut=None):
    """x [n, in] times W [out, in]^T plus b.  mode 'q': (value, E) in float64; '32': binary32 (torch linear); 'split': binary32 from
    fp16 planes, three products.  fx: the absolute plane error of an element of x, in U (module docstring)."""
    if mode == "q":
        W64, aW = W.double(), W.double().abs()
        v = x @ W64.t()
        mag = x.abs() @ aW.t()
        n = W.shape[1]
        E = Ex @ aW.t() + (n + 1) * mag
        if b is not None:
            v = v + b.double()
            E = E + (n + 1) * b.double().abs()
        if split:
            fxc = fx if torch.is_tensor(fx) else torch.full((x.shape[0], 1), float(fx), dtype=F64)
            E = E + 12 * mag + fxc * aW.sum(1)[None] + x.abs() @ (aW > 0).double().t() / 128      # (a zero weight has no planes' error)
        return v, E
    if mode == "32":
        return F.linear(x, W, b), None
    w1, w2 = planes(W * 64.0)
    x1, x2 = planes(x)
    acc = x1 @ w1.t() + x1 @ w2.t()
    if mut != "split_w1_x2_dropped":
        acc = acc + x2 @ w1.t()
    if b is None:
        return acc * (1.0 / 64.0), None
    bb = b * (1.0 / 64.0) if mut == "split_bias_scaled_twice" else b
    return acc * (1.0 / 64.0) + bb, None


def relu_q(v, E):
    on = v > -DEC_K * U * E
    return v.clamp(min=0), torch.where(on, E, torch.zeros_like(E))


def gain_bound(Ws):
    """G of the header, in float64: the largest running product of the layers' largest column sums of |W| (output layer first, first
    layer excluded), and 1"""
    cum, worst = 1.0, 1.0
    for W in reversed(Ws[1:]):
        cum *= float(W.double().abs().sum(0).max())
        worst = max(worst, cum)
    return worst


def f32(v):
    return float(torch.tensor(v, dtype=F32))


def amax_formula32(zmax, G32):
    """max |dz| x max(1, G / 16), every operation rounded to binary32"""
    fac = max(1.0, f32(f32(G32) * 0.0625))
    return f32(f32(zmax) * fac)


# ---- nets and inputs ----------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def make_net(kind, g, wscale=1.0, plant=True):
    net = NETS[kind]
    Ws = [torch.randn(net.dims[i + 1], net.dims[i], generator=g) / net.dims[i] ** 0.5 * wscale for i in range(net.nl)]
    Bs = [torch.randn(net.dims[i + 1], generator=g) * 0.1 for i in range(net.nl)]
    if plant:                                  # unit 3: pre-activation exactly +0, unit 4: exactly -0 (mask bit 0, H = 0)
        Ws[0][3], Ws[0][4] = 0.0, 0.0
        Bs[0][3], Bs[0][4] = 0.0, -0.0
    return Ws, Bs


def make_X(kind, T, g, scale=1.0):
    net = NETS[kind]
    X = torch.randn(T, net.xrows, 32, generator=g) * scale
    if kind in (RADIANCE, BRDF, EMIT):
        X[:, 7:31] *= 5.0                                               # the stencil features are the large inputs
    X = torch.where(X == 0, torch.full_like(X, 0.5 * scale), X)         # every row, read or not, finite and non-zero
    return X


# =======================================================================================================================
# forward
# =======================================================================================================================
# case: kind(s), tiles of the buffers T, segments (net, t0, t1, save, crow, z name) as the entry point defines them
# resident tiles of a launch: f32 mlp_grid(n) caps at 256 * 2 workgroups of 4 waves, one tile per wave and trip -> 2048 tiles; the
# split launchers cap at 256 * split_occ groups of 4 tiles: 1024 (radiance, occ 1), 2048 (tone mapper, BRDF, emission: occ 2)
FWD_BASE = dict(entry="fwd", kind=RADIANCE, T=5, t0=0, t1=None, save=1, crow=0, xscale=1.0, wscale=1.0, seed=0, t_on=0)
FWD_CASES = {
    "rad_t1": dict(T=1), "rad_t5_crow88": dict(T=5, crow=88, seed=1), "rad_t37_crow96_t0": dict(T=37, t0=3, t1=36, crow=96, seed=2),
    "rad_x40": dict(T=5, xscale=40.0, seed=3), "rad_x1e-3": dict(T=5, xscale=1e-3, seed=4), "rad_w4": dict(T=5, wscale=4.0, seed=5),
    "rad_save0": dict(T=5, save=0, seed=6), "rad_save2": dict(T=5, save=2, t0=1, t1=4, seed=7),
    "tone_t1": dict(kind=TONEMAP, T=1, seed=10), "tone_t5_save2": dict(kind=TONEMAP, T=5, save=2, seed=11),
    "tone_t37_t0": dict(kind=TONEMAP, T=37, t0=2, t1=35, seed=12), "tone_x40": dict(kind=TONEMAP, T=5, xscale=40.0, seed=13),
    "tone_x1e-3_w4": dict(kind=TONEMAP, T=5, xscale=1e-3, wscale=4.0, seed=14),
    "brdf_t1": dict(kind=BRDF, T=1, seed=20), "brdf_t5_crow88_t0": dict(kind=BRDF, T=5, t0=1, t1=4, crow=88, seed=21),
    "brdf_t37_crow96": dict(kind=BRDF, T=37, crow=96, seed=22),
    "emit_t5_crow96": dict(kind=EMIT, T=5, crow=96, seed=30), "emit_t37_t0_crow88": dict(kind=EMIT, T=37, t0=5, t1=37, crow=88, seed=31),
    "emit_t1_save0": dict(kind=EMIT, T=1, save=0, seed=32),
}
FWD_F32_ONLY = {
    "coarse_t1": dict(kind=COARSE, T=1, seed=40), "coarse_t5_crow12_t0": dict(kind=COARSE, T=5, t0=1, t1=5, crow=12, seed=41),
    "coarse_t37_save0": dict(kind=COARSE, T=37, save=0, seed=42), "coarse_t37_crow12_x40": dict(kind=COARSE, T=37, crow=12, xscale=40.0, seed=43),
    "mixed_t0_mid3": dict(entry="mixed", T=8, t0=1, t_on=3, t1=7, crow=88, seed=50),
    "mixed_mid_eq_t0": dict(entry="mixed", T=6, t0=1, t_on=1, t1=5, crow=96, seed=51),
    "mixed_mid_eq_t1": dict(entry="mixed", T=6, t0=1, t_on=5, t1=5, crow=88, seed=52),
    "rad_t2051": dict(T=2051, seed=60, big=True),                       # 2048 resident + 3: second trip, partial
    "tone_t2051": dict(kind=TONEMAP, T=2051, seed=61, big=True),
    "brdf_t2051": dict(kind=BRDF, T=2051, seed=62, big=True),           # the 128-wide kinds' large count, f32 forward
}
FWD_SPLIT_ONLY = {
    "rad_t1027": dict(T=1027, seed=63, big=True),                       # 256 groups of 4 resident + 3 tiles
    "tone_t2051": dict(kind=TONEMAP, T=2051, seed=64, big=True),        # 512 groups of 4 resident + 3 tiles
    "coarse_einval": dict(kind=COARSE, T=2, seed=65),                   # ESR_EINVAL, nothing written
}
FINE_CASES = {"fine_on0": dict(entry="fine", T=5, t_on=0, crow=88, seed=70), "fine_on3": dict(entry="fine", T=7, t_on=3, crow=88, seed=71),
              "fine_on_all": dict(entry="fine", T=5, t_on=5, crow=96, seed=72), "fine_on3_crow0": dict(entry="fine", T=6, t_on=3, crow=0, seed=73)}
FINE_BIG = {"f32": {"fine_t1400_on651": dict(entry="fine", T=1400, t_on=651, crow=88, seed=74, big=True)},      # 1400 + 651 = 2051 work tiles
            "split": {"fine_t700_on327": dict(entry="fine", T=700, t_on=327, crow=88, seed=75, big=True)}}       # 82 + 94 + 82 groups > 256
_CACHE = {}


def fwd_cases(engine):
    c = dict(FWD_CASES)
    c.update(FWD_F32_ONLY if engine == "f32" else FWD_SPLIT_ONLY)
    c.update(FINE_CASES)
    c.update(FINE_BIG[engine])
    return c


def case_fwd(engine, name):
    key = ("fwd", engine, name)
    if key in _CACHE:
        return _CACHE[key]
    cfg = dict(FWD_BASE, **fwd_cases(engine)[name])
    kind, T, g = cfg["kind"], cfg["T"], _gen(100 + cfg["seed"])
    t1 = T if cfg["t1"] is None else cfg["t1"]
    nets = [make_net(kind, g, cfg["wscale"])]
    if cfg["entry"] == "fine":
        nets.append(make_net(kind, g, cfg["wscale"]))                    # 0: the non-emissive net, 1: the emissive net
        segs = [(0, 0, cfg["t_on"], 0, cfg["crow"], "z_off"), (0, cfg["t_on"], T, 1, 0, "z_off"), (1, 0, cfg["t_on"], 1, 0, "z_emo")]
        znames = {"z_off": T, "z_emo": max(cfg["t_on"], 1)}
    elif cfg["entry"] == "mixed":
        segs = [(0, cfg["t0"], cfg["t_on"], 0, cfg["crow"], "z"), (0, cfg["t_on"], t1, 1, 0, "z")]
        znames = {"z": T}
    else:
        segs = [(0, cfg["t0"], t1, cfg["save"], cfg["crow"], "z")]
        znames = {"z": T}
    inp = dict(cfg, op="fwd", engine=engine, name=name, t1=t1, nets=nets, segs=segs, znames=znames, X=make_X(kind, T, g, cfg["xscale"]),
               einval=(engine == "split" and kind == COARSE))
    _CACHE[key] = inp
    return inp


def fwd_chain(net, Ws, Bs, x, mode, mut=None):
    """pre-activations, activations and outputs of one net on x [n, in]; mode 'q' carries E"""
    split = mode == "split" or (mode, mut) == ("q", "SPLIT")
    h, Eh = (x.double(), torch.zeros(x.shape, dtype=F64)) if mode == "q" else (x, None)
    pres, hs = [], []
    for l in range(net.nl):
        b = Bs[l]
        if mut == "bias_dropped_in_one_hidden_layer" and l == net.nl - 2:
            b = torch.zeros_like(b)
        p, Ep = lin(h, Eh, Ws[l], b, mode, split=split, mut=mut)
        if l == net.nl - 1:
            return pres, hs, (p, Ep)
        pres.append((p, Ep))
        h, Eh = relu_q(p, Ep) if mode == "q" else (torch.relu(p), None)
        hs.append((h, Eh))


def _fwd_fill(inp):
    net = NETS[inp["kind"]]
    T = inp["T"]
    out = {n: torch.full((t, net.zrows, 32), H_FILL) for n, t in inp["znames"].items()}
    for l in range(net.nl - 1):
        out[f"H{l}"] = torch.full((T, net.hid, 32), H_FILL)
        out[f"M{l}"] = torch.full((T, net.words, 64), M_FILL, dtype=I32)
    return out


def emu_fwd(inp, mut=None):
    """the entry in binary32: what a correct kernel may return (and, with `mut`, a wrong one)"""
    net, X = NETS[inp["kind"]], inp["X"]
    out = _fwd_fill(inp)
    if inp["einval"]:
        return out
    mode = "32" if inp["engine"] == "f32" else "split"
    last = max(si for si, sg in enumerate(inp["segs"]) if sg[2] > sg[1])
    for si, (ni, a, b, save, crow, zn) in enumerate(inp["segs"]):
        if mut == "t0_ignored" and si == 0:
            a = 0
        if mut == "last_tile_skipped" and si == last:
            b -= 1
        if b <= a:
            continue
        Ws, Bs = inp["nets"][ni]
        pres, hs, (z, _) = fwd_chain(net, Ws, Bs, x_ref(net, X[a:b], crow, mut), mode, mut)
        zt = torch.zeros(b - a, net.zrows, 32)
        zt[:, :net.out_dim] = tm(z, b - a)
        if mut == "last_output_row_of_the_brdf_net_dropped" and net.kind == BRDF:
            zt[:, net.out_dim - 1] = 0.0
        if mut == "z_padding_rows_unwritten":
            zt[:, net.out_dim:] = H_FILL
        out[zn][a:b] = zt
        if mut == "detached_tiles_saved" and save == 0:
            save = 1
        d = 0
        if mut == "second_net_saved_at_first_nets_tile_index" and ni == 1:
            d = min(inp["t_on"], inp["T"] - b)
        for l in range(net.nl - 1):
            if save:
                out[f"M{l}"][a + d:b + d] = mask_encode(tm(pres[l][0] > 0, b - a), swap_half=(mut == "mask_bit_in_the_other_lane_half"))
            if save == 1:
                out[f"H{l}"][a + d:b + d] = tm(hs[l][0], b - a)
    return out


def verify_fwd(inp, got, K):
    net, X, T = NETS[inp["kind"]], inp["X"], inp["T"]
    fill = _fwd_fill(inp)
    val = {k: v.double() if v.dtype == F32 else v.clone() for k, v in fill.items()}
    E = {k: torch.zeros(v.shape, dtype=F64) for k, v in fill.items() if v.dtype == F32}
    zero = {k: torch.zeros(v.shape, dtype=torch.bool) for k, v in fill.items() if v.dtype == F32}
    keep = {k: torch.ones(v.shape, dtype=torch.bool) for k, v in fill.items()}            # values that must keep their prefill bits
    fails, flips, decisions, sub = [], 0, 0, 0
    for ni, a, b, save, crow, zn in ([] if inp["einval"] else inp["segs"]):
        if b <= a:
            continue
        Ws, Bs = inp["nets"][ni]
        pres, hs, (z, Ez) = fwd_chain(net, Ws, Bs, x_ref(net, X[a:b], crow), "q", "SPLIT" if inp["engine"] == "split" else None)
        val[zn][a:b] = 0.0
        val[zn][a:b, :net.out_dim] = tm(z, b - a)
        E[zn][a:b, :net.out_dim] = tm(Ez, b - a)
        zero[zn][a:b, net.out_dim:] = True
        keep[zn][a:b] = False
        sub += int(((z.abs() < TINY) & (z != 0)).sum())
        for l in range(net.nl - 1):
            if save == 1:
                val[f"H{l}"][a:b], E[f"H{l}"][a:b] = tm(hs[l][0], b - a), tm(hs[l][1], b - a)
                keep[f"H{l}"][a:b] = False
                sub += int(((hs[l][0] < TINY) & (hs[l][0] > 0)).sum())
            if save:
                keep[f"M{l}"][a:b] = False
                p, Ep = tm(pres[l][0], b - a), tm(pres[l][1], b - a)
                gotm = mask_decode(got[f"M{l}"][a:b], net.hid)
                diff = gotm != (p > 0)
                bad = diff & ~(p.abs() < DEC_K * U * Ep)
                decisions += p.numel()
                flips += int(diff.sum())
                if bool(bad.any()):
                    i = torch.nonzero(bad)[0].tolist()
                    fails.append(f"M{l}: {int(bad.sum())} mask bits differ outside the band; first at (tile, feature, sample) "
                                 f"{[i[0] + a, i[1], i[2]]}: pre {float(p[tuple(i)])!r}")
    if flips > max(2, decisions // 20000):
        fails.append(f"{flips} of {decisions} mask bits differ: more than max(2, decisions / 20000)")
    r = Ref({k: (val[k], E[k], zero[k]) for k in E})
    r.bits = {k: (keep[k], fill[k]) for k in fill}
    r.note = {"mask flips": flips, "decisions": decisions, "subnormal values": sub}
    worst, f2 = _judge(r, got, K)
    return r, worst, fails + f2


# =======================================================================================================================
# input gradients
# =======================================================================================================================
# resident tiles: f32 mlp_grid(n, occ): occ 2 for radiance and coarse -> 2048, occ 3 for the tone mapper, BRDF, emission -> 3072;
# split: as the split forward (1024 radiance, 2048 the others)
DG_BASE = dict(entry="dgrad", kind=RADIANCE, T=6, t0=0, t1=None, seed=0, t_on=0, null=None, amax0=0.0, wscale=1.0, chained=False)
DG_CASES = {
    "rad_t1": dict(T=1), "rad_t6": dict(T=6, seed=1), "rad_t37_t0": dict(T=37, t0=2, t1=36, seed=2, amax0=0.5),
    "rad_null_dz1": dict(T=6, null=1, seed=3), "rad_w4": dict(T=6, wscale=4.0, seed=4), "rad_amax_prefill_above": dict(T=6, seed=5, amax0=1e9),
    "tone_t1": dict(kind=TONEMAP, T=1, seed=10), "tone_t6_null0": dict(kind=TONEMAP, T=6, null=0, seed=11),
    "tone_t37_t0": dict(kind=TONEMAP, T=37, t0=1, t1=34, seed=12),
    "brdf_t6": dict(kind=BRDF, T=6, seed=20), "brdf_t37_t0": dict(kind=BRDF, T=37, t0=4, t1=37, seed=21), "brdf_t1": dict(kind=BRDF, T=1, seed=22),
    "emit_t6_t0": dict(kind=EMIT, T=6, t0=1, t1=5, seed=30), "emit_t37": dict(kind=EMIT, T=37, seed=31),
    "fine_on0": dict(entry="fine", T=6, t_on=0, seed=40), "fine_on3": dict(entry="fine", T=8, t_on=3, seed=41),
    "fine_on_all": dict(entry="fine", T=6, t_on=6, seed=42),
    "rad_chained": dict(T=5, seed=50, chained=True), "tone_chained": dict(kind=TONEMAP, T=5, seed=51, chained=True),
    "brdf_chained": dict(kind=BRDF, T=5, seed=52, chained=True), "emit_chained": dict(kind=EMIT, T=5, seed=53, chained=True),
}
DG_F32_ONLY = {
    "coarse_t1": dict(kind=COARSE, T=1, seed=60), "coarse_t6_t0": dict(kind=COARSE, T=6, t0=1, t1=6, seed=61), "coarse_t37": dict(kind=COARSE, T=37, seed=62),
    "coarse_chained": dict(kind=COARSE, T=5, seed=63, chained=True),
    "rad_t2051": dict(T=2051, seed=70, big=True), "tone_t3075": dict(kind=TONEMAP, T=3075, seed=71, big=True),
    "emit_t3075": dict(kind=EMIT, T=3075, seed=72, big=True),           # the 128-wide kinds' large count, f32 input gradients
    "fine_t2051_on1000": dict(entry="fine", T=2051, t_on=1000, seed=73, big=True),
}
DG_SPLIT_ONLY = {
    "rad_t1027": dict(T=1027, seed=74, big=True), "tone_t2051": dict(kind=TONEMAP, T=2051, seed=75, big=True),
    "fine_t1027_on500": dict(entry="fine", T=1027, t_on=500, seed=76, big=True),
}
DZ_SCALES = (1.0, 1e-4, 1e-7, 30.0)


def dg_cases(engine):
    c = dict(DG_CASES)
    c.update(DG_F32_ONLY if engine == "f32" else DG_SPLIT_ONLY)
    return c


def make_dz(net, T, g):
    """neighbouring tiles of very different scale; tile 4 (if any) all zero, tile 5 a single 1e-20; the padding rows are 0"""
    dz = torch.randn(T, net.zrows, 32, generator=g)
    for t in range(T):
        dz[t] *= DZ_SCALES[t % 4]
    dz *= 10.0 ** (-3.0 * torch.rand(T, 1, 32, generator=g))             # per-sample magnitudes over three decades
    if T > 4:
        dz[4::64] = 0.0
    if T > 5:
        dz[5::64] = 0.0
        dz[5::64, 1, 7] = 1e-20
    dz[:, net.out_dim:] = 0.0
    return dz


def make_masks(net, T, g):
    """per tile, in turn: random words, all ones, all zeros, one bit per word, a checkerboard across the lane halves"""
    Ms = []
    for l in range(net.nl - 1):
        M = torch.randint(-2 ** 31, 2 ** 31 - 1, (T, net.words, 64), generator=g, dtype=torch.int64).to(I32)
        M[1::5] = -1
        M[2::5] = 0
        one = (1 << torch.randint(0, 31, (net.words, 64), generator=g, dtype=torch.int64)).to(I32)
        M[3::5] = one
        M[4::5, :, :32] = 0x55555555
        M[4::5, :, 32:] = torch.tensor(0xAAAAAAAA - 2 ** 32, dtype=torch.int64).to(I32)
        Ms.append(M)
    return Ms


def case_dgrad(engine, name):
    key = ("dgrad", engine, name)
    if key in _CACHE:
        return _CACHE[key]
    cfg = dict(DG_BASE, **dg_cases(engine)[name])
    kind, T, g = cfg["kind"], cfg["T"], _gen(200 + cfg["seed"])
    net = NETS[kind]
    t1 = T if cfg["t1"] is None else cfg["t1"]
    nets = [make_net(kind, g, cfg["wscale"], plant=False)]
    if cfg["entry"] == "fine":
        nets.append(make_net(kind, g, cfg["wscale"], plant=False))       # 0: the emissive net on [0, t_on), 1: the other on [t_on, T)
        segs = [(0, 0, cfg["t_on"]), (1, cfg["t_on"], T)]
    else:
        segs = [(0, cfg["t0"], t1)]
    inp = dict(cfg, op="dgrad", engine=engine, name=name, t1=t1, nets=nets, segs=segs, dz=make_dz(net, T, g), M=make_masks(net, T, g))
    if cfg["chained"]:
        inp["X"] = make_X(kind, T, g)                                    # the masks are the forward's: filled in by the runner
    _CACHE[key] = inp
    return inp


def dgrad_chain(net, Ws, dz, masks, mode, G=1.0, mut=None):
    """dz [n, zrows], masks [l] -> bool [n, hid]; returns dZ[l] list (index = hidden layer) and dX columns [n, in_dim], with E in 'q'"""
    split = mode == "split" or (mode, mut) == ("q", "SPLIT")
    n = dz.shape[0]
    g = dz[:, :net.out_dim]
    zt = g.abs().reshape(n // 32, -1).amax(1)                            # the tile's largest |dz|
    fx = None
    if mode == "q":
        g, Eg = g.double(), torch.zeros(n, net.out_dim, dtype=F64)
        fx = (G * zt.double() * 2.0 ** -14).repeat_interleave(32)[:, None]        # (1 / 2) 2^-k, 2^-k <= 2 G max|dz| 2^-14
    else:
        Eg = None
    sc = None
    if mode == "split":                                                  # the tile's power of two: G max |dz| 2^k in [2^14, 2^15)
        e = torch.floor(torch.log2(zt.double().clamp_min(1e-300))) + math.ceil(math.log2(G))
        k = torch.where(zt > 0, 14 - e, torch.zeros_like(e)).clamp(-100, 100)
        if mut == "split_tile_scaled_by_the_previous_tiles_power":
            k = torch.cat([k[:1], k[:-1]])
        sc = (2.0 ** k).float().repeat_interleave(32)[:, None]
        g = g * sc
    out = [None] * (net.nl - 1)
    for l in range(net.nl - 1, -1, -1):
        if l < net.nl - 1:
            ml = l
            if mut == "mask_of_layer_l_applied_to_layer_l_minus_1" and l < net.nl - 2:
                ml = l + 1
            m = masks[ml]
            g = torch.where(m, g, torch.zeros_like(g))
            if Eg is not None:
                Eg = torch.where(m, Eg, torch.zeros_like(Eg))
            out[l] = (g if sc is None else g / sc, Eg)
        g, Eg = lin(g, Eg, Ws[l].t(), None, mode, split=split, fx=fx, mut=mut)
    return out, (g if sc is None else g / sc, Eg)


def _dg_fill(inp):
    net, T = NETS[inp["kind"]], inp["T"]
    out = {f"dZ{l}": torch.full((T, net.hid, 32), H_FILL) for l in range(net.nl - 1)}
    out["dX"] = torch.full((T, 64, 32), H_FILL)
    if inp["engine"] == "split":
        out["amax"] = torch.tensor([inp["amax0"]])
    return out


def _dx_rows(net):
    rows = [r for r in range(net.written) if net.colmap[r] >= 0]
    return rows, [net.colmap[r] for r in rows]


def emu_gain32(Ws):
    return f32(gain_bound(Ws))


def emu_dgrad(inp, mut=None):
    net = NETS[inp["kind"]]
    out = _dg_fill(inp)
    mode = "32" if inp["engine"] == "f32" else "split"
    rows, cols = _dx_rows(net)
    for ni, a, b in inp["segs"]:
        if b <= a:
            continue
        Ws = inp["nets"][ni][0]
        G = gain_bound(Ws)
        out[f"G{ni}"] = torch.tensor([emu_gain32(Ws)])
        masks = [rm(mask_decode(M[a:b], net.hid)) for M in inp["M"]]
        dZ, (dx, _) = dgrad_chain(net, Ws, rm(inp["dz"][a:b]), masks, mode, G, mut)
        for l in range(net.nl - 1):
            if inp["null"] != l:
                out[f"dZ{l}"][a:b] = tm(dZ[l][0], b - a)
        blk = torch.zeros(b - a, net.written, 32)
        blk[:, rows] = tm(dx[:, cols], b - a)
        if mut == "dx_rows_from_32_up_unwritten":
            blk[:, 32:] = H_FILL
        out["dX"][a:b, :net.written] = blk
        if mut == "dx_row_beyond_the_documented_range_written":
            out["dX"][a:b, net.written] = 0.0
        if "amax" in out:
            zmax = float(inp["dz"][a:b, :net.out_dim].abs().max())
            out["amax"] = torch.maximum(out["amax"], torch.tensor([amax_formula32(zmax, emu_gain32(Ws))]))
    return out


def verify_dgrad(inp, got, K):
    net, T = NETS[inp["kind"]], inp["T"]
    fill = _dg_fill(inp)
    got = dict(got)
    Gs = {k: float(got.pop(k)) for k in list(got) if k.startswith("G")}
    val = {k: v.double() for k, v in fill.items()}
    E = {k: torch.zeros(v.shape, dtype=F64) for k, v in fill.items()}
    zero = {k: torch.zeros(v.shape, dtype=torch.bool) for k, v in fill.items()}
    keep = {k: torch.ones(v.shape, dtype=torch.bool) for k, v in fill.items()}
    rows, cols = _dx_rows(net)
    fails, sub = [], 0
    amax = f32(inp["amax0"])
    for ni, a, b in inp["segs"]:
        if b <= a:
            continue
        Ws = inp["nets"][ni][0]
        G = gain_bound(Ws)
        masks = [rm(mask_decode(M[a:b], net.hid)) for M in inp["M"]]
        dZ, (dx, Edx) = dgrad_chain(net, Ws, rm(inp["dz"][a:b]), masks, "q", G, "SPLIT" if inp["engine"] == "split" else None)
        for l in range(net.nl - 1):
            if inp["null"] == l:
                continue
            k = f"dZ{l}"
            val[k][a:b], E[k][a:b], keep[k][a:b] = tm(dZ[l][0], b - a), tm(dZ[l][1], b - a), False
            zero[k][a:b] = ~tm(masks[l], b - a)
            sub += int(((dZ[l][0].abs() < TINY) & (dZ[l][0] != 0)).sum())
        val["dX"][a:b, :net.written] = 0.0
        val["dX"][a:b, rows], E["dX"][a:b, rows] = tm(dx[:, cols], b - a), tm(Edx[:, cols], b - a)
        norow = [r for r in range(net.written) if net.colmap[r] < 0]
        zero["dX"][a:b, norow] = True                                     # a written row without a reference column: exactly 0
        keep["dX"][a:b, :net.written] = False
        sub += int(((dx.abs() < TINY) & (dx != 0)).sum())
        if "amax" in fill:
            G32 = Gs[f"G{ni}"]
            nsum = max(W.shape[0] for W in Ws[1:]) + net.nl
            if abs(G32 - G) > nsum * U * G:
                fails.append(f"gain bound of net {ni}: {G32!r}, float64 {G!r}")
            amax = max(amax, amax_formula32(float(inp["dz"][a:b, :net.out_dim].abs().max()), G32))
    r = Ref({k: (val[k], E[k], zero[k]) for k in fill if k != "amax"})
    r.bits = {k: (keep[k], fill[k]) for k in fill if k != "amax"}
    if "amax" in fill:
        r.bits["amax"] = (torch.ones(1, dtype=torch.bool), torch.tensor([amax]))
    r.note = {"subnormal values": sub}
    worst, f2 = _judge(r, got, K)
    return r, worst, fails + f2


# =======================================================================================================================
# weight gradients
# =======================================================================================================================
# a launch has <= 256 workgroups (plan_batch / plan_uni), one tile per workgroup and trip: 261 tiles take a second, partial trip
WG_BASE = dict(jobs=[(RADIANCE, 0, 0, 5)], seed=0, bscale=1.0, ecap=False, pre=0.0, batch=False)
WG_CASES = {
    "rad_t1": dict(jobs=[(RADIANCE, 0, 0, 1)]), "rad_t5_crow88": dict(jobs=[(RADIANCE, 88, 0, 5)], seed=1),
    "rad_t37_t0_crow96": dict(jobs=[(RADIANCE, 96, 3, 37)], seed=2), "tone_t5": dict(jobs=[(TONEMAP, 0, 0, 5)], seed=3),
    "tone_t37_t0": dict(jobs=[(TONEMAP, 0, 2, 37)], seed=4), "brdf_t5_crow96": dict(jobs=[(BRDF, 96, 0, 5)], seed=5),
    "emit_t37_crow88_t0": dict(jobs=[(EMIT, 88, 1, 37)], seed=6), "brdf_t1": dict(jobs=[(BRDF, 0, 0, 1)], seed=7),
    "two_jobs": dict(jobs=[(RADIANCE, 0, 0, 5), (RADIANCE, 0, 2, 9)], seed=8),
    "six_jobs_mixed": dict(jobs=[(RADIANCE, 0, 0, 5), (TONEMAP, 0, 1, 7), (BRDF, 88, 0, 3), (EMIT, 96, 2, 6), (RADIANCE, 96, 0, 1),
                                 (TONEMAP, 0, 0, 37)], seed=9),
    "rad_t5_prefill_0.25": dict(jobs=[(RADIANCE, 0, 0, 5)], seed=12, pre=0.25),      # the prefill dominates: one atomic's rounding at |prefill|
    "emit_t5_prefill_0.25": dict(jobs=[(EMIT, 0, 0, 5)], seed=13, pre=0.25),
    "rad_t261": dict(jobs=[(RADIANCE, 0, 0, 261)], seed=10, big=True), "tone_t261": dict(jobs=[(TONEMAP, 0, 0, 261)], seed=11, big=True),
}
WG_F32_ONLY = {
    "coarse_t5_crow12": dict(jobs=[(COARSE, 12, 0, 5)], seed=20), "coarse_t37_t0": dict(jobs=[(COARSE, 0, 4, 37)], seed=21),
    "five_jobs_with_coarse": dict(jobs=[(COARSE, 0, 0, 5), (RADIANCE, 88, 0, 3), (COARSE, 12, 1, 4), (EMIT, 0, 0, 5), (TONEMAP, 0, 0, 2)], seed=22),
    "coarse_t261": dict(jobs=[(COARSE, 0, 0, 261)], seed=23, big=True),  # the 128-wide kinds' large count, f32 weight gradients
    "rad_t5_one_job_batch": dict(jobs=[(RADIANCE, 88, 1, 5)], seed=25, batch=True),  # esr_mlp_wgrad_batch with one job
    "ecap": dict(jobs=[(RADIANCE, 0, 0, 5)], seed=24, ecap=True),        # a too-small scratch: ESR_ECAP, nothing written
}
WG_SPLIT_ONLY = {"rad_t5_loose": dict(jobs=[(RADIANCE, 0, 0, 5)], seed=30, bscale=8.0), "tone_t37_loose": dict(jobs=[(TONEMAP, 0, 0, 37)], seed=31, bscale=8.0),
                 "six_jobs_loose": dict(jobs=WG_CASES["six_jobs_mixed"]["jobs"], seed=32, bscale=8.0),
                 "emit_t261_loose": dict(jobs=[(EMIT, 0, 0, 261)], seed=33, bscale=8.0, big=True)}


def wg_cases(engine):
    c = dict(WG_CASES)
    c.update(WG_F32_ONLY if engine == "f32" else WG_SPLIT_ONLY)
    return c


def wg_rounds(tiles, n_jobs_in_launch=WG_MAX_JOBS):
    """roundings on the path of an addend (module docstring): the samples a workgroup sums, the slab reduction, the atomics"""
    nwg = max(1, min(tiles, WG_GRID // n_jobs_in_launch))
    return 32 * math.ceil(tiles / nwg) + REDUCE_PG + math.ceil(2 * WG_GRID / REDUCE_PG) + 1


def make_wg_operands(net, T, g):
    """H >= 0 with exact zeros and negative zeros, dZ and dz over four decades per sample"""
    mag = lambda: 1e-2 * 10.0 ** (-4.0 * torch.rand(T, 1, 32, generator=g))
    H = [torch.relu(torch.randn(T, net.hid, 32, generator=g) + 0.4) for _ in range(net.nl - 1)]
    for h in H:
        h[:, 5::7] = torch.where(h[:, 5::7] == 0, torch.full_like(h[:, 5::7], -0.0), h[:, 5::7])
        h[:, ::9] *= 0.05                                               # activations below 0.125: subnormal fp16 residuals
    dZ = [(torch.randn(T, net.hid, 32, generator=g) * mag() * (1.0 + 3.0 * l)).clamp(-0.16, 0.16) for l in range(net.nl - 1)]
    dz = (torch.randn(T, net.zrows, 32, generator=g) * mag()).clamp(-0.01, 0.01)
    dz[:, net.out_dim:] = 0.0
    return H, dZ, dz


def case_wgrad(engine, name):
    key = ("wgrad", engine, name)
    if key in _CACHE:
        return _CACHE[key]
    cfg = dict(WG_BASE, **wg_cases(engine)[name])
    g = _gen(300 + cfg["seed"])
    jobs = []
    for kind, crow, t0, t1 in cfg["jobs"]:
        net = NETS[kind]
        H, dZ, dz = make_wg_operands(net, t1, g)
        X = make_X(kind, t1, g)
        gw0 = [torch.randn(net.dims[l + 1], net.dims[l], generator=g) * 1e-3 + cfg["pre"] for l in range(net.nl)]
        gb0 = [torch.randn(net.dims[l + 1], generator=g) * 1e-2 - cfg["pre"] for l in range(net.nl)]
        jobs.append(dict(kind=kind, crow=crow, t0=t0, t1=t1, X=X, H=H, dZ=dZ, dz=dz, gw0=gw0, gb0=gb0))
    B = max(max(float(j["dz"].abs().max()), max(float(z.abs().max()) for z in j["dZ"]) / 16.0) for j in jobs)
    inp = dict(cfg, op="wgrad", engine=engine, name=name, J=jobs, B=f32(B * cfg["bscale"]))
    _CACHE[key] = inp
    return inp


def _wg_pairs(job, mut=None):
    net = NETS[job["kind"]]
    a, b = job["t0"], job["t1"]
    A = [rm(z[a:b]) for z in job["dZ"]] + [rm(job["dz"][a:b, :net.out_dim])]
    Bm = [x_ref(net, job["X"][a:b], job["crow"], mut)] + [rm(h[a:b]) for h in job["H"]]
    return A, Bm


def split_scale(B):
    """the power of two s with B s in [2^7, 2^8)"""
    if not (B > 0):
        return 1.0
    return 2.0 ** (8 - math.frexp(B)[1])


def emu_wgrad(inp, mut=None):
    out = {}
    for j, job in enumerate(inp["J"]):
        net = NETS[job["kind"]]
        A, Bm = _wg_pairs(job, mut)
        for l in range(net.nl):
            gw, gb = job["gw0"][l].clone(), job["gb0"][l].clone()
            if not inp["ecap"]:
                a = A[l]
                if inp["engine"] == "split":
                    s = split_scale(inp["B"])
                    a1, a2 = planes(a * s)
                    b1, b2 = planes(Bm[l])
                    d = (a1.t() @ b1 + a1.t() @ b2 + (0 if mut == "split_w1_x2_dropped" else a2.t() @ b1)) / s
                else:
                    d = a.t() @ Bm[l]
                if mut == "weight_gradient_transposed_in_one_layer" and l == 1 and d.shape[0] == d.shape[1]:
                    d = d.t()
                gw = d if mut == "gw_overwritten" else gw + d
                ab = a.reshape(-1, 32, a.shape[1])
                if mut == "bias_gradient_over_31_of_32_samples":
                    ab = ab[:, :31]
                gb = gb + ab.sum((0, 1))
            out[f"gw{j}_{l}"], out[f"gb{j}_{l}"] = gw, gb
    return out


def verify_wgrad(inp, got, K):
    ref, bits_ = {}, {}
    split = inp["engine"] == "split"
    for j, job in enumerate(inp["J"]):
        net = NETS[job["kind"]]
        A, Bm = _wg_pairs(job)
        r = wg_rounds(job["t1"] - job["t0"])
        for l in range(net.nl):
            gw0, gb0 = job["gw0"][l].double(), job["gb0"][l].double()
            if inp["ecap"]:
                bits_[f"gw{j}_{l}"] = (torch.ones(gw0.shape, dtype=torch.bool), job["gw0"][l])
                bits_[f"gb{j}_{l}"] = (torch.ones(gb0.shape, dtype=torch.bool), job["gb0"][l])
                ref[f"gw{j}_{l}"], ref[f"gb{j}_{l}"] = (gw0, 0 * gw0, None), (gb0, 0 * gb0, None)
                continue
            a, b = A[l].double(), Bm[l].double()
            d, mag = a.t() @ b, a.abs().t() @ b.abs()
            E = r * mag + gw0.abs() + (gw0 + d).abs()
            if split:
                E = E + 12 * mag + inp["B"] * 2.0 ** -8 * b.abs().sum(0)[None] + 0.5 * a.abs().sum(0)[:, None]
            ref[f"gw{j}_{l}"] = (gw0 + d, E, None)
            sb = a.sum(0)
            ref[f"gb{j}_{l}"] = (gb0 + sb, r * a.abs().sum(0) + gb0.abs() + (gb0 + sb).abs(), None)
    rr = Ref(ref)
    rr.bits, rr.note = bits_, {}
    worst, fails = _judge(rr, got, K)
    return rr, worst, fails


# =======================================================================================================================
# the tone mapper's weight gradient from its inputs
# =======================================================================================================================
# resident tiles: two per workgroup, grid <= 256 (f32) / 512 (split): 512 / 1024 -> 1027 takes a second, partial trip in both
# small cases: N(0, 1) inputs, redrawn with the next seed until no hidden pre-activation lies within DEC_K U absref of 0 (the seed
# that passed is recorded here; case_tone asserts the margin); large cases: signs fixed by construction
TONE_CASES = {"t1": dict(T=1, t0=0, seed0=0, seed=1), "t2": dict(T=2, t0=0, seed0=0, seed=2), "t5_t0": dict(T=6, t0=1, seed0=0, seed=63),
              "t37_fixed_signs_t0": dict(T=37, t0=3, fixed=True, seed0=5, seed=5),
              "t1027_fixed_signs": dict(T=1027, t0=0, fixed=True, seed0=6, seed=6, big=True)}
TONE_MAX_REDRAWS = 64


def tone_rounds(tiles, engine):
    pairs = 2 * min((tiles + 1) // 2, 256 if engine == "f32" else 512)
    return 32 * math.ceil(tiles / pairs) + REDUCE_PG + math.ceil(pairs / REDUCE_PG) + 1


def _tone_draw(T, seed, fixed):
    g = _gen(400 + seed)
    W0 = torch.randn(192, 33, generator=g) / 33 ** 0.5
    b0 = torch.randn(192, generator=g) * 0.1
    W1 = torch.randn(3, 192, generator=g) / 192 ** 0.5
    Xt = torch.randn(T, 48, 32, generator=g)
    if fixed:                                                           # |Xt| <= 1, L1(W0 row) <= 3, b0 = +-4: every sign fixed
        Xt = Xt.clamp(-1, 1)
        W0 = W0 * (3.0 / W0.abs().sum(1, keepdim=True)).clamp(max=1.0) * 0.999
        b0 = torch.where(torch.arange(192) % 2 == 0, torch.tensor(4.0), torch.tensor(-4.0))
    W0[5], b0[5] = 0.0, 0.0                                             # a unit whose pre-activation is exactly 0: off, E = 0
    Xt = torch.where(Xt == 0, torch.full_like(Xt, 0.5), Xt)
    dzt = torch.randn(T, 4, 32, generator=g) * 1e-2 * 10.0 ** (-3.0 * torch.rand(T, 1, 32, generator=g))
    dzt = dzt.clamp(-0.01, 0.01)
    dzt[:, 3] = 0.0
    return W0, b0, W1, Xt, dzt


def _tone_margin_ok(W0, b0, Xt, t0, split):
    x = rm(Xt[t0:, :33]).double()
    p, E = lin(x, torch.zeros_like(x), W0, b0, "q", split=split)
    return bool(((p.abs() >= DEC_K * U * E) | ((p == 0) & (E == 0))).all())


def tone_first_seed(name):
    """the first seed from seed0 on whose draw leaves no decision in doubt (what TONE_CASES records as `seed`)"""
    cfg = TONE_CASES[name]
    for redraw in range(TONE_MAX_REDRAWS + 1):
        W0, b0, _, Xt, _ = _tone_draw(cfg["T"], cfg["seed0"] + redraw, cfg.get("fixed", False))
        if _tone_margin_ok(W0, b0, Xt, cfg["t0"], True):
            return cfg["seed0"] + redraw
    raise AssertionError(f"{name}: no draw without a decision in doubt in {TONE_MAX_REDRAWS} redraws")


def case_tone(engine, name):
    key = ("tone", engine, name)
    if key in _CACHE:
        return _CACHE[key]
    cfg = dict(TONE_CASES[name])
    T, t0, fixed = cfg["T"], cfg["t0"], cfg.get("fixed", False)
    seed = cfg["seed"]
    W0, b0, W1, Xt, dzt = _tone_draw(T, seed, fixed)
    assert _tone_margin_ok(W0, b0, Xt, t0, True), f"{name}: a decision in doubt"      # (the wider band of the two engines, for both)
    g = _gen(500 + seed)
    pre = {"gw0": torch.randn(192, 33, generator=g) * 1e-3, "gb0": torch.randn(192, generator=g) * 1e-2,
           "gw1": torch.randn(3, 192, generator=g) * 1e-3, "gb1": torch.randn(3, generator=g) * 1e-2}
    G = max(1.0, float(W1.double().abs().sum(0).max()))
    B = f32(float(dzt.abs().max()) * max(1.0, G / 16.0))
    inp = dict(op="tone", engine=engine, name=name, T=T, t0=t0, W0=W0, b0=b0, W1=W1, Xt=Xt, dzt=dzt, pre=pre, B=B, big=cfg.get("big", False))
    _CACHE[key] = inp
    return inp


def _tone_any(inp, mode, mut=None):
    t0 = inp["t0"]
    x, dz = rm(inp["Xt"][t0:, :33]), rm(inp["dzt"][t0:, :3])
    if mode == "q":
        split = inp["engine"] == "split"
        x, dz = x.double(), dz.double()
        p, Ep = lin(x, torch.zeros_like(x), inp["W0"], inp["b0"], "q", split=split)
        h, Eh = relu_q(p, Ep)
        on = p > 0
        fxs = inp["B"] * 2.0 ** -8
        d, Ed = lin(dz, torch.zeros_like(dz), inp["W1"].t(), None, "q", split=split, fx=fxs)
        d, Ed = torch.where(on, d, 0 * d), torch.where(on, Ed, 0 * Ed)
        return x, dz, (h, Eh), (d, Ed)
    m = "32" if inp["engine"] == "f32" else "split"
    p, _ = lin(x, None, inp["W0"], inp["b0"], m, mut=mut)
    on = (p >= 0) if mut == "tone_hidden_mask_taken_as_ge_0" else (p > 0)
    h = torch.where(p > 0, p, torch.zeros_like(p))
    if m == "split":
        s = split_scale(inp["B"])
        d = lin(dz * s, None, inp["W1"].t(), None, m, mut=mut)[0] / s
    else:
        d = lin(dz, None, inp["W1"].t(), None, m)[0]
    return x, dz, (h, None), (torch.where(on, d, torch.zeros_like(d)), None)


def emu_tone(inp, mut=None):
    x, dz, (h, _), (d, _) = _tone_any(inp, "32", mut)
    pre = inp["pre"]
    if inp["engine"] == "split":
        s = split_scale(inp["B"])

        def prod(a, b):
            a1, a2 = planes(a * s)
            b1, b2 = planes(b)
            return (a1.t() @ b1 + a1.t() @ b2 + (0 if mut == "split_w1_x2_dropped" else a2.t() @ b1)) / s
    else:
        prod = lambda a, b: a.t() @ b
    d31 = d.reshape(-1, 32, 192)[:, :31] if mut == "bias_gradient_over_31_of_32_samples" else d.reshape(-1, 32, 192)
    g0, g1 = prod(d, x), prod(dz, h)
    if mut == "gw_overwritten":
        return {"gw0": g0, "gb0": pre["gb0"] + d31.sum((0, 1)), "gw1": g1, "gb1": pre["gb1"] + dz.sum(0)}
    return {"gw0": pre["gw0"] + g0, "gb0": pre["gb0"] + d31.sum((0, 1)), "gw1": pre["gw1"] + g1, "gb1": pre["gb1"] + dz.sum(0)}


def verify_tone(inp, got, K):
    x, dz, (h, Eh), (d, Ed) = _tone_any(inp, "q")
    r = tone_rounds(inp["T"] - inp["t0"], inp["engine"])
    split = inp["engine"] == "split"
    pre = {k: v.double() for k, v in inp["pre"].items()}

    def acc(p0, a, Ea, b, Eb):
        v, mag = a.t() @ b, a.abs().t() @ b.abs()
        E = Ea.t() @ b.abs() + a.abs().t() @ Eb + r * mag + p0.abs() + (p0 + v).abs()
        if split:
            E = E + 12 * mag + inp["B"] * 2.0 ** -8 * b.abs().sum(0)[None] + 0.5 * a.abs().sum(0)[:, None]
        return (p0 + v, E, None)
    z = lambda t: torch.zeros_like(t)
    ref = {"gw0": acc(pre["gw0"], d, Ed, x, z(x)), "gw1": acc(pre["gw1"], dz, z(dz), h, Eh),
           "gb0": (pre["gb0"] + d.sum(0), Ed.sum(0) + r * d.abs().sum(0) + pre["gb0"].abs() + (pre["gb0"] + d.sum(0)).abs(), None),
           "gb1": (pre["gb1"] + dz.sum(0), r * dz.abs().sum(0) + pre["gb1"].abs() + (pre["gb1"] + dz.sum(0)).abs(), None)}
    rr = Ref(ref)
    rr.bits, rr.note = {}, {}
    worst, fails = _judge(rr, got, K)
    return rr, worst, fails


# =======================================================================================================================
# absmax
# =======================================================================================================================
ABS_CASES = {"n1": (1, 0.0), "n3": (3, 0.0), "n4": (4, 0.0), "n1027_prefill_below": (1027, 1e-3), "n1027_prefill_above": (1027, 1e6),
             "n262147": (262147, 0.0), "all_zero": (37, 0.0), "negative_zero_and_largest_negative": (129, 0.0)}


def case_absmax(engine, name):
    n, pre = ABS_CASES[name]
    g = _gen(600 + n)
    x = torch.randn(n, generator=g) * 10.0 ** (-3.0 * torch.rand(n, generator=g))
    if name == "all_zero":
        x = torch.zeros(n)
        x[::2] = -0.0
    if name.startswith("negative"):
        x[-1] = -77.0
        x[0] = -0.0
    return dict(op="absmax", engine=engine, name=name, x=x, pre=pre, big=False)


def emu_absmax(inp, mut=None):
    x = inp["x"][:-1] if mut == "scalar_tail_skipped" and inp["x"].numel() % 4 else inp["x"]
    m = float(x.abs().max()) if x.numel() else 0.0
    return {"out": torch.tensor([m if mut == "gw_overwritten" else max(f32(inp["pre"]), m)])}


def verify_absmax(inp, got, K):
    want = torch.tensor([max(f32(inp["pre"]), float(inp["x"].abs().max()))])
    r = Ref({"out": (want.double(), torch.zeros(1, dtype=F64), None)})
    r.bits, r.note = {"out": (torch.ones(1, dtype=torch.bool), want)}, {}
    worst, fails = _judge(r, got, K)
    return r, worst, fails


# =======================================================================================================================
# the comparison, the operations, their families and the mutants
# =======================================================================================================================
def _judge(r, got, K):
    """shade_ref64.compare plus the bit expectations of Ref.bits"""
    worst, fails = compare(Ref({k: v for k, v in r.out.items()}), {k: got[k] for k in r.out}, K)
    for name, (mask, want) in r.bits.items():
        g = got[name].detach().cpu().reshape(want.shape).to(want.dtype)
        bad = (bits(g) != bits(want)) & mask
        if bool(bad.any()):
            i = int(torch.nonzero(bad.reshape(-1))[0])
            fails.append(f"{name}: {int(bad.sum())} of {int(mask.sum())} values that must keep given bits differ; first at flat index {i}: "
                         f"got {g.reshape(-1)[i].item()!r}, want {want.reshape(-1)[i].item()!r}")
    return worst, fails


def _ops(engine):
    e = engine
    return {
        f"fwd_{e}": (lambda n: case_fwd(e, n), list(fwd_cases(e)), verify_fwd, emu_fwd, f"fwd_{e}"),
        f"dgrad_{e}": (lambda n: case_dgrad(e, n), list(dg_cases(e)), verify_dgrad, emu_dgrad, f"dgrad_{e}"),
        f"wgrad_{e}": (lambda n: case_wgrad(e, n), list(wg_cases(e)), verify_wgrad, emu_wgrad, f"wgrad_{e}"),
        f"tone_wgrad_{e}": (lambda n: case_tone(e, n), list(TONE_CASES), verify_tone, emu_tone, "tone_wgrad"),
    }


# op -> (case builder, case names, verify(inp, got, K) -> (ref, worst, fails), binary32 emulation, family)
OPS = {**_ops("f32"), **_ops("split"),
       "absmax": (lambda n: case_absmax("f32", n), list(ABS_CASES), verify_absmax, emu_absmax, "absmax")}
ENTRY_POINTS = {
    "fwd_f32": ("esr_mlp_fwd", "esr_mlp_fwd_mixed", "esr_mlp_fwd_fine"), "fwd_split": ("esr_mlp_fwd_split", "esr_mlp_fwd_fine_split"),
    "dgrad_f32": ("esr_mlp_dgrad", "esr_mlp_dgrad_fine"), "dgrad_split": ("esr_mlp_dgrad_split", "esr_mlp_dgrad_fine_split"),
    "wgrad_f32": ("esr_mlp_wgrad", "esr_mlp_wgrad_batch"), "wgrad_split": ("esr_mlp_wgrad_batch",),
    "tone_wgrad_f32": ("esr_tone_wgrad_recompute",), "tone_wgrad_split": ("esr_tone_wgrad_recompute_split",), "absmax": ("esr_absmax",),
}


def build(op, case):
    return OPS[op][0](case)


def all_cases():
    return [(op, case) for op, spec in OPS.items() for case in spec[1]]


def _case_cfg(op, case):
    e = "split" if op.endswith("split") else "f32"
    if op.startswith("fwd"):
        return fwd_cases(e)[case]
    if op.startswith("dgrad"):
        return dg_cases(e)[case]
    if op.startswith("wgrad"):
        return wg_cases(e)[case]
    if op.startswith("tone"):
        return TONE_CASES[case]
    return {}


def is_big(op, case):
    return bool(_case_cfg(op, case).get("big", False))


def verify(op, inp, got, K):
    return OPS[op][2](inp, dict(got), K)


# K per family, for both test files: the next power of two (possibly below 1) at or above twice the worst ratio
# |gpu - ref| / (U absref) measured on the MI355X over every case of test_gpu_mlp_ref64.py (printed under -s); the factor two leaves
# room for the order of the float atomics of the weight-gradient reductions.  Beside each: the measured worst, and the binary32
# emulation's on the same cases.
K_FAMILY = {
    "fwd_f32": 1,        # measured worst 0.276 (esr_mlp_fwd, tone mapper, inputs x 1e-3 and weights x 4; emulation 0.168)
    "fwd_split": 1,      # 0.438 (esr_mlp_fwd_split, the same case; emulation 0.438: the planes' quantisation is deterministic)
    "dgrad_f32": 2,      # 0.677 (esr_mlp_dgrad: the three-term products of dZ[last]; emulation 0.677)
    "dgrad_split": 2,    # 0.752 (esr_mlp_dgrad_split, weights x 4; emulation 0.752)
    "wgrad_f32": 1,      # 0.498 (esr_mlp_wgrad on a prefill of 0.25: the one rounding of the float atomic; emulation 0.340)
    "wgrad_split": 2,    # 0.507 (esr_mlp_wgrad_batch with amax, chained radiance case; emulation 0.327)
    "tone_wgrad": 0.5,   # 0.239 (esr_tone_wgrad_recompute, one tile; the split twin 0.209; emulation 0.239)
    "absmax": 1,         # exact (a bit check)
}

_FWD, _DG, _WG = ["fwd_f32", "fwd_split"], ["dgrad_f32", "dgrad_split"], ["wgrad_f32", "wgrad_split"]
_TONE = ["tone_wgrad_f32", "tone_wgrad_split"]
# mutant of the emulation -> the ops it applies to; each must break the bound (or a bit expectation, or the mask rule) on at least one
# small case of each of those ops
MUTANTS = {
    "color_row0_ignored": _FWD + _WG,
    "sdf_and_first_stencil_row_swapped": _FWD + _WG,
    "bias_dropped_in_one_hidden_layer": _FWD,
    "last_output_row_of_the_brdf_net_dropped": _FWD,
    "z_padding_rows_unwritten": _FWD,
    "last_tile_skipped": _FWD,
    "t0_ignored": _FWD,
    "detached_tiles_saved": _FWD,
    "second_net_saved_at_first_nets_tile_index": _FWD,
    "mask_bit_in_the_other_lane_half": _FWD,
    "mask_of_layer_l_applied_to_layer_l_minus_1": _DG,
    "dx_rows_from_32_up_unwritten": _DG,
    "dx_row_beyond_the_documented_range_written": _DG,
    "weight_gradient_transposed_in_one_layer": _WG,
    "bias_gradient_over_31_of_32_samples": _WG + _TONE,
    "gw_overwritten": _WG + _TONE + ["absmax"],
    "split_w1_x2_dropped": ["fwd_split", "dgrad_split", "wgrad_split", "tone_wgrad_split"],
    "split_bias_scaled_twice": ["fwd_split"],
    "split_tile_scaled_by_the_previous_tiles_power": ["dgrad_split"],
    "tone_hidden_mask_taken_as_ge_0": _TONE,
    "scalar_tail_skipped": ["absmax"],
}
