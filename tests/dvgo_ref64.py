"""Float64 restatement of the DVGO pre-stage kernels (csrc/dvgo.hip: esr_dvgo_fwd, esr_dvgo_eval, esr_dvgo_bwd, esr_dvgo_count,
esr_dvgo_count_add) at the C ABI, with a binary32 emulation that follows the kernel's structure (runs, the 64-lane scans in the
kernel's order, the per-lane cell accumulator) and the input builders shared by tests/test_dvgo_ref64_host.py and
tests/test_gpu_dvgo_ref64.py; never imported by the product path.

Exact part.  The kernel header promises separately rounded binary32 operations for the sample point p_i = o + d (t_min + (step_scale
(i + u)) / |d|), for esr_world_to_index and for the out-of-box test.  They are replayed in binary32 (dvgo_ref.sample, then the index
expression as written): the point, the continuous index, floor(idx), the one-dimensional weights (idx - i0, (i0 + 1) - idx) and the
masked flag are the kernel's bit for bit.  The cell of a sample is therefore no banded decision and nothing is exempted for it.
Everything after the index is `Q` arithmetic in float64 (lts_ref64's docstring has the algebra), |got - value| <= K U absref + FLOOR:
  corner weight  (wz wy) wx, two roundings (none where the factors are exact 0 / 1: a sample on a node)
  fetch          8 terms, sum rule with r = 8
  alpha          x = d + shift; softplus (6 sp); t = -sp interval; e = exp t (2 ulp); alpha = 1 - e; 0 exactly on masked samples
  p              max(1 - alpha, 1e-10): one more rounding; under the clamp the binary32 constant, exact
  T_j            prod_{i<j} p_i.  On the path of sample j the kernel rounds at most K times in its run product (K = ceil(S / 64)), 6
                 times in the scan and K times in the run again:  E = T_j (sum_{i<j} E(p_i) / p_i + 2 K + 6), 0 for j = 0.
                 T below 2^-126 is held by FLOOR alone (1e-30 against a subnormal's 1.4e-45).
  sigmoid        1 / (1 + exp(-x)) by Q
  ray sums       rgb, off_rgb, emo_rgb, depth: sum rule with r = K + 6 (the run and the six shuffle levels) over Q products;
                 on_rgb = off_rgb + emo_rgb, disp = 1 / (depth + T_S far), |o - p| by Q (three products, two sums, a square root)
  backward       the inputs alpha, alphainv_cum and raw_rgb are the forward's own binary32 outputs and enter exactly.
                 dw_j = g_w + g_rgb . raw_j;  g_j = g_cum_j + dw_j alpha_j;  R_{j-1} = g_j + p_j R_j from R_{S-1} = g_cum_S;
                 dalpha_j = dw_j T_j - [not clamped] T_j R_j;  the density cell gets dalpha_j e interval softplus'(x) w_corner (masked:
                 0), the colour cells (g_raw + g_rgb alpha_j T_j) s (1 - s) w_corner at EVERY sample (the emissive grid on mode-1 rays).
                 R carries the propagated input errors plus 3 (2 K + 7) roundings on its magnitude sum |g_i| prod p (the kernel composes
                 one affine map per run: K fused steps, six scan levels of a product and a sum each, one more, K again).
                 Per cell: absref = sum E_i + r M + n (|init| + M), M = sum |contribution|, r = the most samples of one run that fall
                 into the cell (register accumulation), n = the non-zero contributions (an upper bound of the float atomics, each at a
                 magnitude <= |init| + M) -- the per-cell rule of the feature-scatter and expgrad checks.  A cell whose contributions
                 and initial value are all exact integers below 2^24 has absref 0 (every partial sum is representable).
                 The value is the explicit adjoint above; the host test asserts it equals float64 autograd of the forward.
                 Before it uses them, verify_bwd holds alpha, alphainv_cum and raw_rgb to 16 K U absref of the forward's restatement: a
                 sanity gate against a garbage input, not a bound (the forward is held to K by its own operation).
  view count     sum: the same per-cell rule with one run per ray (one lane walks all S samples), weight 1, no jitter, no mask.
Decisions with a band.  (1) the clamp 1 - a >= 1e-10: in binary32 1 - a is 0 or >= 2^-24, so the decision is alpha == 1.0f, i.e.
e <= 2^-25.  `force` takes it from the kernel's own alpha output; a forced branch that differs from the float64 one must have its
float64 e within DEC_K U E_e of 2^-25 (asserted).  T, the weights and the colour gradients are continuous across it, grad_density at
that sample is not.  (2) sum > 1 of esr_dvgo_count_add: count is held bit for bit to count0 + (the kernel's own sum > 1); a voxel where
that differs from the float64 sum's decision must have its float64 sum within DEC_K U absref of 1.  x > 20 in softplus is continuous
to 2e-9 relative and has no band.  The exempt share of a case stays <= FLIP_CAP.
Bit expectations (Ref.bits): alpha == 0 on masked samples; a ray that misses the box has alpha 0, weights 0, alphainv_cum 1 and
white_bg 1; raw_rgb of a sample with no corner on the grid is sigmoid(0) (twice that on a mode-1 ray); gradient cells without a
non-zero contribution keep their planted bits; a backward with all four upstream pointers NULL leaves the three buffers untouched."""
from __future__ import annotations

from types import SimpleNamespace

import torch

import dvgo_ref
from grid_ref64 import _judge, _ref, bits, same_bits       # noqa: F401  (same_bits: the GPU test's)
from lts_ref64 import FLIP_CAP, Q, lift, xexp, xsoftplus, xspgrad, xsqrt, xstack, xsum, xwhere
from shade_ref64 import DEC_K, FLOOR, U, Ref, compare      # noqa: F401

F32, F64, I32 = torch.float32, torch.float64, torch.int32
WAVE, WAVES, TRIP = 64, 4, 256 * 64                         # lanes, waves per workgroup, the workgroup cap of a launch
COUNT_BLOCK = 256
E_CLAMP = 2.0 ** -25


def f32(v):
    return float(torch.tensor(v, dtype=F32))


P_MIN = f32(1e-10)
P_MIN32 = torch.tensor(1e-10, dtype=F32)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def fma32(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def sqrt32(a):
    return a.double().sqrt().float()


def run_len(S):
    K = (S + WAVE - 1) // WAVE
    return K, (S + K - 1) // K                              # samples per lane, lanes that own a sample


# =======================================================================================================================
# sampling, index and corners: binary32, bit for bit
# =======================================================================================================================
def _model(inp):
    return SimpleNamespace(xyz_min=inp["lo"], xyz_max=inp["hi"], near=inp["near"], far=inp["far"], stepsize=1.0,
                           voxel_size=torch.tensor(inp["step_scale"], dtype=F32))


def ray_norm(rays_d):
    return rays_d.norm(dim=-1, keepdim=True).reshape(-1).contiguous()


def sampling(inp, jitter=True):
    """the binary32 replay of one ray set -> namespace (pts, masked, miss, t, i0, w1 [N,S,3,2], cell, inb [N,S,8])"""
    o, d, S, dims = inp["rays_o"], inp["rays_d"], inp["S"], inp["dims"]
    lo, hi = inp["lo"], inp["hi"]
    j = inp.get("jitter") if jitter else None
    pts, masked = dvgo_ref.sample(_model(inp), o, d, S, j)
    v = torch.where(d == 0, torch.full_like(d, 1e-6), d)
    ta, tb = (hi - o) / v, (lo - o) / v
    tmin = torch.minimum(ta, tb).amax(-1).clamp(min=inp["near"], max=inp["far"])
    tmax = torch.maximum(ta, tb).amin(-1).clamp(min=inp["near"], max=inp["far"])
    i = torch.arange(S, dtype=F32)[None].expand(o.shape[0], -1)
    if j is not None:
        i = i + j.reshape(-1, 1)
    t = tmin[:, None] + (torch.tensor(inp["step_scale"], dtype=F32) * i) / ray_norm(d)[:, None]
    c = corners(pts, lo, hi, dims)
    return SimpleNamespace(pts=pts, masked=masked, miss=tmax <= tmin, t=t, idx=c.idx, i0=c.i0, w1=c.w1, cell=c.cell, inb=c.inb)


def corners(pts, lo, hi, dims):
    """esr_world_to_index and esr_tri_setup of binary32 points [..., 3], in binary32: the continuous index, its floor, the
    one-dimensional weights w1 [..., 3, 2] = ((i0 + 1) - idx, idx - i0), and per corner (cx 4 + cy 2 + cz) the flat cell and whether it is
    on the grid"""
    top = torch.tensor([x - 1.0 for x in dims], dtype=F32)
    u = (pts - lo) / (hi - lo)
    idx = (((u * 2.0 - 1.0) + 1.0) / 2.0) * top
    fl = torch.floor(idx)
    i0 = fl.long()
    w1 = torch.stack([(fl + 1.0) - idx, idx - fl], -1)
    cells, inbs = [], []
    for k in range(8):
        c = (k >> 2, (k >> 1) & 1, k & 1)
        ii = [i0[..., a] + c[a] for a in range(3)]
        inb = torch.ones_like(ii[0], dtype=torch.bool)
        for a in range(3):
            inb &= (ii[a] >= 0) & (ii[a] < dims[a])
        cl = [ii[a].clamp(0, dims[a] - 1) for a in range(3)]
        cells.append((cl[0] * dims[1] + cl[1]) * dims[2] + cl[2])
        inbs.append(inb)
    return SimpleNamespace(idx=idx, i0=i0, w1=w1, cell=torch.stack(cells, -1), inb=torch.stack(inbs, -1))


def corner_w(G, mode):
    """[N,S,8] corner weights (wz wy) wx in the number system of `mode`, corner = cx 4 + cy 2 + cz"""
    out = []
    for k in range(8):
        cx, cy, cz = k >> 2, (k >> 1) & 1, k & 1
        out.append((lift(G.w1[..., 2, cz], mode) * lift(G.w1[..., 1, cy], mode)) * lift(G.w1[..., 0, cx], mode))
    return xstack(out, -1)


def fetch(grid, G, W, mode):
    """zero-padded trilinear fetch of grid [C, cells] -> [C,N,S]"""
    v = grid[:, G.cell] * G.inb.to(grid.dtype)
    if mode == "q":
        return xsum(Q(v) * Q(W.v[None], W.E[None]), -1, 8)
    acc = torch.zeros(v.shape[:-1], dtype=F32)
    for k in range(8):
        acc = fma32(v[..., k], W[..., k], acc)
    return acc


def xsigmoid(x):
    if isinstance(x, Q):
        return 1.0 / (1.0 + xexp(-x))
    return 1.0 / (1.0 + torch.exp(-x))


def qz(shape):
    return Q(torch.zeros(shape, dtype=F64))


def qx(t):
    """a binary32 (or None -> nothing) input as an exact Q"""
    return Q(t.double())


# =======================================================================================================================
# the float64 restatement
# =======================================================================================================================
def _grids64(inp, grids=None):
    if grids is not None:
        return grids
    return {k: inp[k].double().reshape(inp[k].shape[0] if k != "density" else 1, -1) for k in ("density", "off_color", "emo_color")}


def em_on(inp):
    n = inp["rays_o"].shape[0]
    if inp.get("em_modes") is not None:
        return inp["em_modes"] == 1
    return torch.full((n,), bool(inp["em_all"]))


def alpha_q(inp, G, W, grids):
    d = fetch(grids["density"], G, W, "q")[0]
    x = d + inp["act_shift"]
    e = xexp((-xsoftplus(x)) * inp["interval"])
    return x, e


def fwd_q(inp, G, force=None, grids=None, evaluate=False):
    """every quantity of the two forwards as Q [N,S..]; `force`: the clamp decisions (bool [N,S]) to use instead of the float64 ones"""
    S = inp["S"]
    K, _ = run_len(S)
    g = _grids64(inp, grids)
    W = corner_w(G, "q")
    x, e = alpha_q(inp, G, W, g)
    a = xwhere(G.masked, qz(G.masked.shape), 1.0 - e)
    clamp64 = (e.v.detach() <= E_CLAMP) & ~G.masked
    clamped = clamp64 if force is None else (force & ~G.masked)
    p = xwhere(clamped, Q(torch.full(clamped.shape, P_MIN, dtype=F64)), 1.0 - a)
    Tv = torch.cat([torch.ones_like(p.v[:, :1]), torch.cumprod(p.v, 1)], 1)
    rel = torch.cumsum(p.E / p.v.detach(), 1)
    rnd = torch.full((S + 1,), 2.0 * K + 6)
    rnd[0] = 0.0
    TE = Tv.detach() * (torch.cat([torch.zeros_like(rel[:, :1]), rel], 1) + rnd[None])
    T = Q(Tv, TE)
    w = a * T[:, :S]
    so = xsigmoid(fetch(g["off_color"], G, W, "q"))
    se = xsigmoid(fetch(g["emo_color"], G, W, "q"))
    so, se = Q(so.v.permute(1, 2, 0), so.E.permute(1, 2, 0)), Q(se.v.permute(1, 2, 0), se.E.permute(1, 2, 0))
    r = SimpleNamespace(e=e, a=a, clamp64=clamp64, clamped=clamped, p=p, T=T, w=w, so=so, se=se, W=W, x=x)
    w3 = w[..., None]
    if evaluate:
        r.off_rgb, r.emo_rgb = xsum(w3 * so, 1, K + 6), xsum(w3 * se, 1, K + 6)
        r.on_rgb = r.off_rgb + r.emo_rgb
        dd = qx(inp["rays_o"])[:, None, :] - qx(G.pts)
        sq = dd * dd
        dist = xsqrt((sq[..., 0] + sq[..., 1]) + sq[..., 2])
        r.depth = xsum(w * dist, 1, K + 6)
        r.disp = 1.0 / (r.depth + T[:, S] * inp["far"])
    else:
        on = em_on(inp)[:, None, None]
        r.raw = xwhere(on, se + so, so)
        r.rgb = xsum(w3 * r.raw, 1, K + 6)
    return r


def _o(q, zero=None):
    return (q.v.detach(), q.E, zero)


def clamp_legit(r, fails):
    """the forced clamp decisions that differ from the float64 ones: each strictly inside the band of 2^-25"""
    flip = (r.clamped != r.clamp64)
    e = r.e.v.detach()
    bad = flip & ~((e - E_CLAMP).abs() < DEC_K * U * r.e.E)
    if bool(bad.any()):
        i = int(torch.nonzero(bad.reshape(-1))[0])
        fails.append(f"clamp: {int(bad.sum())} forced decisions lie outside the band of 2^-25; first at flat index {i}: e = "
                     f"{float(e.reshape(-1)[i]):.9g}, E = {float(r.e.E.reshape(-1)[i]):.3g}")
    return int(flip.sum())


def _finish(r, ref, got, K, flips, n_values, fails0):
    ref.flips = {"clamp": flips}
    ref.share = flips / max(1, n_values)
    worst, fails = _judge(ref, got, K)
    fails = fails0 + fails
    if ref.share > FLIP_CAP:
        fails.append(f"the exempt share {ref.share:.3g} exceeds FLIP_CAP")
    return ref, worst, fails


def _expand(inp, t):
    """a per-ray tensor of the distinct rays -> of every ray (the second-trip cases repeat a small ray set)"""
    return t if inp.get("rep") is None else t[inp["rep"]]


def _fwd_bits(inp, G, r, evaluate):
    miss = G.miss
    one = lambda *s: torch.ones(*s, dtype=F32)
    N, S = G.masked.shape
    b = {"alpha": (G.masked, torch.zeros(N, S))}
    m1 = miss[:, None]
    if evaluate:
        b["white_bg"] = (miss, one(N))
    else:
        b["alphainv_cum"] = (m1.expand(N, S + 1), one(N, S + 1))
        b["weights"] = (m1.expand(N, S), torch.zeros(N, S))
        off = ~G.inb.any(-1)
        want = torch.where(em_on(inp)[:, None, None], one(1), torch.tensor(0.5)).expand(N, S, 3)
        b["raw_rgb"] = (off[..., None].expand(N, S, 3), want.contiguous())
    return {k: (_expand(inp, m), _expand(inp, v)) for k, (m, v) in b.items()}


def verify_fwd(inp, got, K, evaluate=False):
    G = sampling(inp)
    got = {k: v.detach().cpu() for k, v in got.items()}
    N, S = G.masked.shape
    a_got = got["alpha"].reshape(-1, S)
    first = a_got if inp.get("rep") is None else a_got[inp["first"]]
    r = fwd_q(inp, G, force=first == 1.0, evaluate=evaluate)
    fails = []
    flips = clamp_legit(r, fails)
    ex = lambda t: tuple(None if x is None else _expand(inp, x) for x in t)
    out = {"alpha": ex(_o(r.a, G.masked))}
    if evaluate:
        out.update(depth=ex(_o(r.depth)), disp=ex(_o(r.disp)), white_bg=ex(_o(r.T[:, S])), off_rgb=ex(_o(r.off_rgb)),
                   emo_rgb=ex(_o(r.emo_rgb)), on_rgb=ex(_o(r.on_rgb)))
    else:
        out.update(alphainv_cum=ex(_o(r.T)), weights=ex(_o(r.w)), raw_rgb=ex(_o(r.raw)), rgb=ex(_o(r.rgb)))
    ref = _ref(out, _fwd_bits(inp, G, r, evaluate))
    ref.q = r
    return _finish(r, ref, got, K, flips, N * S, fails)


def verify_eval(inp, got, K):
    return verify_fwd(inp, got, K, evaluate=True)


# ---- backward ---------------------------------------------------------------------------------------------------------
CH = 7                                                       # density, off r g b, emo r g b


def _up(inp, name, shape):
    t = inp.get(name)
    return qz(shape) if t is None else qx(t)


def bwd_values(inp, G, a, T, raw, clamped, grids=None):
    """the explicit adjoint: per sample and channel the value that is spread over the 8 corners, Q [N,S,7], and the corner weights"""
    S = inp["S"]
    K, _ = run_len(S)
    N = a.v.shape[0]
    g = _grids64(inp, grids)
    W = corner_w(G, "q")
    gC = _up(inp, "g_rgb", (N, 3))
    gcum = _up(inp, "g_alphainv_cum", (N, S + 1))
    dw = _up(inp, "g_weights", (N, S))
    for c in range(3):
        dw = dw + gC[:, c][:, None] * raw[..., c]
    gj = gcum[:, :S] + dw * a
    p = xwhere(clamped, Q(torch.full(clamped.shape, P_MIN, dtype=F64)), 1.0 - a)
    Rv, RE = gcum.v[:, S].clone(), torch.zeros(N, dtype=F64)
    RM = Rv.abs()
    rounds = 3.0 * (2 * K + 7)
    vs, Es = [None] * S, [None] * S
    for j in range(S - 1, -1, -1):
        vs[j], Es[j] = Rv, RE + rounds * RM
        pv, pE = p.v[:, j], p.E[:, j]
        RE = pv.abs() * RE + Rv.abs() * pE + gj.E[:, j]
        RM = pv.abs() * RM + gj.v[:, j].abs()
        Rv = pv * Rv + gj.v[:, j]
    R = Q(torch.stack(vs, 1), torch.stack(Es, 1)) if S else qz((N, 0))
    Tj = T[:, :S]
    dwT = dw * Tj
    da = xwhere(clamped, dwT, dwT - Tj * R)
    x, e = alpha_q(inp, G, W, g)
    dad = (e * inp["interval"]) * xspgrad(x)
    v0 = xwhere(G.masked, qz(G.masked.shape), da * dad)
    w = a * Tj
    draw = _up(inp, "g_raw_rgb", (N, S, 3)) + gC[:, None, :] * w[..., None]
    so = xsigmoid(fetch(g["off_color"], G, W, "q"))
    se = xsigmoid(fetch(g["emo_color"], G, W, "q"))
    perm = lambda q: Q(q.v.permute(1, 2, 0), q.E.permute(1, 2, 0))
    so, se = perm(so), perm(se)
    voff = (draw * (1.0 - so)) * so
    vemo = xwhere(em_on(inp)[:, None, None], (draw * (1.0 - se)) * se, qz((N, S, 3)))
    vals = Q(torch.cat([v0.v[..., None], voff.v, vemo.v], -1), torch.cat([v0.E[..., None], voff.E, vemo.E], -1))
    return vals, W


def scatter_cells(inp, G, contrib, init, run_of_sample, mult=None):
    """contrib Q [N,S,8,C], init [C, cells] float64 -> (value, absref, touched) [C, cells] by the per-cell rule of the docstring"""
    N, S = G.masked.shape
    C, ncell = init.shape
    keep = G.inb.reshape(-1)
    cell = G.cell.reshape(-1)[keep]
    m = torch.ones(N, dtype=F64) if mult is None else mult.double()
    mk = m[:, None, None].expand(N, S, 8).reshape(-1)[keep]
    v = contrib.v.detach().reshape(-1, C)[keep]
    E = contrib.E.reshape(-1, C)[keep]
    z = lambda: torch.zeros(ncell, C, dtype=F64)
    s = z().index_add_(0, cell, v * mk[:, None])
    M = z().index_add_(0, cell, v.abs() * mk[:, None])
    Es = z().index_add_(0, cell, E * mk[:, None])
    n = z().index_add_(0, cell, (v != 0).double() * mk[:, None])
    frac = z().index_add_(0, cell, ((v != torch.round(v)) | (E != 0)).double())
    # r: the most samples of one run that fall into the cell
    run = (torch.arange(N)[:, None] * (S + 1) + run_of_sample[None, :])[:, :, None].expand(N, S, 8).reshape(-1)[keep]
    key, cnt = torch.unique(run * ncell + cell, return_counts=True)
    r = torch.zeros(ncell, dtype=F64).scatter_reduce_(0, key % ncell, cnt.double(), "amax", include_self=True)
    i0 = init.T
    absref = Es + r[:, None] * M + n * (i0.abs() + M)
    exact = (frac == 0) & (i0 == torch.round(i0)) & (i0.abs() + M < 2.0 ** 24)
    absref = torch.where(exact, torch.zeros_like(absref), absref)
    return (i0 + s).T, absref.T, (n > 0).T


GRAD_NAMES = ("grad_density", "grad_off", "grad_emo")


def _planes(t3):
    """[grad_density [X,Y,Z], grad_off [3,..], grad_emo [3,..]] -> [7, cells]"""
    return torch.cat([t.reshape(-1, t.shape[-3] * t.shape[-2] * t.shape[-1]) for t in t3], 0)


def _unplanes(inp, t):
    X, Y, Z = inp["dims"]
    return {"grad_density": t[0].reshape(X, Y, Z), "grad_off": t[1:4].reshape(3, X, Y, Z), "grad_emo": t[4:7].reshape(3, X, Y, Z)}


def verify_bwd(inp, got, K):
    """got: alpha, alphainv_cum, raw_rgb (the forward's outputs the backward read), the three gradient buffers and their copies of the
    call with no upstream gradient (null_*)"""
    G = sampling(inp)
    got = {k: v.detach().cpu() for k, v in got.items()}
    N, S = G.masked.shape
    pick = (lambda t: t) if inp.get("rep") is None else (lambda t: t[inp["first"]])
    a32, T32, raw32 = pick(got["alpha"].reshape(-1, S)), pick(got["alphainv_cum"].reshape(-1, S + 1)), pick(got["raw_rgb"].reshape(-1, S, 3))
    clamped = (a32 == 1.0) & ~G.masked
    fails = []
    r = fwd_q(inp, G, force=clamped)
    flips = clamp_legit(r, fails)
    for name, q, t in (("alpha", r.a, a32), ("alphainv_cum", r.T, T32), ("raw_rgb", r.raw, raw32)):
        if not bool(torch.isfinite(t).all()) or bool(((t.double() - q.v.detach()).abs() > 16 * K * U * q.E + FLOOR).any()):
            fails.append(f"{name}: the forward output the backward reads is far from the restatement")   # (a gate, not the bound)
    vals, W = bwd_values(inp, G, qx(a32), qx(T32), qx(raw32), clamped)
    contrib = vals[..., None, :] * Q(W.v[..., None], W.E[..., None])
    init = _planes([inp["grad0"][k].double() for k in GRAD_NAMES])
    Kr, _ = run_len(S)
    val, absref, touched = scatter_cells(inp, G, contrib, init, torch.arange(S) // Kr, inp.get("mult"))
    out, b = {}, {}
    init32 = _unplanes(inp, _planes([inp["grad0"][k] for k in GRAD_NAMES]))
    for (k, v), (_, e), (_, t) in zip(_unplanes(inp, val).items(), _unplanes(inp, absref).items(), _unplanes(inp, touched).items()):
        out[k] = (v, e, None)
        b[k] = (~t, init32[k])
        b["null_" + k] = (torch.ones_like(t), init32[k])
    got = {k: v for k, v in got.items() if k in out or k in b}
    ref = _ref(out, b)
    ref.count = touched
    return _finish(r, ref, got, K, flips, N * S, fails)


# ---- view count -------------------------------------------------------------------------------------------------------
def count_parts(inp):
    """float64 sums of the distinct rays (weights of the unjittered, unmasked samples), by the per-cell rule"""
    G = sampling(inp, jitter=False)
    W = corner_w(G, "q")
    N, S = G.masked.shape
    contrib = Q(W.v[..., None], W.E[..., None])
    init = inp["sum0"].double().reshape(1, -1)
    return scatter_cells(inp, G, contrib, init, torch.zeros(S, dtype=torch.long), inp.get("mult"))


def verify_count(inp, got, K):
    got = {k: v.detach().cpu() for k, v in got.items()}
    val, absref, _ = count_parts(inp)
    dims = inp["dims"]
    val, absref = val.reshape(dims), absref.reshape(dims)
    s_got = got["sum"].reshape(dims)
    want = inp["count0"] + (s_got > 1.0).float()
    flip = (s_got > 1.0) != (val > 1.0)
    bad = flip & ~((val - 1.0).abs() < DEC_K * U * absref)
    fails = []
    if bool(bad.any()):
        fails.append(f"count: {int(bad.sum())} voxels decide sum > 1 against a float64 sum outside the band of 1")
    ref = _ref({"sum": (val, absref, None)}, {"count": (torch.ones(dims, dtype=torch.bool), want)})
    ref.flips = {"sum > 1": int(flip.sum())}
    ref.share = int(flip.sum()) / max(1, val.numel())
    worst, f2 = _judge(ref, got, K)
    fails += f2
    if ref.share > FLIP_CAP:
        fails.append(f"the exempt share {ref.share:.3g} exceeds FLIP_CAP")
    return ref, worst, fails


# =======================================================================================================================
# the binary32 emulation, in the kernel's structure
# =======================================================================================================================
def _runs(x, S, K, L, fill):
    """[N,S,...] -> [N,L,K,...], the tail filled"""
    pad = L * K - S
    if pad:
        x = torch.cat([x, torch.full((x.shape[0], pad) + tuple(x.shape[2:]), fill, dtype=x.dtype)], 1)
    return x.reshape(x.shape[0], L, K, *x.shape[2:])


def _shift_up(x, off, fill):
    """lane l reads lane l - off (the fill below lane `off`)"""
    off = min(off, x.shape[1])
    return torch.cat([torch.full_like(x[:, :off], fill), x[:, :x.shape[1] - off]], 1)


def _shift_down(x, off, fill):
    off = min(off, x.shape[1])
    return torch.cat([x[:, off:], torch.full_like(x[:, :off], fill)], 1)


def wave_sum32(v):
    """esr_wave_sum of [N,L,..] lane values (lanes beyond L hold 0): the xor butterfly off = 32 .. 1, lane 0's result"""
    N, L = v.shape[:2]
    v = torch.cat([v, torch.zeros((N, WAVE - L) + tuple(v.shape[2:]), dtype=v.dtype)], 1)
    lanes = torch.arange(WAVE)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lanes ^ off]
    return v[:, 0]


def _grids32(inp):
    return {k: inp[k].reshape(inp[k].shape[0] if k != "density" else 1, -1) for k in ("density", "off_color", "emo_color")}


def _softplus32(x):
    return torch.where(x > 20, x, torch.log1p(torch.exp(x.clamp(max=20.0))))


def emu_forward(inp, mut=None, evaluate=False):
    """-> (outputs, namespace of the intermediates)"""
    S = inp["S"]
    K, L = run_len(S)
    G = sampling(inp)
    N = G.masked.shape[0]
    g, W = _grids32(inp), corner_w(G, "32")
    x = fetch(g["density"], G, W, "32")[0] + inp["act_shift"]
    a = 1.0 - torch.exp((-_softplus32(x)) * inp["interval"])
    if mut != "masked_sample_keeps_alpha":
        a = torch.where(G.masked, torch.zeros(()), a)
    p = torch.maximum(1.0 - a, P_MIN32)
    pr = _runs(p, S, K, L, 1.0)
    prod = torch.ones(N, L)
    for k in range(K):
        prod = prod * pr[:, :, k]
    incl = prod
    for off in (1, 2, 4, 8, 16, 32):
        incl = incl * _shift_up(incl, off, 1.0)
    excl = _shift_up(incl, 1, 1.0)
    T = torch.ones(N, L) if mut == "run_transmittance_restarts_at_one" else excl
    Ts = []
    for k in range(K):
        Ts.append(T)
        T = T * pr[:, :, k]
    Tj = torch.stack(Ts, 2).reshape(N, L * K)[:, :S]
    TS = T[:, (S - 1) // K]
    if mut == "last_transmittance_from_lane_63" and L == WAVE:
        # Reading the final T of lane 63 itself is benign: a lane that owns nothing holds the product of every lane before it, the same
        # T_S in another order.  What this mutant guards is the order inside the owner: lane 63's T from BEFORE its own run, wrong
        # whenever lane 63 owns a sample (S = 64, 127, 128).
        TS = excl[:, WAVE - 1]
    if mut == "last_transmittance_owner_ignores_run_length":
        # the owner taken as lane (S - 1) mod 64, as if K were 1: a lane in front of the true owner (S - 1) / K whenever K > 1
        # (S = 65, 129: lane 0; S = 200: lane 7), whose T lacks the runs behind it
        own = (S - 1) % WAVE
        TS = T[:, own] if own < L else T[:, L - 1]
    w = a * Tj
    so = xsigmoid(fetch(g["off_color"], G, W, "32")).permute(1, 2, 0)
    se = xsigmoid(fetch(g["emo_color"], G, W, "32")).permute(1, 2, 0)
    valid = (torch.arange(L * K) < S).reshape(L, K)

    def lane_sum(term):                                      # fma(w, value, acc) along the run, then the wave sum
        tr = _runs(term[0], S, K, L, 0.0), _runs(term[1], S, K, L, 0.0)
        acc = torch.zeros((N, L) + tuple(tr[1].shape[3:]))
        for k in range(K):
            wk = tr[0][:, :, k]
            acc = fma32(wk.reshape(wk.shape + (1,) * (tr[1].dim() - 3)), tr[1][:, :, k], acc)
        return wave_sum32(acc)
    out = {"alpha": a}
    if evaluate:
        dd = inp["rays_o"][:, None, :] - G.pts
        dist = sqrt32((dd[..., 0] * dd[..., 0] + dd[..., 1] * dd[..., 1]) + dd[..., 2] * dd[..., 2])
        if mut == "depth_from_t_instead_of_distance":
            dist = G.t
        off_rgb, emo_rgb, depth = lane_sum((w, so)), lane_sum((w, se)), lane_sum((w, dist))
        out.update(depth=depth, disp=1.0 / (depth + TS * inp["far"]), white_bg=TS, off_rgb=off_rgb, emo_rgb=emo_rgb, on_rgb=off_rgb + emo_rgb)
    else:
        on = em_on(inp)
        if mut == "emo_added_on_mode_0_ray":
            on = torch.ones_like(on)
        raw = torch.where(on[:, None, None], se + so, so)
        out.update(alphainv_cum=torch.cat([Tj, TS[:, None]], 1), weights=w, raw_rgb=raw, rgb=lane_sum((w, raw)))
    out = {k: _expand(inp, v) for k, v in out.items()}
    return out, SimpleNamespace(G=G, W=W, x=x, a=a, p=p, Tj=Tj, so=so, se=se, valid=valid, g=g)


def emu_fwd(inp, mut=None):
    return emu_forward(inp, mut)[0]


def emu_eval(inp, mut=None):
    return emu_forward(inp, mut, evaluate=True)[0]


class CellAcc:
    """the per-lane cell accumulator of the scatters, for [N,L] lanes at once: base [N,L,3], v [N,L,8,C]; dst [C, cells] binary32"""
    def __init__(self, N, L, C, dst, dims, mut=None):
        self.base = torch.full((N, L, 3), -2 ** 30, dtype=torch.long)
        self.v = torch.zeros(N, L, 8, C)
        self.dst, self.dims, self.mut, self.C = dst, dims, mut, C

    def _add_corner(self, k, sel):
        c = torch.tensor((k >> 2, (k >> 1) & 1, k & 1))
        xyz = self.base + c
        inb = sel.clone()
        for a in range(3):
            inb &= (xyz[..., a] >= 0) & (xyz[..., a] < self.dims[a])
        flat = (xyz[..., 0] * self.dims[1] + xyz[..., 1]) * self.dims[2] + xyz[..., 2]
        v = self.v[:, :, k, :]
        m = inb[..., None] & (v != 0)
        ncell = self.dst.shape[1]
        idx = (torch.arange(self.C)[None, None, :] * ncell + flat[..., None])[m]
        self.dst.reshape(-1).index_add_(0, idx, v[m])

    def sample(self, i0, valid, w8, val):
        """i0 [N,L,3] cell of the next sample, valid [N,L] or [L], w8 [N,L,8], val [N,L,C]"""
        mut = self.mut
        valid = valid.expand(i0.shape[:2])
        d = torch.where(valid[..., None], i0 - self.base, torch.zeros((), dtype=torch.long))
        moved = (d != 0).any(-1)
        for k in range(8):
            c = (k >> 2, (k >> 1) & 1, k & 1)
            keep = torch.ones_like(moved)
            for a in range(3):
                n_ = c[a] - d[..., a]
                keep &= (n_ >= 0) & (n_ <= 1)
            self._add_corner(k, moved if mut == "moved_corner_added_and_kept" else moved & ~keep)
        far = (d.abs() > 1).any(-1)
        v = self.v
        before = torch.zeros_like(moved)
        for axis, bit in ((0, 4), (1, 2), (2, 1)):
            da = d[..., axis]
            if mut == "diagonal_move_keeps_a_face":
                da = torch.where(before, torch.zeros_like(da), da)
                before = before | (d[..., axis] != 0)
            up, dn = (da == 1)[..., None, None], (da == -1)[..., None, None]
            if mut == "negative_move_shifts_the_wrong_way":
                up, dn = up | dn, torch.zeros_like(dn)
            lo = [k for k in range(8) if not k & bit]
            hi = [k | bit for k in lo]
            l, h = v[:, :, lo, :], v[:, :, hi, :]
            zero = torch.zeros(())
            v = v.clone()
            v[:, :, lo, :] = torch.where(up, h, torch.where(dn, zero, l))
            v[:, :, hi, :] = torch.where(up, zero, torch.where(dn, l, h))
        if mut != "far_move_keeps_corners":
            v = torch.where(far[..., None, None], torch.zeros(()), v)
        self.base = torch.where(valid[..., None], i0, self.base)
        self.v = torch.where(valid[..., None, None], fma32(val[..., None, :], w8[..., :, None], v), v)

    def flush(self):
        if self.mut == "last_cell_never_flushed":
            return
        every = torch.ones(self.base.shape[:2], dtype=torch.bool)
        for k in range(8):
            self._add_corner(k, every)


def _times(inp, run_once, dst0):
    """the scatter of the distinct rays, repeated for the cases that repeat their ray set"""
    if inp.get("mult") is None:
        run_once(dst0, None)
        return dst0
    for m in torch.unique(inp["mult"]).tolist():
        delta = torch.zeros_like(dst0)
        run_once(delta, inp["mult"] == m)
        if bool((delta != 0).any()):
            for _ in range(m):
                dst0 += delta
    return dst0


def emu_bwd(inp, mut=None):
    S, dims = inp["S"], inp["dims"]
    K, L = run_len(S)
    fw, f = emu_forward(dict(inp, rep=None))
    G, W, N = f.G, f.W, f.a.shape[0]
    a, Tj, raw = f.a, f.Tj, fw["raw_rgb"]
    z = lambda *s: torch.zeros(*s)
    gC = inp["g_rgb"] if inp.get("g_rgb") is not None else z(N, 3)
    gcum = inp["g_alphainv_cum"] if inp.get("g_alphainv_cum") is not None else z(N, S + 1)
    dw = inp["g_weights"] if inp.get("g_weights") is not None else z(N, S)
    for c in range(3):
        dw = fma32(gC[:, c][:, None].expand(N, S), raw[..., c], dw)
    gj = gcum[:, :S] + dw * a
    p = f.p
    R_ = lambda t, fill: _runs(t, S, K, L, fill)
    pr, gr = R_(p, 1.0), R_(gj, 0.0)
    A, B = torch.ones(N, L), torch.zeros(N, L)
    for k in range(K):
        B = fma32(A, gr[:, :, k], B)
        A = A * pr[:, :, k]
    for off in (1, 2, 4, 8, 16, 32):
        A2, B2 = _shift_down(A, off, 1.0), _shift_down(B, off, 0.0)
        B = B + A * B2
        A = A * A2
    if mut != "suffix_scan_includes_own_lane":
        A, B = _shift_down(A, 1, 1.0), _shift_down(B, 1, 0.0)
    gS = z(N) if mut == "g_alphainv_cum_last_column_dropped" else gcum[:, S]
    Rr = fma32(A, gS[:, None].expand(N, L), B)
    xr = R_(f.x, 0.0)
    e = torch.exp((-_softplus32(xr)) * inp["interval"])
    zz = torch.exp(xr.clamp(max=20.0))
    dad = (e * inp["interval"]) * torch.where(xr > 20, torch.ones(()), zz / (zz + 1.0))
    ar, Tr, dwr = R_(a, 0.0), R_(Tj, 0.0), R_(dw, 0.0)
    wr = ar * Tr
    draw = R_(inp["g_raw_rgb"] if inp.get("g_raw_rgb") is not None else z(N, S, 3), 0.0)
    if mut != "g_rgb_missing_from_colour_gradient":
        draw = fma32(gC[:, None, None, :].expand_as(draw), wr[..., None].expand_as(draw), draw)
    sor, ser = R_(f.so, 0.5), R_(f.se, 0.5)
    voff = draw * (1.0 - sor) * sor
    vemo = torch.where(em_on(inp)[:, None, None, None], draw * (1.0 - ser) * ser, torch.zeros(()))
    mr = R_(G.masked, True)
    i0r, Wr = R_(G.i0, 0), R_(W, 0.0)
    vals = []
    for k in range(K - 1, -1, -1):
        vk = f.valid[:, k]
        ak, Tk = ar[:, :, k], Tr[:, :, k]
        dp = Tk * Rr
        da = dwr[:, :, k] * Tk
        sub = (1.0 - ak) >= P_MIN32
        if mut == "clamp_passes_gradient_below_min":
            sub = torch.ones_like(sub)
        da = torch.where(sub, da - dp, da)
        Rr = torch.where(vk[None], fma32(pr[:, :, k], Rr, gr[:, :, k]), Rr)
        v0 = torch.where(mr[:, :, k], torch.zeros(()), da * dad[:, :, k])
        vals.append((k, vk, torch.cat([v0[..., None], voff[:, :, k], vemo[:, :, k]], -1)))

    def once(dst, only):
        sel = torch.ones(N, dtype=torch.bool) if only is None else only
        acc = CellAcc(int(sel.sum()), L, CH, dst, dims, mut)
        for k, vk, v in vals:
            acc.sample(i0r[sel][:, :, k], vk[None], Wr[sel][:, :, k], v[sel])
        acc.flush()
    dst = _planes([inp["grad0"][k].clone() for k in GRAD_NAMES])
    _times(inp, once, dst)
    out = _unplanes(inp, dst)
    out.update({"null_" + k: inp["grad0"][k].clone() for k in GRAD_NAMES})
    out.update(alpha=fw["alpha"], alphainv_cum=fw["alphainv_cum"], raw_rgb=fw["raw_rgb"])
    return {k: (_expand(inp, v) if k in ("alpha", "alphainv_cum", "raw_rgb") else v) for k, v in out.items()}


def emu_count(inp, mut=None):
    S, dims = inp["S"], inp["dims"]
    G = sampling(inp, jitter=mut == "jitter_applied_to_the_view_count")
    W = corner_w(G, "32")
    N = G.masked.shape[0]
    one = torch.ones(N, 1, 1)

    def once(dst, only):
        sel = torch.ones(N, dtype=torch.bool) if only is None else only
        acc = CellAcc(int(sel.sum()), 1, 1, dst, dims, mut)
        for j in range(S):
            acc.sample(G.i0[sel][:, j][:, None], torch.ones(1, dtype=torch.bool)[None], W[sel][:, j][:, None], one[sel])
        acc.flush()
    s = _times(inp, once, inp["sum0"].clone().reshape(1, -1)).reshape(dims)
    thr = (s >= 1.0) if mut == "count_threshold_at_equal" else (s > 1.0)
    return {"sum": s, "count": inp["count0"] + thr.float()}


# =======================================================================================================================
# cases
# =======================================================================================================================
GRIDS = {
    "5x4x3": dict(dims=(5, 4, 3), lo=(-1.0, -0.75, -0.5), hi=(1.5, 1.0, 0.75), voxel=0.6),
    "1x6x2": dict(dims=(1, 6, 2), lo=(-0.5, -1.0, -0.5), hi=(0.5, 1.5, 0.25), voxel=0.5),
    "9x9x9": dict(dims=(9, 9, 9), lo=(0.0, 0.0, 0.0), hi=(8.0, 8.0, 8.0), voxel=1.0),
}
# the special rays on the 9^3 lattice box [0,8]^3 (mapped affinely into the other boxes): (origin, direction)
SPECIAL = [
    ((-2.0, 3.0, 5.0), (2.0, 0.0, 0.0)),         # +x along a lattice line, |d| = 2
    ((4.0, 10.0, 2.0), (0.0, -1.0, 0.0)),        # -y along a lattice line
    ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)),       # the body diagonal
    ((9.0, 9.0, 9.0), (-1.0, -1.0, -1.0)),       # and its reverse
    ((-0.5, 8.5, 3.3), (1.0, -1.0, 0.0)),        # mixed move signs (+1, -1, 0)
    ((3.0, 3.0, 3.0), (1.0, 0.0, 0.0)),          # origin inside the box, on a node
    ((-3.0, 20.0, 4.0), (1.0, 0.0, 0.0)),        # misses the box
    ((5.5, 2.2, 6.1), (1.0, 0.1, 0.0)),          # origin inside, leaves through the +x face after 2.5 voxels
    ((0.5, 7.6, -1.0), (0.0, 0.3, 1.5)),         # grazes the upper y face: cells of base dims - 1
    ((8.0, 8.0, -2.0), (0.0, 0.0, 1.0)),         # along the upper corner edge: every sample on the last node of two axes
]


def _rays(grid, n, seed, first=0):
    g = GRIDS[grid]
    lo, hi = torch.tensor(g["lo"], dtype=F64), torch.tensor(g["hi"], dtype=F64)
    gen = _gen(seed)
    o, d = [], []
    for k in range(n):
        if k < len(SPECIAL):
            so, sd = SPECIAL[(k + first) % len(SPECIAL)]
            o.append(lo + torch.tensor(so, dtype=F64) / 8.0 * (hi - lo))
            d.append(torch.tensor(sd, dtype=F64) / 8.0 * (hi - lo))
        else:
            c, h = (lo + hi) / 2, (hi - lo) / 2
            u = torch.randn(3, generator=gen, dtype=F64)
            src = c + 2.5 * float(h.norm()) * u / u.norm()
            dst = c + h * (torch.rand(3, generator=gen, dtype=F64) * 2 - 1)
            o.append(src)
            d.append((dst - src) * float(0.5 + 1.5 * torch.rand(1, generator=gen, dtype=F64)))
    return torch.stack(o).float(), torch.stack(d).float()


def _density(kind, grid, seed):
    dims = GRIDS[grid]["dims"]
    gen = _gen(seed)
    smooth = torch.randn(*dims, generator=gen) * 2.0 + 1.0
    if kind == "smooth":
        return smooth
    if kind == "empty":
        return torch.full(dims, -100.0)
    if kind == "opaque":
        return torch.full(dims, 1e4)
    if kind == "mixed":                                     # smooth, with an empty slab and an opaque slab
        t = smooth.clone()
        t[..., 0] = -100.0
        t[:, -1] = 1e4
        return t
    if kind == "ramp":                                      # along the +x lattice line y = 3, z = 5: softplus(d + shift) interval =
        t = torch.full(dims, -100.0)                        # 17.8 .. 16.8 across the 2^-25 threshold at 17.33 (9^3 grid only); the
        for i in range(dims[0]):                            # clamped samples come first, where T is still 1
            t[i, 3, 5] = (17.8 - 0.125 * i) / INTERVAL - ACT_SHIFT
        t[:, 4:6, 2] = 3.0                                  # something behind the -y line too
        return t
    raise KeyError(kind)


INTERVAL, ACT_SHIFT = 0.5, -2.0
UP_KINDS = {"cum": ("g_alphainv_cum",), "weights": ("g_weights",), "raw": ("g_raw_rgb",), "rgb": ("g_rgb",),
            "all": ("g_alphainv_cum", "g_weights", "g_raw_rgb", "g_rgb"), "none": ()}

# name: grid, step in voxels, S, rays, first special ray, jitter, em, density, upstream (backward)
_T = lambda grid, step, S, n, first, jit, em, dens, up: dict(grid=grid, step=step, S=S, n=n, first=first, jitter=jit, em=em, density=dens, up=up)
TRAIN_CASES = {
    "lattice_S1_n1": _T("9x9x9", 1.0, 1, 1, 0, None, "all0", "smooth", "all"),
    "lattice_S2_n3": _T("9x9x9", 1.0, 2, 3, 1, "zero", "all1", "smooth", "cum"),
    "lattice_S11_n10_ramp": _T("9x9x9", 1.0, 11, 10, 0, None, "mixed", "ramp", "all"),
    "lattice_S63_n4": _T("9x9x9", 1.0, 63, 4, 2, None, "mixed", "mixed", "weights"),
    "lattice_S64_n5": _T("9x9x9", 0.1, 64, 5, 0, "0.999", "all1", "smooth", "raw"),
    "lattice_S65_n12_opaque": _T("9x9x9", 0.5, 65, 12, 0, "random", "mixed", "opaque", "all"),
    "g543_S127_n5": _T("5x4x3", 0.1, 127, 5, 4, "random", "all0", "smooth", "rgb"),
    "g543_S128_n12": _T("5x4x3", 0.1, 128, 12, 0, None, "mixed", "mixed", "all"),
    "g543_S129_n4_far": _T("5x4x3", 2.5, 129, 4, 0, "random", "mixed", "smooth", "all"),
    "g543_S200_n13": _T("5x4x3", 0.1, 200, 13, 0, "random", "mixed", "smooth", "all"),
    "g543_S65_n3_step7": _T("5x4x3", 7.0, 65, 3, 2, None, "all1", "smooth", "all"),
    "g162_S129_n12": _T("1x6x2", 0.1, 129, 12, 0, "random", "mixed", "smooth", "all"),
    "g162_S5_n11_empty": _T("1x6x2", 1.0, 5, 11, 0, "zero", "all0", "empty", "none"),
    "g543_S3_second_trip": _T("5x4x3", 1.0, 3, TRIP * WAVES + 5, 0, "random", "mixed", "smooth", "all"),
}
BIG_TRAIN = "g543_S3_second_trip"
BIG_DISTINCT = 37
_C = lambda grid, step, S, n, first, jit, sum0: dict(grid=grid, step=step, S=S, n=n, first=first, jitter=jit, sum0=sum0)
COUNT_CASES = {
    "lattice_S9_n10": _C("9x9x9", 1.0, 9, 10, 0, "random", "zero"),
    "lattice_S12_n300": _C("9x9x9", 0.5, 12, 300, 0, None, "zero"),
    "g543_S20_n5": _C("5x4x3", 0.5, 20, 5, 2, "0.999", "random"),
    "g543_S7_n40_far": _C("5x4x3", 2.5, 7, 40, 0, None, "random"),
    "g543_S4_n3_step7": _C("5x4x3", 7.0, 4, 3, 2, None, "zero"),
    "g543_S40_n1_step0.1": _C("5x4x3", 0.1, 40, 1, 4, None, "zero"),
    "g162_S9_n257": _C("1x6x2", 1.0, 9, 257, 0, "random", "random"),
    "g543_S2_second_trip": _C("5x4x3", 1.0, 2, COUNT_BLOCK * TRIP + 259, 0, None, "zero"),
}
BIG_COUNT = "g543_S2_second_trip"
_CACHE = {}


def _base(name, c, seed):
    g = GRIDS[c["grid"]]
    n = c["n"]
    inp = dict(name=name, dims=g["dims"], lo=torch.tensor(g["lo"], dtype=F32), hi=torch.tensor(g["hi"], dtype=F32), near=0.0, far=64.0,
               step_scale=f32(c["step"] * g["voxel"]), interval=f32(INTERVAL), act_shift=f32(ACT_SHIFT), S=c["S"], grid=c["grid"], step=c["step"])
    gen = _gen(seed)
    big = n > 4096
    nd = BIG_DISTINCT if big else n
    inp["rays_o"], inp["rays_d"] = _rays(c["grid"], nd, seed + 1, c["first"])
    if big:                                                  # a small ray set repeated: the reference works on the distinct rays
        if "sum0" in c:                                      # view count: all but three islands of rays pass far from the grid
            far_ray = nd - 1
            inp["rays_o"][far_ray] = torch.tensor([50.0, 50.0, 50.0])
            inp["rays_d"][far_ray] = torch.tensor([1.0, 0.0, 0.0])
            rep = torch.full((n,), far_ray, dtype=torch.long)
            for start in (0, COUNT_BLOCK * TRIP - 18, n - 36):
                rep[start:start + 36] = torch.arange(36)
        else:
            rep = torch.arange(n) % nd
        inp["rep"], inp["mult"] = rep, torch.bincount(rep, minlength=nd)
        inp["first"] = torch.stack([torch.nonzero(rep == k)[0, 0] for k in range(nd)])
    jk = c["jitter"]
    inp["jitter"] = None if jk is None else torch.zeros(nd) if jk == "zero" else torch.full((nd,), f32(0.999)) if jk == "0.999" \
        else torch.rand(nd, generator=gen)
    inp["jitter_kind"] = jk
    return inp, gen, nd


def full_rays(inp):
    """the ray arrays as the kernel receives them (the repeated ray set expanded)"""
    ex = lambda t: None if t is None else _expand(inp, t).contiguous()
    return {k: ex(inp.get(k)) for k in ("rays_o", "rays_d", "jitter", "em_modes", "g_alphainv_cum", "g_weights", "g_raw_rgb", "g_rgb")}


def _wide(shape, gen):
    """magnitudes 1e-6 .. 1e3, mixed signs, exact zeros planted"""
    t = torch.sign(torch.randn(shape, generator=gen)) * torch.pow(10.0, torch.rand(shape, generator=gen) * 9 - 6)
    flat = t.reshape(-1)
    flat[::5] = 0.0
    return t


def case_train(name):
    if ("train", name) in _CACHE:
        return _CACHE[("train", name)]
    c = TRAIN_CASES[name]
    seed = 100 + sum(map(ord, name))
    inp, gen, nd = _base(name, c, seed)
    dims, S = inp["dims"], inp["S"]
    inp["density"] = _density(c["density"], c["grid"], seed + 2)
    inp["off_color"], inp["emo_color"] = torch.randn(3, *dims, generator=gen) * 1.5, torch.randn(3, *dims, generator=gen) * 1.5
    em = c["em"]
    inp["em_all"] = 1 if em == "all1" else 0
    inp["em_modes"] = (torch.arange(nd) % 3).to(I32) if em == "mixed" else None
    for k, shape in (("g_alphainv_cum", (nd, S + 1)), ("g_weights", (nd, S)), ("g_raw_rgb", (nd, S, 3)), ("g_rgb", (nd, 3))):
        inp[k] = _wide(shape, gen) if k in UP_KINDS[c["up"]] else None
    inp["grad0"] = {"grad_density": torch.randn(*dims, generator=gen) * 0.1, "grad_off": torch.randn(3, *dims, generator=gen) * 0.1,
                    "grad_emo": torch.randn(3, *dims, generator=gen) * 0.1}
    inp["up"], inp["density_kind"], inp["em_kind"] = c["up"], c["density"], em
    inp["census"] = census(inp, count=False)
    inp["claims"] = set(inp["census"])
    _CACHE[("train", name)] = inp
    return inp


def case_count(name):
    if ("count", name) in _CACHE:
        return _CACHE[("count", name)]
    c = COUNT_CASES[name]
    seed = 500 + sum(map(ord, name))
    inp, gen, nd = _base(name, c, seed)
    dims = inp["dims"]
    inp["sum0"] = torch.zeros(dims) if c["sum0"] == "zero" else torch.rand(*dims, generator=gen) * 0.5
    inp["count0"] = torch.randint(0, 4, dims, generator=gen).float()
    inp["em_modes"], inp["em_all"] = None, 0
    inp["census"] = census(inp, count=True)
    inp["claims"] = set(inp["census"])
    _CACHE[("count", name)] = inp
    return inp


# ---- census -----------------------------------------------------------------------------------------------------------
def census(inp, count):
    """the classes a case reaches, from its data"""
    S, dims = inp["S"], inp["dims"]
    n = inp["rays_o"].shape[0] if inp.get("rep") is None else inp["rep"].numel()
    K, L = (S, 1) if count else run_len(S)
    G = sampling(inp, jitter=not count)
    c = {f"S = {S}", f"K = {K}", f"grid {inp['grid']}", f"step {inp['step']} voxels", f"{n} rays" if n <= 5 else "more than 5 rays"}
    if not count:
        if S % K:
            c.add("ragged last run")
        if L < WAVE:
            c.add("empty tail lanes")
        if L < WAVE and (S - 1) // K > 0:
            c.add("owner of the last sample in the middle of the wave")
        if L == WAVE:
            c.add("lane 63 owns a sample")
        if n > TRIP * WAVES:
            c.add("second trip")
    elif n > COUNT_BLOCK * TRIP:
        c.add("second trip")
    if 1 in dims:
        c.add("axis of length 1")
    jk = inp["jitter_kind"]
    c.add("jitter NULL" if jk is None else f"jitter {jk}")
    if bool((inp["rays_d"] == 0).any()):
        c.add("exact-zero direction component")
    inside = ((inp["rays_o"] > inp["lo"]) & (inp["rays_o"] < inp["hi"])).all(-1)
    if bool(inside.any()):
        c.add("origin inside the box")
    if bool(G.miss.any()):
        c.add("ray misses the box")
    some = G.inb.any(-1)
    node = ((G.w1 == 0) | (G.w1 == 1)).all(-1).all(-1)
    if bool((node & some).any()):
        c.add("sample on a node")
    part = some & ~G.inb.all(-1)
    for a in range(3):
        if bool((part & (G.i0[..., a] == -1)).any()):
            c.add("cell of base -1 with corners on the grid")
        if bool((part & (G.i0[..., a] == dims[a] - 1)).any()):
            c.add("cell of base dims - 1 with corners on the grid")
    # moves inside a run, in the order the scatter walks (the backward walks a run from its end)
    run = torch.arange(S) // K
    same = run[1:] == run[:-1]
    if S > 1:
        d = (G.i0[:, 1:] - G.i0[:, :-1])[:, same]
        touch = (some[:, 1:] | some[:, :-1])[:, same]
        d = d[touch]
        if count is False:
            d = -d
        nz = (d != 0).sum(-1)
        far = (d.abs() > 1).any(-1)
        unit = ~far & (nz > 0)
        for cond, label in (((nz == 0), "no move"), (far, "far move"), (unit & (nz == 1) & (d.sum(-1) == 1), "single-axis move +1"),
                            (unit & (nz == 1) & (d.sum(-1) == -1), "single-axis move -1"), (unit & (nz == 3) & (d == 1).all(-1), "three-axis move +1"),
                            (unit & (nz == 3) & (d == -1).all(-1), "three-axis move -1"),
                            (unit & (d == 1).any(-1) & (d == -1).any(-1) & (d == 0).any(-1), "move with mixed signs (+1, -1, 0)"),
                            (unit & (nz == 2), "two-axis move")):
            if bool(cond.any()):
                c.add(label)
        # samples per cell inside a run
        if bool((((G.i0[:, 2:] == G.i0[:, :-2]).all(-1)) & (same[1:] & same[:-1])[None]).any()):
            c.add("three or more samples of a run in one cell")
        if K >= 2:
            leave = (~G.masked[:, :-1] & G.masked[:, 1:])[:, same] & ~G.miss[:, None]
            if bool(leave.any()):
                c.add("leaves the box inside a run")
    if count:
        c.add("sum starts at 0" if not bool((inp["sum0"] != 0).any()) else "sum starts non-zero")
        return c
    c.add({"all0": "em_modes NULL, em_all 0", "all1": "em_modes NULL, em_all 1", "mixed": "em_modes mixed, with the value 2"}[inp["em_kind"]])
    c.add(f"density {inp['density_kind']}")
    c.add(f"upstream {inp['up']}")
    if any(inp.get(k) is not None and bool((inp[k] == 0).any()) for k in UP_KINDS["all"]):
        c.add("zeros planted in the upstream gradients")
    f = emu_forward(dict(inp, rep=None))[1]
    live = ~G.masked
    if bool((f.a[live] == 0).any()):
        c.add("alpha exactly 0 inside the box")
    if bool((f.a == 1).any()):
        c.add("alpha exactly 1")
    if bool(((f.Tj > 0) & (f.Tj < 2.0 ** -126)).any()):
        c.add("subnormal T")
    if bool((f.Tj == 0).any()):
        c.add("T exactly 0")
    near1 = live & (f.a >= 1.0 - 2.0 ** -20)
    if bool((near1 & (f.a == 1)).any()) and bool((near1 & (f.a < 1)).any()):
        c.add("alpha on both sides of the 2^-25 threshold")
    return c


# =======================================================================================================================
# the operations, their families and the mutants
# =======================================================================================================================
BWD_CASES = list(TRAIN_CASES)
EVAL_CASES = [k for k in TRAIN_CASES if k != BIG_TRAIN]
# op -> (case builder, case names, verify(inp, got, K) -> (ref, worst, fails), binary32 emulation, family, C entry points)
OPS = {
    "dvgo_fwd": (case_train, list(TRAIN_CASES), verify_fwd, emu_fwd, "dvgo_fwd", ("esr_dvgo_fwd",)),
    "dvgo_eval": (case_train, EVAL_CASES, verify_eval, emu_eval, "dvgo_fwd", ("esr_dvgo_eval",)),
    "dvgo_bwd": (case_train, BWD_CASES, verify_bwd, emu_bwd, "dvgo_bwd", ("esr_dvgo_fwd", "esr_dvgo_bwd")),
    "dvgo_count": (case_count, list(COUNT_CASES), verify_count, emu_count, "dvgo_count", ("esr_dvgo_count", "esr_dvgo_count_add")),
}


def build(op, case):
    return OPS[op][0](case)


def all_cases():
    return [(op, case) for op, spec in OPS.items() for case in spec[1]]


def is_big(case):
    return str(case) in (BIG_TRAIN, BIG_COUNT)


def verify(op, inp, got, K):
    return OPS[op][2](inp, dict(got), K)


# K per family, for both test files: the next power of two at or above twice the worst ratio |gpu - ref| / (U absref) measured on the
# MI355X over every case of test_gpu_dvgo_ref64.py (printed under -s); the factor two leaves room for the order of the float atomics.
# The binary32 emulation reaches the same worst ratios to three digits (they seeded the constants before the GPU run); neither the
# device nor the emulation took a clamp or a sum > 1 decision against the float64 branch on any case.
K_FAMILY = {
    "dvgo_fwd": 2,      # measured worst 0.650 (esr_dvgo_fwd: raw_rgb; alpha 0.485, esr_dvgo_eval 0.485; T, weights and the ray sums below 0.2)
    "dvgo_bwd": 2,      # 0.931 (esr_dvgo_bwd: grad_emo on lattice nodes; 0.533 on the 65 541-ray second trip)
    "dvgo_count": 1,    # 0.398 (esr_dvgo_count on g543_S20_n5; the lattice-aligned sums and every count are exact)
}

# mutant of the emulation -> the ops it applies to; each must break the bound (or a bit expectation) on a small case of each of them
MUTANTS = {
    "run_transmittance_restarts_at_one": ["dvgo_fwd", "dvgo_eval"],
    "last_transmittance_from_lane_63": ["dvgo_fwd", "dvgo_eval"],
    "last_transmittance_owner_ignores_run_length": ["dvgo_fwd", "dvgo_eval"],
    "suffix_scan_includes_own_lane": ["dvgo_bwd"],
    "clamp_passes_gradient_below_min": ["dvgo_bwd"],
    "masked_sample_keeps_alpha": ["dvgo_fwd", "dvgo_eval"],
    "emo_added_on_mode_0_ray": ["dvgo_fwd"],
    "g_rgb_missing_from_colour_gradient": ["dvgo_bwd"],
    "g_alphainv_cum_last_column_dropped": ["dvgo_bwd"],
    "moved_corner_added_and_kept": ["dvgo_bwd", "dvgo_count"],
    "diagonal_move_keeps_a_face": ["dvgo_bwd", "dvgo_count"],
    "far_move_keeps_corners": ["dvgo_bwd", "dvgo_count"],
    "negative_move_shifts_the_wrong_way": ["dvgo_bwd", "dvgo_count"],
    "last_cell_never_flushed": ["dvgo_bwd", "dvgo_count"],
    "depth_from_t_instead_of_distance": ["dvgo_eval"],
    "jitter_applied_to_the_view_count": ["dvgo_count"],
    "count_threshold_at_equal": ["dvgo_count"],
}
