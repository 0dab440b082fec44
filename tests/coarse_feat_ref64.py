"""Float64 restatement of the two feature kernels of the coarse renderer (csrc/coarse.hip: esr_coarse_feat_fwd, esr_coarse_feat_bwd) at the
C ABI, with a plain binary32 torch emulation and the input builders shared by tests/test_coarse_feat_ref64_host.py and
tests/test_gpu_coarse_feat_ref64.py; never imported by the product path.

Exact part.  The sample position is the bit-exact replay of esr_ray_geom / esr_ray_point (feat_ref64.ray_geom, ray_point); the index
(esr_world_to_index), its floor and the one-dimensional weights are replayed in binary32 (dvgo_ref64.corners): the cell of a sample is no
banded decision.  `unit` = (p - min) / (max - min) is an exact binary32 quotient and the view direction is copied: bit checks.
Forward, per value on all 72 rows of X [tiles,72,32] and on gnorm, |got - value| <= K U absref + FLOOR with `Q` (lts_ref64):
  rows 0-11, 12-23   colours: 8-term sums (r = 8) of a value times the two-rounding weight (wz wy) wx; rows 12-23 only on tiles < tiles_on
  gnorm              |g| = sqrt((g0^2 + g1^2) + g2^2) of the fetched gradient
  rows 24-26         g / (|g| + 1e-5f)
  rows 30-59, 63-68  sin / cos of unit 2^i (the product is exact) and of the view direction: 2 U absolute on the exact argument (the
                     bound shade_ref64 uses for sinf / cosf)
  bit expectations   rows 69-71 are 0; all 72 rows and gnorm are 0 on padding lanes (rec_ray = -1); rows 12-23 are 0 on off tiles; rows
                     27-29 and 60-62 equal the replay.
Backward, per cell of g_off_color, g_emo_color [X,Y,Z,12] and g_grad_grid [X,Y,Z,3].  X and gnorm are the forward's own outputs and enter
exactly (only rows 24-26 are read); nrm > 0 therefore reads an input and has no band.  The colour gradient of the off net is dX_off
rows 0-11, of the emissive net dX_emo rows 0-11 (voxurfc.py calls that net at colour row 12, so its first 12 inputs are rows 12-23 of
X); dn = dX_off[24..26] + [on] dX_emo[24..26]; den = nrm + eps; g = normal den (two more roundings than the forward's g);
dg = dn / den - [nrm > 0] g (dn . g) / (den den nrm).  Every non-zero value times a non-zero weight is one float atomic:
absref = sum E_i + M + n (|init| + M) per cell (M = sum |contribution|, n = their number).  The host test asserts that this explicit
adjoint equals float64 autograd of the forward.  Before it uses them, verify_bwd holds the rows it read to 16 K U absref of the forward's
restatement: a sanity gate against a garbage tile, not a bound (the forward is held to K by its own operation).  No decision is banded and nothing is exempted: the flip share is 0."""
from __future__ import annotations

from types import SimpleNamespace

import torch

from dvgo_ref64 import corner_w, corners, fma32, scatter_cells, sqrt32
from feat_ref64 import ray_geom, ray_point
from grid_ref64 import _judge, _ref, same_bits              # noqa: F401  (same_bits: the GPU test's)
from lts_ref64 import FLIP_CAP, Q, xsqrt, xsum, xwhere        # noqa: F401
from shade_ref64 import DEC_K, FLOOR, U, Ref, compare        # noqa: F401

F32, F64, I32 = torch.float32, torch.float64, torch.int32
XC, DXR, LANES = 72, 64, 32
R_COL, R_ALT, R_NRM, R_XYZ, R_SIN, R_COS, R_VD, R_VS, R_VC = 0, 12, 24, 27, 30, 45, 60, 63, 66
TRIP_TILES = 2048 * 256 // LANES                             # esr_grid_for's default cap: tiles per trip


def f32(v):
    return float(torch.tensor(v, dtype=F32))


EPS = f32(1e-5)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def qx(t):
    return Q(t.double())


def qz(shape):
    return Q(torch.zeros(shape, dtype=F64))


# =======================================================================================================================
# positions and corners of the distinct tiles: binary32, bit for bit
# =======================================================================================================================
def positions(inp):
    """-> namespace: p [n,3], live [n], on [n] (the lane's tile carries the emissive group), unit [n,3], view [n,3], G (corners [n,1,..])"""
    r = inp["rec_ray"].long()
    live = r >= 0
    rc = r.clamp_min(0)
    start, dirv, _ = ray_geom(inp["rays_o"][rc], inp["rays_d"][rc], inp["lo"], inp["hi"], inp["near"], inp["stepdist"])
    p = ray_point(start, dirv, inp["stepdist"], inp["rec_step"])
    p = torch.where(live[:, None], p, torch.zeros_like(p))
    c = corners(p[:, None, :], inp["lo"], inp["hi"], inp["dims"])
    c.inb = c.inb & live[:, None, None]
    c.masked = ~live[:, None]
    unit = (p - inp["lo"]) / (inp["hi"] - inp["lo"])
    on = inp["on"].repeat_interleave(LANES)
    return SimpleNamespace(p=p, live=live, on=on, unit=unit, view=inp["viewdirs"][rc], G=c)


def _cl(grid):
    """channels-last [X,Y,Z,C] -> [C, cells]"""
    return grid.reshape(-1, grid.shape[-1]).T


def fetch_q(grid, G, W):
    """[C, cells] float64 -> Q [n, C]"""
    v = grid[:, G.cell[:, 0]] * G.inb[:, 0].to(grid.dtype)            # [C,n,8]
    q = xsum(Q(v) * Q(W.v[None, :, 0], W.E[None, :, 0]), -1, 8)
    return Q(q.v.T, q.E.T)


def xsqrt0(a):
    """xsqrt with the value 0 (and a zero derivative) at an exact 0"""
    pos = a.v.detach() > 0
    one = torch.ones_like(a.v)
    q = xsqrt(Q(torch.where(pos, a.v, one), a.E))
    return Q(torch.where(pos, q.v, torch.zeros_like(one)), torch.where(pos, q.E, a.E))


def normal_q(g, nrm):
    return g / (nrm + EPS)[:, None]


def fwd_q(inp, P, grids=None):
    g = grids or {k: _cl(inp[k].double()) for k in ("off_color", "emo_color", "grad_grid")}
    W = corner_w(P.G, "q")
    off, emo, gg = fetch_q(g["off_color"], P.G, W), fetch_q(g["emo_color"], P.G, W), fetch_q(g["grad_grid"], P.G, W)
    sq = gg * gg
    nrm = xsqrt0((sq[:, 0] + sq[:, 1]) + sq[:, 2])
    return SimpleNamespace(off=off, emo=emo, g=gg, nrm=nrm, normal=normal_q(gg, nrm), W=W)


def _tile(t):
    """[n, rows] -> [tiles, rows, 32]"""
    return t.reshape(-1, LANES, t.shape[1]).permute(0, 2, 1)


def _untile(t):
    """[tiles, rows, 32] -> [n, rows]"""
    return t.permute(0, 2, 1).reshape(-1, t.shape[1])


def _expand(inp, t):
    """per distinct tile -> per tile (the second-trip case repeats a small set of tiles)"""
    return t if inp.get("rep") is None else t[inp["rep"]]


def verify_fwd(inp, got, K):
    P = positions(inp)
    r = fwd_q(inp, P)
    n = P.live.numel()
    val, E = torch.zeros(n, XC, dtype=F64), torch.zeros(n, XC, dtype=F64)
    exact = torch.zeros(n, XC, dtype=torch.bool)
    want = torch.zeros(n, XC)

    def put(row, q):
        w = q.v.shape[1]
        val[:, row:row + w], E[:, row:row + w] = q.v.detach(), q.E
    put(R_COL, r.off)
    put(R_ALT, xwhere(P.on[:, None], r.emo, qz(r.emo.v.shape)))
    put(R_NRM, r.normal)
    u, v = P.unit.double(), P.view.double()
    two = torch.pow(2.0, torch.arange(5, dtype=F64))
    a = (u[:, :, None] * two).reshape(n, 15)
    for row, t in ((R_XYZ, u), (R_SIN, torch.sin(a)), (R_COS, torch.cos(a)), (R_VD, v), (R_VS, torch.sin(v)), (R_VC, torch.cos(v))):
        val[:, row:row + t.shape[1]] = t
        E[:, row:row + t.shape[1]] = 0.0 if row in (R_XYZ, R_VD) else 2.0
    for row, t in ((R_XYZ, P.unit), (R_VD, P.view)):
        exact[:, row:row + 3], want[:, row:row + 3] = True, t
    exact[:, 69:72] = True
    exact |= ~P.live[:, None]
    exact[:, R_ALT:R_ALT + 12] |= ~P.on[:, None]
    dead = ~P.live[:, None]
    val, E, want = [torch.where(dead, torch.zeros((), dtype=t.dtype), t) for t in (val, E, want)]
    gn_v, gn_E = torch.where(P.live, r.nrm.v.detach(), torch.zeros((), dtype=F64)), torch.where(P.live, r.nrm.E, torch.zeros((), dtype=F64))
    ex = lambda t: _expand(inp, t)
    T = lambda t: ex(_tile(t))
    L = lambda t: ex(t.reshape(-1, LANES)).reshape(-1)
    out = {"X": (T(val), T(E), T(dead.expand(n, XC))), "gnorm": (L(gn_v), L(gn_E), L(~P.live))}
    ref = _ref(out, {"X": (T(exact), T(want).contiguous())})
    ref.flips, ref.share = {}, 0.0
    got = {k: v.detach().cpu() for k, v in got.items()}
    worst, fails = _judge(ref, got, K)
    v, a, _ = out["X"]
    ratio = (got["X"].double().reshape(v.shape) - v).abs() / (U * a).clamp_min(1e-300) * (a > 0)
    ref.note = {name: round(float(ratio[:, r0:r1].max()), 3) for name, r0, r1 in ROW_GROUPS}
    return ref, worst, fails


ROW_GROUPS = (("colours", 0, 24), ("normal", 24, 27), ("sin / cos of the position", 30, 60), ("sin / cos of the view direction", 63, 69))


# ---- backward ---------------------------------------------------------------------------------------------------------
def bwd_values(inp, P, normal, nrm):
    """the explicit adjoint per sample: Q [n,12] for the off colours, [n,12] for the emissive colours (0 on off tiles), [n,3] for the
    gradient grid; `normal` [n,3] and `nrm` [n] are exact inputs (Q with E = 0)"""
    dO, dE = qx(_untile(inp["dX_off"])), qx(_untile(inp["dX_emo"]))
    on = P.on[:, None]
    v_off = dO[:, R_COL:R_COL + 12]
    v_emo = xwhere(on, dE[:, R_COL:R_COL + 12], qz((on.shape[0], 12)))
    dn = xwhere(on, dO[:, R_NRM:R_NRM + 3] + dE[:, R_NRM:R_NRM + 3], dO[:, R_NRM:R_NRM + 3])
    den = nrm + EPS
    g = normal * den[:, None]
    pr = dn * g
    dot = (pr[:, 0] + pr[:, 1]) + pr[:, 2]
    first = dn / den[:, None]
    pos = nrm.v.detach() > 0
    safe = Q(torch.where(pos, nrm.v, torch.ones_like(nrm.v)), nrm.E)
    second = (g * dot[:, None]) / ((den * den) * safe)[:, None]
    dg = xwhere(pos[:, None], first - second, first)
    return v_off, v_emo, dg


BWD_OUT = (("g_off_color", "off_color", 12), ("g_emo_color", "emo_color", 12), ("g_grad_grid", "grad_grid", 3))


def verify_bwd(inp, got, K):
    """got: X, gnorm (the forward's outputs the backward read) and the three gradient buffers"""
    P = positions(inp)
    got = {k: v.detach().cpu() for k, v in got.items()}
    first = (lambda t: t) if inp.get("rep") is None else (lambda t: t[inp["first"]])
    X = _untile(first(got["X"].reshape(-1, XC, LANES)))
    gn = first(got["gnorm"].reshape(-1, LANES)).reshape(-1)
    fails = []
    r = fwd_q(inp, P)
    for name, q, t in (("X rows 24-26", r.normal, X[:, R_NRM:R_NRM + 3]), ("gnorm", r.nrm, gn)):
        live = P.live if t.dim() == 1 else P.live[:, None]
        if not bool(torch.isfinite(t).all()) or bool((((t.double() - q.v.detach()).abs() > 16 * K * U * q.E + FLOOR) & live).any()):
            fails.append(f"{name}: the forward output the backward reads is far from the restatement")   # (a gate, not the bound)
    vals = bwd_values(inp, P, qx(X[:, R_NRM:R_NRM + 3]), qx(gn))
    W = corner_w(P.G, "q")
    out, b = {}, {}
    mult = None if inp.get("mult") is None else inp["mult"].repeat_interleave(LANES)
    for (name, grid, C), v in zip(BWD_OUT, vals):
        if name == "g_emo_color" and inp["null_emo"]:
            continue
        contrib = Q(v.v[:, None, None, :], v.E[:, None, None, :]) * Q(W.v[..., None], W.E[..., None])
        init = _cl(inp["grad0"][name].double())
        val, absref, touched = scatter_cells(inp, P.G, contrib, init, torch.zeros(1, dtype=torch.long), mult)
        shape = inp["grad0"][name].shape
        out[name] = (val.T.reshape(shape), absref.T.reshape(shape), None)
        b[name] = (~touched.T.reshape(shape), inp["grad0"][name])
    ref = _ref(out, b)
    ref.flips, ref.share = {}, 0.0
    worst, f2 = _judge(ref, {k: v for k, v in got.items() if k in out}, K)
    return ref, worst, fails + f2


# =======================================================================================================================
# the binary32 emulation
# =======================================================================================================================
def fetch32(grid, G, W, fused=True):
    v = grid[:, G.cell[:, 0]] * G.inb[:, 0].to(grid.dtype)            # [C,n,8]
    acc = torch.zeros(v.shape[:2])
    for k in range(8):
        acc = fma32(v[..., k], W[None, :, 0, k], acc)
    return acc.T


def emu_forward(inp, mut=None):
    P = positions(inp)
    n = P.live.numel()
    W = corner_w(P.G, "32")
    off, emo, g = (fetch32(_cl(inp[k]), P.G, W) for k in ("off_color", "emo_color", "grad_grid"))
    nrm = sqrt32((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
    X = torch.zeros(n, XC)
    on = P.on
    if mut == "tiles_on_off_by_one":
        on = _on_mutant(inp).repeat_interleave(LANES)
    if mut == "emo_rows_filled_on_off_tiles":
        on = torch.ones_like(on)
    X[:, R_COL:R_COL + 12] = off
    X[:, R_ALT:R_ALT + 12] = torch.where(on[:, None], emo, torch.zeros(()))
    X[:, R_NRM:R_NRM + 3] = g / (nrm if mut == "normal_without_eps" else nrm + EPS)[:, None]
    X[:, R_XYZ:R_XYZ + 3] = P.unit
    shift = 1 if mut == "pe_frequency_off_by_one" else 0
    a = (P.unit[:, :, None] * torch.pow(2.0, torch.arange(5) + shift)).reshape(n, 15)
    X[:, R_SIN:R_SIN + 15], X[:, R_COS:R_COS + 15] = torch.sin(a), torch.cos(a)
    src = P.unit if mut == "view_encoding_uses_position" else P.view
    X[:, R_VD:R_VD + 3], X[:, R_VS:R_VS + 3], X[:, R_VC:R_VC + 3] = P.view, torch.sin(src), torch.cos(src)
    if mut != "padding_lane_keeps_features":
        X = torch.where(P.live[:, None], X, torch.zeros(()))
        nrm = torch.where(P.live, nrm, torch.zeros(()))
    X = torch.nan_to_num(X, nan=9.0, posinf=9.0, neginf=9.0)            # (normal_without_eps at |g| = 0)
    return {"X": _tile(X), "gnorm": nrm}, P, W


def _on_mutant(inp):
    """`t <= tiles_on` on the distinct tiles: the first off tile counts as on"""
    on = inp["on"].clone()
    off = torch.nonzero(~on)
    if off.numel():
        on[int(off[0])] = True
    return on


def emu_fwd(inp, mut=None):
    out = emu_forward(inp, mut)[0]
    return {"X": _expand(inp, out["X"]), "gnorm": _expand(inp, out["gnorm"].reshape(-1, LANES)).reshape(-1)}


def emu_bwd(inp, mut=None):
    fw, P, W = emu_forward(inp)
    X, nrm = _untile(fw["X"]), fw["gnorm"]
    dO, dE = _untile(inp["dX_off"]), _untile(inp["dX_emo"])
    on = P.on
    if mut == "tiles_on_off_by_one":
        on = _on_mutant(inp).repeat_interleave(LANES)
    live = P.live
    G = P.G
    if mut == "padding_lane_keeps_features":                  # padding lanes scatter as ray 0, step 0
        alt = dict(inp, rec_ray=inp["rec_ray"].clamp_min(0), rec_step=torch.where(inp["rec_ray"] >= 0, inp["rec_step"], torch.zeros((), dtype=I32)))
        fw, P2, W = emu_forward(alt)
        X, nrm, G, live = _untile(fw["X"]), fw["gnorm"], P2.G, P2.live
    o = on[:, None]
    col_e = dE[:, R_ALT:R_ALT + 12] if mut == "emo_colour_gradient_from_rows_12" else dE[:, R_COL:R_COL + 12]
    v_off, v_emo = dO[:, R_COL:R_COL + 12], torch.where(o, col_e, torch.zeros(()))
    dn = dO[:, R_NRM:R_NRM + 3]
    if mut != "emo_normal_gradient_ignored":
        dn = dn + torch.where(o, dE[:, R_NRM:R_NRM + 3], torch.zeros(()))
    den = nrm + EPS
    g = X[:, R_NRM:R_NRM + 3] * den[:, None]
    dot = torch.zeros_like(den)
    for a in range(3):
        dot = dot + dn[:, a] * g[:, a]
    first = dn / den[:, None]
    pos = nrm > 0
    second = g * dot[:, None] / (den * den * torch.where(pos, nrm, torch.ones(())))[:, None]
    dg = first if mut == "normal_adjoint_drops_projection_term" else torch.where(pos[:, None], first - second, first)
    out = {}
    reps = None if inp.get("mult") is None else inp["mult"].repeat_interleave(LANES)
    for (name, grid, C), v in zip(BWD_OUT, (v_off, v_emo, dg)):
        if name == "g_emo_color" and inp["null_emo"]:
            continue
        dst = inp["grad0"][name].clone().reshape(-1, C)
        contrib = v[:, None, :] * W[:, 0, :, None]                                       # [n,8,C]
        keep = (G.inb[:, 0] & live[:, None])[..., None] & (contrib != 0)
        cell = (G.cell[:, 0][..., None] * C + torch.arange(C))[keep]
        if reps is None:
            dst.reshape(-1).index_add_(0, cell, contrib[keep])
        else:
            for m in torch.unique(reps).tolist():
                km = keep & (reps == m)[:, None, None]
                delta = torch.zeros_like(dst)
                delta.reshape(-1).index_add_(0, (G.cell[:, 0][..., None] * C + torch.arange(C))[km], contrib[km])
                for _ in range(m):
                    dst += delta
        out[name] = dst.reshape(inp["grad0"][name].shape)
    out["X"] = _expand(inp, fw["X"])
    out["gnorm"] = _expand(inp, fw["gnorm"].reshape(-1, LANES)).reshape(-1)
    return out


# =======================================================================================================================
# cases
# =======================================================================================================================
GRIDS = {"5x4x3": dict(dims=(5, 4, 3), lo=(0.0, 0.0, 0.0), hi=(4.0, 3.0, 2.0)),
         "16x16x16": dict(dims=(16, 16, 16), lo=(0.0, 0.0, 0.0), hi=(15.0, 15.0, 15.0))}
# name: grid, tiles, tiles_on, padding lanes at the end of the on block / of the off block, a whole padding tile (index or None)
_C = lambda grid, T, Ton, pad_on, pad_off, pad_tile: dict(grid=grid, T=T, Ton=Ton, pad_on=pad_on, pad_off=pad_off, pad_tile=pad_tile)
BIG_T = TRIP_TILES + 3
CASES = {
    "g543_T1_on0": _C("5x4x3", 1, 0, 0, 5, None),
    "g543_T1_on1": _C("5x4x3", 1, 1, 7, 0, None),
    "g543_T2_on1": _C("5x4x3", 2, 1, 3, 30, None),
    "g543_T9_on0": _C("5x4x3", 9, 0, 0, 1, 4),
    "g16_T2_on0": _C("16x16x16", 2, 0, 0, 0, None),
    "g16_T2_on2": _C("16x16x16", 2, 2, 31, 0, None),
    "g16_T9_on1": _C("16x16x16", 9, 1, 0, 9, None),
    "g16_T9_on4": _C("16x16x16", 9, 4, 11, 2, 2),
    "g16_T9_on9": _C("16x16x16", 9, 9, 1, 0, 8),
    "g16_second_trip": _C("16x16x16", BIG_T, TRIP_TILES // 2 + 5, 5, 6, None),
}
BIG = "g16_second_trip"
BIG_PERIOD = 7
N_RAYS = 24
_CACHE = {}


def _rec(D, gen, n_rays, max_step):
    ray = torch.sort(torch.randint(0, n_rays, (D * LANES,), generator=gen))[0].to(I32)
    step = torch.randint(0, max_step, (D * LANES,), generator=gen).to(I32)
    return ray.reshape(D, LANES), step.reshape(D, LANES)


def case(name):
    if name in _CACHE:
        return _CACHE[name]
    c = CASES[name]
    g = GRIDS[c["grid"]]
    dims = g["dims"]
    gen = _gen(900 + sum(map(ord, name)))
    lo, hi = torch.tensor(g["lo"], dtype=F32), torch.tensor(g["hi"], dtype=F32)
    T, Ton = c["T"], c["Ton"]
    big = T > 64
    # rays: lattice lines (points on nodes), then random rays through the box, some starting inside
    o, d = torch.zeros(N_RAYS, 3), torch.zeros(N_RAYS, 3)
    ctr, half = (hi + lo) / 2, (hi - lo) / 2
    for k in range(N_RAYS):
        if k < 3:
            o[k] = torch.tensor([[-2.0, 1.0, 1.0], [2.0, 5.0, 0.0], [1.0, 2.0, -3.0]][k])
            d[k] = torch.tensor([[2.0, 0.0, 0.0], [0.0, -1.0, 0.0], [0.0, 0.0, 1.0]][k])
        else:
            u = torch.randn(3, generator=gen)
            src = ctr + (0.5 if k % 4 == 0 else 2.5) * float(half.norm()) * u / u.norm()
            dst = ctr + half * (torch.rand(3, generator=gen) * 2 - 1)
            o[k], d[k] = src, (dst - src) * float(0.5 + torch.rand(1, generator=gen))
    view = d / d.norm(dim=-1, keepdim=True)
    max_step = int(max(dims)) + 3
    if big:                                                  # a period of tiles repeated; the distinct tiles: the period as on, then as off
        ray_p, step_p = _rec(BIG_PERIOD, gen, N_RAYS, max_step)
        ray_d, step_d = torch.cat([ray_p, ray_p]), torch.cat([step_p, step_p])
        t = torch.arange(T)
        rep = t % BIG_PERIOD + BIG_PERIOD * (t >= Ton).long()
        on = torch.arange(2 * BIG_PERIOD) < BIG_PERIOD
        D = 2 * BIG_PERIOD
    else:
        D = T
        ray_d, step_d = _rec(D, gen, N_RAYS, max_step)
        rep, on = None, torch.arange(T) < Ton
    census = set()
    # the first lanes: the three lattice rays, every step (points on nodes)
    ray_d[0, :9] = torch.tensor([0, 0, 0, 0, 1, 1, 1, 2, 2], dtype=I32)
    step_d[0, :9] = torch.tensor([0, 1, 2, 3, 0, 1, 2, 0, 1], dtype=I32)
    if not big:
        if c["pad_on"] and Ton:
            ray_d[Ton - 1, LANES - c["pad_on"]:] = -1
        if c["pad_off"] and T > Ton:
            ray_d[T - 1, LANES - c["pad_off"]:] = -1
        if c["pad_tile"] is not None:
            ray_d[c["pad_tile"]] = -1
    else:
        ray_d[BIG_PERIOD - 1, LANES - c["pad_on"]:] = -1
        ray_d[2 * BIG_PERIOD - 1, LANES - c["pad_off"]:] = -1
    X, Y, Z = dims
    gg = torch.randn(X, Y, Z, 3, generator=gen)
    z0, z1 = (2, 3) if X == 5 else (4, 8)
    gg[:z0] = 0.0                                            # |g| = 0: the dn / den branch
    gg[z0:z1] = torch.randn(z1 - z0, Y, Z, 3, generator=gen) * 1e-6   # |g| below eps
    inp = dict(name=name, dims=dims, lo=lo, hi=hi, near=0.0, stepdist=1.0, T=T, Ton=Ton, rays_o=o, rays_d=d, viewdirs=view,
               rec_ray=ray_d.reshape(-1), rec_step=step_d.reshape(-1), on=on, rep=rep, grad_grid=gg,
               off_color=torch.randn(X, Y, Z, 12, generator=gen), emo_color=torch.randn(X, Y, Z, 12, generator=gen), null_emo=Ton == 0)
    if rep is not None:
        inp["mult"] = torch.bincount(rep, minlength=D)
        inp["first"] = torch.stack([torch.nonzero(rep == k)[0, 0] for k in range(D)])
    wide = lambda: torch.sign(torch.randn(D, DXR, LANES, generator=gen)) * torch.pow(10.0, torch.rand(D, DXR, LANES, generator=gen) * 6 - 4)
    inp["dX_off"], inp["dX_emo"] = wide(), wide()
    for t in (inp["dX_off"], inp["dX_emo"]):
        t.reshape(-1)[::7] = 0.0
    inp["grad0"] = {"g_off_color": torch.randn(X, Y, Z, 12, generator=gen) * 0.1, "g_emo_color": torch.randn(X, Y, Z, 12, generator=gen) * 0.1,
                    "g_grad_grid": torch.randn(X, Y, Z, 3, generator=gen) * 0.1}
    # census, from the data
    P = positions(inp)
    f = emu_forward(inp)[0]
    nrm = f["gnorm"]
    some = P.G.inb[:, 0].any(-1)
    census |= {f"{T} tiles" if not big else "second trip", f"grid {c['grid']}",
               "tiles_on = 0" if Ton == 0 else "tiles_on = tiles_all" if Ton == T else "tiles_on = 1" if Ton == 1 else "tiles_on inside"}
    if bool((P.live & some & (nrm == 0)).any()):
        census.add("|g| = 0")
    if bool((P.live & (nrm > 0) & (nrm < EPS)).any()):
        census.add("|g| below eps")
    if bool((P.live & (nrm > 1e-2)).any()):
        census.add("|g| of order 1")
    node = ((P.G.w1[:, 0] == 0) | (P.G.w1[:, 0] == 1)).all(-1).all(-1)
    if bool((P.live & node & some).any()):
        census.add("point on a grid node")
    part = some & ~P.G.inb[:, 0].all(-1)
    if bool((P.live & part).any()):
        census.add("boundary cell with corners off the grid")
    if bool((P.live & ~some).any()):
        census.add("point with no corner on the grid")
    if bool((inp["dX_off"] == 0).any()) and bool((inp["dX_emo"] == 0).any()):
        census.add("zero entries in dX")
    if all(bool((t != 0).all()) for t in inp["grad0"].values()):
        census.add("non-zero initial gradient buffers")
    if Ton == 0:
        census.add("emo_color, dX_emo and g_emo_color NULL")
    # padding, from rec_ray as the kernel receives it: a block ends in padding lanes when its last tile has live lanes, then -1 only
    rr = full(inp)["rec_ray"].reshape(T, LANES) >= 0
    ends_padded = lambda t: bool(rr[t, 0]) and not bool(rr[t, -1]) and bool((rr[t, 1:] <= rr[t, :-1]).all())
    if Ton and ends_padded(Ton - 1):
        census.add("padding lanes at the end of the on block")
    if T > Ton and ends_padded(T - 1):
        census.add("padding lanes at the end of the off block")
    if bool((~rr).all(1).any()):
        census.add("a whole padding tile")
    inp["census"], inp["claims"] = census, set(census)
    _CACHE[name] = inp
    return inp


def full(inp):
    """the arrays as the kernel receives them (the repeated tile set expanded): rec_ray, rec_step [T*32], dX_off, dX_emo [T,64,32]"""
    ex = lambda t: _expand(inp, t).contiguous()
    return dict(rec_ray=ex(inp["rec_ray"].reshape(-1, LANES)).reshape(-1), rec_step=ex(inp["rec_step"].reshape(-1, LANES)).reshape(-1),
                dX_off=ex(inp["dX_off"]), dX_emo=ex(inp["dX_emo"]))


# op -> (case builder, case names, verify(inp, got, K) -> (ref, worst, fails), binary32 emulation, family, C entry points)
OPS = {
    "coarse_feat_fwd": (case, list(CASES), verify_fwd, emu_fwd, "coarse_feat_fwd", ("esr_coarse_feat_fwd",)),
    "coarse_feat_bwd": (case, list(CASES), verify_bwd, emu_bwd, "coarse_feat_bwd", ("esr_coarse_feat_fwd", "esr_coarse_feat_bwd")),
}


def build(op, name):
    return OPS[op][0](name)


def all_cases():
    return [(op, name) for op, spec in OPS.items() for name in spec[1]]


def is_big(name):
    return str(name) == BIG


def verify(op, inp, got, K):
    return OPS[op][2](inp, dict(got), K)


# K per family, for both test files: the next power of two at or above twice the worst ratio |gpu - ref| / (U absref) measured on the
# MI355X over every case of test_gpu_coarse_feat_ref64.py (printed under -s); the factor two leaves room for the order of the float atomics.
# The binary32 emulation reaches the same 0.970 on the backward and 0.309 on the forward, where its sin / cos are the host's: on the
# device the colours reach 0.309 as well, the normal 0.14, and the worst value is a sin / cos of the position.
K_FAMILY = {
    "coarse_feat_fwd": 2,   # measured worst 0.572 (esr_coarse_feat_fwd: sin / cos of the position; of the view direction 0.399)
    "coarse_feat_bwd": 2,   # 0.970 (esr_coarse_feat_bwd on the 16^3 grid; 0.945 on the 16 387-tile second trip)
}

# mutant of the emulation -> the ops it applies to; each must break the bound (or a bit expectation) on a small case of each of them
MUTANTS = {
    "emo_rows_filled_on_off_tiles": ["coarse_feat_fwd"],
    "padding_lane_keeps_features": ["coarse_feat_fwd", "coarse_feat_bwd"],
    "tiles_on_off_by_one": ["coarse_feat_fwd", "coarse_feat_bwd"],
    "normal_without_eps": ["coarse_feat_fwd"],
    "normal_adjoint_drops_projection_term": ["coarse_feat_bwd"],
    "emo_normal_gradient_ignored": ["coarse_feat_bwd"],
    "emo_colour_gradient_from_rows_12": ["coarse_feat_bwd"],
    "view_encoding_uses_position": ["coarse_feat_fwd"],
    "pe_frequency_off_by_one": ["coarse_feat_fwd"],
}
