"""Float64 restatement of the element-wise stages between the MLP passes, the compositing and the losses (csrc/shade.hip and
the two shade kernels of csrc/coarse.hip), with a plain binary32 torch emulation of each operation and the input builders
shared by tests/test_shade_ref64_host.py and tests/test_gpu_shade_ref64.py; never imported by the product path.

Written from the formulas the kernels cite (lin = softplus(emo) + softplus(off); the tone mapper's input [lin, sin(lin 2^i),
cos(lin 2^i)], i < 5; rgb = sigmoid(z); marched[ray] = sum of w * value over the ray's records; the trainer loss
mse(clamp(srgb + bg, 0, 1), gt) + w_lin mse(srgb_curve(clamp(lin + bg)), gt) + w_ent entropy(alphainv_last of the LAST ray)),
on the tile-major layout of DESIGN.md section 2: [tile][row][32 samples], rec_ray = -1 on padding slots.

Padding.  Outputs of kernels that read rec_ray are exactly 0 on every slot with rec_ray = -1.  Three outputs are not, and the
restatement follows the kernels there on purpose: `lin` and `Xt` of esr_fine_tone_in_fwd (the kernel has no rec_ray argument: a
padding lane holds softplus / sin / cos of whatever its pre-activations hold) and `rgb` of esr_fine_composite_fwd (sigmoid(zt) on
every slot).  For these only the padding ROWS (row 3; rows 33-47 of Xt) are asserted 0 and the padding lanes are checked as
values; nothing downstream reads them, every backward masks on rec_ray >= 0 (and is asserted 0 there).

Every entry returns, per output, (value, absref, zero): the float64 value, the error scale and the mask of slots that
must be exactly 0 (padding rows / lanes).  A value is checked as |got - value| <= K * U * absref + FLOOR, U = 2^-24.  absref is
the same computation on magnitudes plus first-order terms of the binary32 intermediates, E_q = a bound of |q_f32 - q| / U:
  expf, logf, log1pf, powf, sinf, cosf                 <= 2 ulp of the result
  sp  = softplus(z)  (z > 20: z, exact)                E = 6 sp          (expf 2, its effect through log1p <= 2, log1pf 2)
  sg  = sigmoid(z) = 1 / (1 + exp(-z))                 E = 6 sg          (expf 2, the sum 1, the divide 1, margin 2)
  sg' = sg (1 - sg)                                    E = E_sg |1 - 2 sg| + 3 sg' ;  from an exact column col: 3 col (1 - col)
  sp' = z > 20 ? 1 : sigmoid(z)                        E = 6 sg (0 above 20)
  lin = sp(off) [+ sp(emo) on the on-tiles]            E = E_sp(off) [+ E_sp(emo) + lin]
  sin(lin 2^i), cos(lin 2^i)                           E = 2^i E_lin + 2   (the product by 2^i is exact; |d sin / d a| <= 1)
  tone-in backward  d = w g_lin + dX_lin + sum_i 2^i (dXs_i Xc_i - dXc_i Xs_i),  M = the same on magnitudes (the X rows are
      INPUTS: the forward's stored rows): 11 products and 11 sums, every partial sum <= M      E = 16 M
      dz = d sp'(z)                                                                            absref = sp' 17 M + M E_sp'
  segment sum  out[ray] = init + sum_k a_k,  a_k = w_k v_k with E_a = |w_k| E_v + |a_k|,  M = sum |a_k|:
      one rounding per addend of the segment (n) and one float atomic per 64-slot wave chunk the ray touches (n_atom), each
      at a magnitude <= |init| + M                      absref = sum E_a + n M + n_atom (|init| + M)
  loss: derived next to the code (ref_loss); its sum takes one rounding per term of a thread (6 per ray and trip, + the
      entropy), 6 for the wave reduction and one atomic per wave.
  pair loss: d = a - b (1), inv = 1 / float(n_sel) (1), g = 2 d inv w (2): absref = 4 |g|; the value sums `trips` terms per
      thread, 6 + 2 reduction levels, one atomic per workgroup.
Scalars are the binary32 values the C ABI receives.

Decisions.  z > 20, gt >= 1, the entropy clamp of alphainv_last and sign(a - b) compare INPUTS (or an exactly rounded
difference): the restatement applies the kernel's documented convention (z == 20 takes the smooth branch, a clamp passes the
gradient at equality, sign(0) = 0) and they have no band.  ps in [0, 1], pl >= 0, l0 <= 1 under gt >= 1 and x <= 0.0031308
compare computed quantities: they are the restatement's own unless the caller forces the kernel's (`force`), and a forced
decision that differs must lie strictly inside DEC_K * U * E of its threshold (E = 0 for an exact quantity, so exact-boundary
inputs are never exempt).  Flips are counted in Ref.flips."""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import torch
import torch.nn.functional as F

F32, F64 = torch.float32, torch.float64
U = 2.0 ** -24
DEC_K = 16                       # as march_ref64.DEC_K
XT_ROWS, DX_ROWS = 48, 64
GRID_CAP = 2048                  # esr_grid_for's default cap (workgroups of 256)
ACT_BATCH_CAP, PAIR_CAP, PAIR_BATCH_CAP = 1024, 256, 128
ACT_MAX_JOBS, PAIR_MAX_JOBS = 4, 6


def f32(v):
    return float(torch.tensor(v, dtype=F32))


KNEE = f32(0.0031308)
A_LO = f32(1e-6)
A_HI = float(torch.tensor(1.0, dtype=F32) - torch.tensor(1e-6, dtype=F32))


@dataclass
class Ref:
    out: dict                                    # name -> (value, absref, zero mask or None)
    dec: dict = field(default_factory=dict)      # the decisions used
    band: dict = field(default_factory=dict)     # decision -> mask of values strictly inside the band
    flips: dict = field(default_factory=dict)
    share: float = 0.0                           # flipped values / values


# ---- elementary functions ---------------------------------------------------------------------------------------------
def softplus64(z):
    sp = F.softplus(z, beta=1, threshold=20)
    return sp, torch.where(z > 20, torch.zeros_like(sp), 6 * sp)


def sigmoid64(z):
    sg = torch.sigmoid(z)
    return sg, 6 * sg


def spgrad64(z):
    sg = torch.sigmoid(z)
    return torch.where(z > 20, torch.ones_like(sg), sg), torch.where(z > 20, torch.zeros_like(sg), 6 * sg)


def actgrad64(z, act):
    if act == 0:
        return spgrad64(z)
    sg = torch.sigmoid(z)
    return sg * (1 - sg), 6 * sg * (1 - 2 * sg).abs() + 3 * sg * (1 - sg)


def ch(t, c):
    """row c of a tile-major [T, rows, 32] tensor as a per-slot vector [T * 32]"""
    return t[:, c, :].reshape(-1)


def tm(cols, rows=4):
    """per-slot vectors -> tile-major [T, rows, 32], the remaining rows 0"""
    T = cols[0].numel() // 32
    o = torch.zeros(T, rows, 32, dtype=cols[0].dtype)
    for c, v in enumerate(cols):
        o[:, c, :] = v.reshape(T, 32)
    return o


def _rowmask(T, rows, from_row):
    m = torch.zeros(T, rows, 32, dtype=torch.bool)
    m[:, from_row:, :] = True
    return m


def _padmask(rec_ray, rows=4, n_live_rows=3):
    """zero mask of a [T, rows, 32] output: rows >= n_live_rows and every lane of a padding slot"""
    T = rec_ray.numel() // 32
    m = _rowmask(T, rows, n_live_rows)
    m |= (rec_ray.reshape(T, 1, 32) < 0)
    return m


def seg_counts(rec_ray, n_rays):
    """per ray: addends and float atomics (64-slot wave chunks touched)"""
    j = torch.arange(rec_ray.numel())
    live = rec_ray >= 0
    ray = rec_ray[live].long()
    n_add = torch.bincount(ray, minlength=n_rays)
    nchunk = rec_ray.numel() // 64 + 1
    key = torch.unique(ray * nchunk + j[live] // 64)
    n_atom = torch.bincount(key // nchunk, minlength=n_rays)
    return live, ray, n_add, n_atom


def seg_sum64(rec_ray, n_rays, a, E_a, init):
    """out[ray, c] = init + sum of a [S, C] over the ray's slots, with the absref of the module docstring"""
    live, ray, n_add, n_atom = seg_counts(rec_ray, n_rays)
    C_ = a.shape[1]
    s = torch.zeros(n_rays, C_, dtype=F64).index_add_(0, ray, a[live])
    M = torch.zeros(n_rays, C_, dtype=F64).index_add_(0, ray, a[live].abs())
    E = torch.zeros(n_rays, C_, dtype=F64).index_add_(0, ray, E_a[live])
    init = init.double()
    absref = E + n_add[:, None] * M + n_atom[:, None] * (init.abs() + M)
    return init + s, absref


# ---- fine tail --------------------------------------------------------------------------------------------------------
def lin64(z_off, z_emo, tiles_on, detach_off=False):
    """lin [T, 3, 32] and E_lin"""
    T = z_off.shape[0]
    on = (torch.arange(T) < tiles_on)[:, None, None]
    so, Eso = softplus64(z_off[:, :3].double())
    se, Ese = softplus64(z_emo[:, :3].double())
    if detach_off:
        so = torch.where(on, so.detach(), so)
    lin = torch.where(on, so + se, so)
    return lin, torch.where(on, Eso + Ese + lin.detach(), Eso)


def xt64(lin):
    """the 33 live rows of Xt [T, 33, 32] from lin [T, 3, 32]"""
    f = (2.0 ** torch.arange(5, dtype=F64))[None, None, :, None]
    a = lin[:, :, None, :] * f
    T = lin.shape[0]
    return torch.cat([lin, torch.sin(a).reshape(T, 15, 32), torch.cos(a).reshape(T, 15, 32)], 1)


def ref_tone_in_fwd(inp):
    T = inp["tiles_all"]
    lin, E = lin64(inp["z_off"], inp["z_emo"], inp["tiles_on"])
    X = torch.zeros(T, XT_ROWS, 32, dtype=F64)
    X[:, :33] = xt64(lin)
    EX = torch.zeros_like(X)
    EX[:, :3] = E
    f = (2.0 ** torch.arange(5, dtype=F64))[None, None, :, None]
    Es = (E[:, :, None, :] * f + 2).reshape(T, 15, 32)
    EX[:, 3:18], EX[:, 18:33] = Es, Es
    lin4 = torch.zeros(T, 4, 32, dtype=F64)
    lin4[:, :3] = lin
    E4 = torch.zeros_like(lin4)
    E4[:, :3] = E
    return Ref(out=dict(lin=(lin4, E4, _rowmask(T, 4, 3)), Xt=(X, EX, _rowmask(T, XT_ROWS, 33))))


def _tone_d64(inp):
    """d and M per channel [3][S] of the tone-in backward (0 on padding)"""
    rec_ray, w = inp["rec_ray"], inp["rec_w"].double()
    live = rec_ray >= 0
    ray = rec_ray.clamp_min(0).long()
    dX, X, g = inp["dXt"].double(), inp["Xt"].double(), inp["g_lin"].double()
    ds, Ms = [], []
    for c in range(3):
        d = w * g[ray, c] + ch(dX, c)
        M = (w * g[ray, c]).abs() + ch(dX, c).abs()
        for i in range(5):
            a, b = ch(dX, 3 + c * 5 + i) * ch(X, 18 + c * 5 + i), ch(dX, 18 + c * 5 + i) * ch(X, 3 + c * 5 + i)
            d = d + 2.0 ** i * (a - b)
            M = M + 2.0 ** i * (a.abs() + b.abs())
        ds.append(torch.where(live, d, torch.zeros_like(d)))
        Ms.append(torch.where(live, M, torch.zeros_like(M)))
    return ds, Ms


def ref_tone_in_bwd(inp):
    """fine: off is detached on the on-tiles -- dz is the emo gradient there and the off gradient on the off-tiles"""
    ds, Ms = _tone_d64(inp)
    T = inp["tiles_all"]
    on = (torch.arange(T) < inp["tiles_on"])[:, None].expand(T, 32).reshape(-1)
    v, a = [], []
    for c in range(3):
        z = torch.where(on, ch(inp["z_emo"], c), ch(inp["z_off"], c)).double()
        sp, Esp = spgrad64(z)
        v.append(ds[c] * sp)
        a.append(Ms[c] * (17 * sp + Esp))
    return Ref(out=dict(dz=(tm(v), tm(a), _padmask(inp["rec_ray"]))))


def ref_lts_tone_in_bwd(inp):
    """no detach: dz_off on every tile, dz_emo on the on-tiles (the rest of dz_emo keeps its contents)"""
    ds, Ms = _tone_d64(inp)
    T, t_on = inp["tiles_all"], inp["tiles_on"]
    out = {}
    for name, zsrc in (("dz_off", inp["z_off"]), ("dz_emo", inp["z_emo"])):
        v, a = [], []
        for c in range(3):
            sp, Esp = spgrad64(ch(zsrc, c).double())
            v.append(ds[c] * sp)
            a.append(Ms[c] * (17 * sp + Esp))
        out[name] = [tm(v), tm(a), _padmask(inp["rec_ray"])]
    v, a, z = out["dz_emo"]
    v[t_on:], a[t_on:], z[t_on:] = inp["dz_emo0"][t_on:].double(), 0.0, False
    return Ref(out={k: tuple(x) for k, x in out.items()})


def ref_composite_fwd(inp):
    """rgb = sigmoid(zt) on every slot (the kernel has no use for rec_ray there: padding lanes hold sigmoid of whatever
    zt holds; only row 3 is padding); srgb_marched / lin_marched accumulate"""
    T, n = inp["tiles_all"], inp["n_rays"]
    col, Ecol = sigmoid64(inp["zt"][:, :3].double())
    w = inp["rec_w"].double()[:, None]
    cs = torch.stack([ch(col, c) for c in range(3)], 1)
    Es = torch.stack([ch(Ecol, c) for c in range(3)], 1)
    ls = torch.stack([ch(inp["lin"], c) for c in range(3)], 1).double()
    srgb = seg_sum64(inp["rec_ray"], n, w * cs, w.abs() * Es + (w * cs).abs(), inp["srgb0"])
    linm = seg_sum64(inp["rec_ray"], n, w * ls, (w * ls).abs(), inp["lin0"])
    rgb = torch.zeros(T, 4, 32, dtype=F64)
    rgb[:, :3] = col
    E = torch.zeros_like(rgb)
    E[:, :3] = Ecol
    return Ref(out=dict(rgb=(rgb, E, _rowmask(T, 4, 3)), srgb_marched=(*srgb, None), lin_marched=(*linm, None)))


def ref_composite_bwd(inp):
    rec_ray, w = inp["rec_ray"], inp["rec_w"].double()
    live = rec_ray >= 0
    ray = rec_ray.clamp_min(0).long()
    gs, gl = inp["g_srgb"].double(), inp["g_lin"].double()
    dw, M, dz, Ez = 0, 0, [], []
    for c in range(3):
        col, l = ch(inp["rgb"], c).double(), ch(inp["lin"], c).double()
        a, b = gs[ray, c] * col, gl[ray, c] * l
        dw, M = dw + a + b, M + a.abs() + b.abs()
        d = w * gs[ray, c] * col * (1 - col)
        dz.append(torch.where(live, d, torch.zeros_like(d)))
        Ez.append(torch.where(live, 4 * d.abs(), torch.zeros_like(d)))
    z = torch.zeros_like(w)
    return Ref(out=dict(dweight=(torch.where(live, dw, z), torch.where(live, 8 * M, z), ~live),
                        dzt=(tm(dz), tm(Ez), _padmask(rec_ray))))


def ref_loss(inp, force=None):
    """mse(clamp(srgb + bg, 0, 1), gt) + w_lin mse(curve(clamp(lin + bg, 0[, 1 where gt >= 1])), gt), both means over 3 n, +
    w_ent H(clamp(alphainv_last[n - 1], 1e-6, 1 - 1e-6)), everything times `scale`; bg = alphainv_last * white_bg.
      inv = scale / (3 n)                    E = 2 inv
      bg                                     E = |bg| (0 for white_bg in {0, 1})
      ps = srgb + bg, pl = lin + bg          E = E_bg + |p| (0 when bg == 0: the input itself)
      ds = clamp(ps) - gt                    E = E_ps + |ds|;  term ds^2 inv: 2 |ds| E_ds inv + ds^2 (E_inv + 2 inv)
      gs = 2 ds inv inside [0, 1]            E = 2 inv E_ds + |gs| (E_inv / inv + 1)
      x = clamp(pl),  y = 12.92 x            E_y = 12.92 E_x + 2 |y|
                      y = 1.055 x^(1/2.4) - 0.055:  pw = x^(1/2.4), E_pw = pw (4 + |ln x| / 2.4) + (pw / (2.4 x)) E_x
                                             (powf 2 ulp, the rounded exponent, margin), E_y = 1.055 E_pw + 2 * 1.055 pw + |y| + 0.055
      dy = y - gt                            E = E_y + |dy|;  term w_lin dy^2 inv: w_lin (2 |dy| E_dy inv + dy^2 (E_inv + 3 inv))
      slope = 12.92 | (1.055 / 2.4) x^(1/2.4 - 1):  E = 12.92 | slope (6 + |ln x| + 0.59 E_x / x)
      g = 2 w_lin dy inv slope               E = |g| (E_inv / inv + 4) + 2 w_lin inv (|slope| E_dy + |dy| E_slope)
      g_last = white_bg sum_c (gs + g)       E = sum_c (E_gs + E_g) + 4 sum_c (|gs| + |g|)   (exactly 0 for white_bg == 0)
      entropy (last ray): q = 1 - p (E_q = q), A = p ln p (E = 3 |A|), B = q ln q (E = E_q (|ln q| + 1) + 3 |B|),
          value w (A + B): E = w (E_A + E_B + |A| + |B|) + 3 |value|;  gradient w (ln q - ln p), only for
          1e-6f <= alphainv_last <= 1 - 1e-6f: E = w (3 |ln p| + 3 |ln q| + E_q / q) + 3 |value|, + |g_last| for the sum
      loss = init + sum: E = sum of the terms' E + M (6 trips + 7 + 1) + n_waves (|init| + M), M = the sum of the terms."""
    n = inp["n_rays"]
    wb, w_lin, w_ent, scale = (f32(inp[k]) for k in ("white_bg", "w_lin", "w_ent", "scale"))
    sm, lm, al, gt = (inp[k].double() for k in ("srgb_m", "lin_m", "last", "rgbs"))
    inv = scale / (3.0 * n)
    E_inv = 2 * inv
    bg = (al * wb)[:, None]
    E_bg = torch.zeros_like(bg) if wb in (0.0, 1.0) else bg.abs()
    ps, pl = sm + bg, lm + bg
    E_ps = torch.where(bg != 0, E_bg + ps.abs(), torch.zeros_like(ps))
    E_pl = torch.where(bg != 0, E_bg + pl.abs(), torch.zeros_like(pl))
    sat = gt >= 1.0
    own = dict(inside=(ps >= 0) & (ps <= 1), pos=pl >= 0, le1=pl <= 1,
               low=torch.where(sat, pl.clamp(0, 1), pl.clamp_min(0)) <= KNEE)
    dist = dict(inside=torch.minimum(ps.abs(), (ps - 1).abs()), pos=pl.abs(), le1=(pl - 1).abs(), low=(pl - KNEE).abs())
    E_dec = dict(inside=E_ps, pos=E_pl, le1=E_pl, low=E_pl)
    band = {k: dist[k] < DEC_K * U * E_dec[k] for k in own}
    band["le1"] &= sat
    dec, flips = dict(own), {}
    if force is not None:
        for k in own:
            diff = force[k] != own[k]
            if k == "le1":
                diff &= sat
            assert not bool((diff & ~band[k]).any()), f"loss: forced `{k}` decisions off the boundary"
            flips[k] = int(diff.sum())
            dec[k] = force[k]
    # srgb term
    xs = torch.where(dec["inside"], ps, torch.where(ps < 0.5, torch.zeros_like(ps), torch.ones_like(ps)))   # outside: 0 or 1
    ds = xs - gt
    E_ds = E_ps + ds.abs()
    t_s = ds * ds * inv
    E_ts = 2 * ds.abs() * E_ds * inv + ds * ds * (E_inv + 2 * inv)
    gs = torch.where(dec["inside"], 2 * ds * inv, torch.zeros_like(ds))
    E_gs = torch.where(dec["inside"], 2 * inv * E_ds + gs.abs() * (E_inv / inv + 1), torch.zeros_like(ds))
    # linear term
    capped = sat & ~dec["le1"]
    x = torch.where(dec["pos"], pl, torch.zeros_like(pl))
    x = torch.where(capped, torch.ones_like(x), x)
    E_x = torch.where(dec["pos"] & ~capped, E_pl, torch.zeros_like(pl))
    low = dec["low"]
    xsafe = torch.where(low, torch.ones_like(x), x).clamp_min(1e-30)
    pw = xsafe ** (1 / 2.4)
    lnx = xsafe.log().abs()
    E_pw = pw * (4 + lnx / 2.4) + pw / (2.4 * xsafe) * E_x
    y = torch.where(low, 12.92 * x, 1.055 * pw - 0.055)
    E_y = torch.where(low, 12.92 * E_x + 2 * y.abs(), 1.055 * E_pw + 2.11 * pw + y.abs() + 0.055)
    dy = y - gt
    E_dy = E_y + dy.abs()
    t_l = w_lin * dy * dy * inv
    E_tl = w_lin * (2 * dy.abs() * E_dy * inv + dy * dy * (E_inv + 3 * inv))
    slope = torch.where(low, torch.full_like(x, 12.92), (1.055 / 2.4) * xsafe ** (1 / 2.4 - 1))
    E_sl = torch.where(low, torch.full_like(x, 12.92), slope * (6 + lnx + 0.59 * E_x / xsafe))
    g = 2 * w_lin * dy * inv * slope
    E_g = g.abs() * (E_inv / inv + 4) + 2 * w_lin * inv * (slope.abs() * E_dy + dy.abs() * E_sl)
    dead = capped | ~dec["pos"]
    g, E_g = torch.where(dead, torch.zeros_like(g), g), torch.where(dead, torch.zeros_like(g), E_g)
    gl = wb * (gs + g).sum(1)
    E_gl = ((E_gs + E_g).sum(1) + 4 * (gs.abs() + g.abs()).sum(1)) * (1.0 if wb != 0 else 0.0)
    # entropy of the last ray
    we = f32(w_ent * scale)
    a = al[n - 1]
    p = a.clamp(A_LO, A_HI)
    q = 1 - p
    A, B = p * p.log(), q * q.log()
    ent = -we * (A + B)
    E_ent = abs(we) * (3 * A.abs() + q * (q.log().abs() + 1) + 3 * B.abs() + A.abs() + B.abs()) + 3 * ent.abs()
    if bool((a >= A_LO) & (a <= A_HI)):
        ge = -we * (p.log() - q.log())
        E_ge = abs(we) * (3 * p.log().abs() + 3 * q.log().abs() + 1) + 3 * ge.abs()
        gl = gl.clone()
        E_gl = E_gl.clone()
        gl[n - 1] = gl[n - 1] + ge
        E_gl[n - 1] = E_gl[n - 1] + E_ge + gl[n - 1].abs()
    M = float(((t_s + t_l).sum() + ent.abs()).detach())
    trips = (n + GRID_CAP * 256 - 1) // (GRID_CAP * 256)
    n_waves = min((n + 63) // 64, GRID_CAP * 4)
    init = float(inp["loss0"])
    loss = init + float(((t_s + t_l).sum() + ent).detach())
    E_loss = float(((E_ts + E_tl).sum() + E_ent).detach()) + M * (6 * trips + 8) + n_waves * (abs(init) + M)
    out = dict(loss=(torch.tensor([loss], dtype=F64), torch.tensor([E_loss], dtype=F64), None),
               g_srgb=(gs.detach(), E_gs.detach(), None), g_lin=(g.detach(), E_g.detach(), None),
               g_last=(gl.detach(), E_gl.detach(), None))
    nflip = sum(flips.values())
    r = Ref(out=out, dec=dec, band=band, flips=flips, share=nflip / (3.0 * n))
    r.loss_t = (t_s + t_l).sum() + ent                     # (differentiable: the autograd check of the host test)
    return r


def force_from_outputs(ref_fn, inp, got, names=("g_srgb", "g_lin")):
    """The kernel's decisions as far as its outputs show them: a decision inside its band is taken as flipped where the
    flipped restatement is nearer to the kernel's value than the restatement's own."""
    r = ref_fn(inp)
    if not any(bool(b.any()) for b in r.band.values()):
        return r
    force = dict(r.dec)
    for k, b in r.band.items():
        if not bool(b.any()):
            continue
        alt = ref_fn(inp, {**r.dec, k: r.dec[k] ^ b})
        better = torch.zeros_like(b)
        for nm in names:
            g = got[nm].double().reshape(r.out[nm][0].shape)
            better |= (g - alt.out[nm][0]).abs() < (g - r.out[nm][0]).abs()
        force[k] = r.dec[k] ^ (b & better)
    return ref_fn(inp, force)


# ---- LTS tail ---------------------------------------------------------------------------------------------------------
def ref_composite3_fwd(inp):
    w = inp["rec_w"].double()[:, None]
    vs = torch.stack([ch(inp["v"], c) for c in range(3)], 1).double()
    o = seg_sum64(inp["rec_ray"], inp["n_rays"], w * vs, (w * vs).abs(), inp["out0"])
    return Ref(out=dict(out=(*o, None)))


def ref_composite3_bwd(inp):
    """dv = w g[ray] (+ dv on accumulate bit 0), dweight = sum_c g[ray, c] v[c] (+ dweight on bit 1); rows >= 3 of dv are
    not written"""
    rec_ray, w, acc = inp["rec_ray"], inp["rec_w"].double(), inp["accumulate"]
    live = rec_ray >= 0
    ray = rec_ray.clamp_min(0).long()
    g = inp["g"].double()
    dv, E = inp["dv0"].double().clone(), torch.zeros_like(inp["dv0"], dtype=F64)
    T = inp["tiles_all"]
    dw, M = torch.zeros_like(w), torch.zeros_like(w)
    for c in range(3):
        d = torch.where(live, w * g[ray, c], torch.zeros_like(w)).reshape(T, 32)
        base = dv[:, c, :] if acc & 1 else 0.0
        dv[:, c, :] = base + d
        E[:, c, :] = d.abs() + ((dv[:, c, :].abs() + d.abs()) if acc & 1 else 0.0)
        a = torch.where(live, g[ray, c] * ch(inp["v"], c).double(), torch.zeros_like(w))
        dw, M = dw + a, M + a.abs()
    dw0 = inp["dw0"].double()
    if acc & 2:
        dwv, Ew = dw0 + dw, 6 * M + dw0.abs() + M
    else:
        dwv, Ew = dw, 6 * M
    return Ref(out=dict(dv=(dv, E, None), dweight=(dwv, Ew, None)))


def ref_act(inp):
    """forward act(z) and backward g act'(z) on rows < n_ch of [T, rows, 32], the other rows 0"""
    z, act, n_ch = inp["z"].double(), inp["act"], inp["n_ch"]
    T, rows = z.shape[0], z.shape[1]
    zero = _rowmask(T, rows, n_ch)
    v, E = softplus64(z) if act == 0 else sigmoid64(z)
    d, Ed = actgrad64(z, act)
    g = inp["g"].double()
    fwd = (torch.where(zero, torch.zeros_like(v), v), torch.where(zero, torch.zeros_like(v), E), zero)
    bwd = (torch.where(zero, torch.zeros_like(v), g * d), torch.where(zero, torch.zeros_like(v), g.abs() * (Ed + d)), zero)
    return Ref(out=dict(fwd=fwd, bwd=bwd))


def act_job_grad64(job):
    """the gathered upstream gradient of a backward job [T, rows, 32] and its magnitude"""
    z = job["z"]
    T, rows = z.shape[0], z.shape[1]
    S = T * 32
    g = job["g_tile"].double().clone() if job.get("g_tile") is not None else torch.zeros(T, rows, 32, dtype=F64)
    M = g.abs()
    n_add = torch.zeros(T, rows, 32, dtype=F64) + (1.0 if job.get("g_tile") is not None else 0.0)
    if job.get("src") is not None:
        src = job["src"].double()
        k = job["inv"].long() if job.get("inv") is not None else torch.arange(S)
        ok = (k >= 0) & (k < src.shape[0])
        rowsv = torch.where(ok[:, None], src[k.clamp(0, max(src.shape[0] - 1, 0))], torch.zeros(S, src.shape[1], dtype=F64))
        for c in range(src.shape[1]):
            g[:, c, :] += rowsv[:, c].reshape(T, 32)
            M[:, c, :] += rowsv[:, c].abs().reshape(T, 32)
            n_add[:, c, :] += 1
    if job.get("pt1") is not None:
        p = job["pt1"].long() - 1
        ok = p >= 0
        for ex, c0 in job["ex"]:
            e = ex.double().reshape(ex.shape[0], -1)
            val = torch.where(ok[:, None], e[p.clamp_min(0)], torch.zeros(S, e.shape[1], dtype=F64))
            for c in range(e.shape[1]):
                g[:, c0 + c, :] += val[:, c].reshape(T, 32)
                M[:, c0 + c, :] += val[:, c].abs().reshape(T, 32)
                n_add[:, c0 + c, :] += 1
    return g, M, n_add


def ref_act_batch(inp):
    out = {}
    for i, job in enumerate(inp["jobs"]):
        z, act, n_ch = job["z"].double(), job["act"], job["n_ch"]
        T, rows = z.shape[0], z.shape[1]
        zero = _rowmask(T, rows, n_ch)
        if not job["bwd"]:
            v, E = softplus64(z) if act == 0 else sigmoid64(z)
        else:
            g, M, n_add = act_job_grad64(job)
            d, Ed = actgrad64(z, act)
            v, E = g * d, M * (Ed + d * (n_add + 1))
        zz = torch.zeros_like(v)
        out[f"job{i}"] = (torch.where(zero, zz, v), torch.where(zero, zz, E), zero)
    return Ref(out=out)


def pair_term64(job):
    """value, its absref pieces and the gradients of one pair-loss term"""
    a = job["a"].double()
    b = job["b"].double() if job.get("b") is not None else torch.zeros_like(a)
    rows, cols = a.shape
    sel = torch.ones(rows, dtype=torch.bool) if job.get("row_mask") is None else (job["row_mask"].long() == job["mask_value"])
    n_sel = (int(job["count"]) if job.get("count") is not None else rows) * cols
    inv = 1.0 / n_sel if n_sel > 0 else 0.0
    d = torch.where(sel[:, None], a - b, torch.zeros_like(a))
    E_d = d.abs() if job.get("b") is not None else torch.zeros_like(a)
    wv, wa, wb = f32(job["w_value"]), f32(job["w_a"]), f32(job["w_b"])
    if job["kind"] == 0:
        t, E_t, g = d * d * inv, 2 * d.abs() * E_d * inv + 3 * d * d * inv, 2 * d * inv
        E_g = 2 * inv * E_d + 2 * g.abs()
    else:
        t, E_t, g = d.abs() * inv, (E_d + 2 * d.abs()) * inv, torch.sign(d) * inv
        E_g = g.abs()
    return dict(value_t=wv * t.sum(), value=wv * float(t.sum().detach()), M=abs(wv) * float(t.sum().detach()),
                E=abs(wv) * float(E_t.sum().detach()),
                ga=((wa * g).detach(), (abs(wa) * (E_g + g.abs())).detach(), None),
                gb=((-wb * g).detach(), (abs(wb) * (E_g + g.abs())).detach(), None), total=rows * cols)


def _pair_sum_rounds(total, cap):
    blocks = max(1, min((total + 255) // 256, cap))
    trips = (total + blocks * 256 - 1) // (blocks * 256)
    return trips + 9, blocks


def ref_pair_loss(inp):
    return ref_pair_batch(dict(jobs=[inp], loss0=inp["loss0"]), cap=PAIR_CAP, single=True)


def ref_pair_batch(inp, cap=PAIR_BATCH_CAP, single=False):
    out, loss, E = {}, float(inp["loss0"]), 0.0
    init, Mtot, atoms = abs(float(inp["loss0"])), 0.0, 0
    for i, job in enumerate(inp["jobs"]):
        t = pair_term64(job)
        rounds, blocks = _pair_sum_rounds(t["total"], cap)
        loss += t["value"]
        E += t["E"] + t["M"] * (rounds + 1)
        Mtot += t["M"]
        atoms += blocks
        pre = "" if single else f"job{i}_"
        if job.get("want_ga", True):
            out[pre + "ga"] = t["ga"]
        if job.get("want_gb", True):
            out[pre + "gb"] = t["gb"]
    E += atoms * (init + Mtot)
    out["loss"] = (torch.tensor([loss], dtype=F64), torch.tensor([E], dtype=F64), None)
    return Ref(out=out)


# ---- coarse -----------------------------------------------------------------------------------------------------------
def coarse_rgb64(inp):
    T = inp["tiles_all"]
    on = (torch.arange(T) < inp["tiles_on"])[:, None, None]
    so, Eso = sigmoid64(inp["z_off"][:, :3].double())
    se, Ese = sigmoid64(inp["z_emo"][:, :3].double())
    rgb = torch.where(on, so + se, so)
    return rgb, torch.where(on, Eso + Ese + rgb.detach(), Eso)


def ref_coarse_shade_fwd(inp):
    """rgb = sigmoid(z_off) + [on] sigmoid(z_emo), 0 on padding lanes; srgb[ray] += w rgb"""
    T, rec_ray = inp["tiles_all"], inp["rec_ray"]
    rgb, E = coarse_rgb64(inp)
    zero = _padmask(rec_ray)
    r4, E4 = torch.zeros(T, 4, 32, dtype=F64), torch.zeros(T, 4, 32, dtype=F64)
    r4[:, :3], E4[:, :3] = rgb, E
    r4, E4 = torch.where(zero, torch.zeros_like(r4), r4), torch.where(zero, torch.zeros_like(r4), E4)
    w = inp["rec_w"].double()[:, None]
    cs = torch.stack([ch(r4, c) for c in range(3)], 1)
    Es = torch.stack([ch(E4, c) for c in range(3)], 1)
    srgb = seg_sum64(rec_ray, inp["n_rays"], w * cs, w.abs() * Es + (w * cs).abs(), inp["srgb0"])
    return Ref(out=dict(rgb=(r4, E4, zero), srgb_marched=(*srgb, None)))


def ref_coarse_shade_bwd(inp):
    """dz = g_srgb[ray] w sigmoid'(z) per head, dweight = g_srgb[ray] . rgb - g_wbg[ray]; rgb is the stored forward"""
    rec_ray, w = inp["rec_ray"], inp["rec_w"].double()
    T, t_on = inp["tiles_all"], inp["tiles_on"]
    live = rec_ray >= 0
    ray = rec_ray.clamp_min(0).long()
    g, gw = inp["g_srgb"].double(), inp["g_wbg"].double()
    z0 = torch.zeros_like(w)
    out = {}
    for name, zsrc in (("dz_off", inp["z_off"]), ("dz_emo", inp["z_emo"])):
        v, a = [], []
        for c in range(3):
            d, Ed = actgrad64(ch(zsrc, c).double(), 1)
            x = torch.where(live, g[ray, c] * w, z0)
            v.append(x * d)
            a.append(x.abs() * (Ed + 2 * d))
        out[name] = [tm(v), tm(a), _padmask(rec_ray)]
    v, a, z = out["dz_emo"]
    v[t_on:], a[t_on:], z[t_on:] = inp["dz_emo0"][t_on:].double(), 0.0, False
    dw, M = -gw[ray], gw[ray].abs()
    for c in range(3):
        x = g[ray, c] * ch(inp["rgb"], c).double()
        dw, M = dw + x, M + x.abs()
    out = {k: tuple(x) for k, x in out.items()}
    out["dweight"] = (torch.where(live, dw, z0), torch.where(live, 7 * M, z0), ~live)
    return Ref(out=out)


# ---- evaluation -------------------------------------------------------------------------------------------------------
def ref_eval_aux(inp):
    """aux [T, 8, 32]: rows 0-2 ((n @ rt) * (1, -1, -1) + 1) / 2, row 4 step * stepdist, the rest and padding lanes 0"""
    rec_ray, X = inp["rec_ray"], inp["X"].double()
    T = inp["tiles_all"]
    live = rec_ray >= 0
    rt = torch.tensor([f32(v) for v in inp["rt"]], dtype=F64).reshape(3, 3)
    nv = torch.stack([ch(X, r) for r in inp["nrow"]], 1)
    dot, M = nv @ rt, nv.abs() @ rt.abs()
    sign = torch.tensor([1.0, -1.0, -1.0], dtype=F64)
    v = (dot * sign + 1) / 2
    E = (5 * M + M + 1) / 2 + v.abs()
    depth = inp["rec_step"].double() * f32(inp["stepdist"])
    z0 = torch.zeros(T * 32, dtype=F64)
    cols = [torch.where(live, v[:, c], z0) for c in range(3)] + [z0, torch.where(live, depth, z0)]
    Es = [torch.where(live, E[:, c], z0) for c in range(3)] + [z0, torch.where(live, depth.abs(), z0)]
    zero = _padmask(rec_ray, 8, 8)
    zero[:, 3], zero[:, 5:] = True, True
    return Ref(out=dict(aux=(tm(cols, 8), tm(Es, 8), zero)))


def ref_eval_disp(inp):
    """depth = depth3[:, 0] (a copy); disp = 1 / (depth + alphainv_last * far)"""
    d, al, far = inp["depth3"][:, 0].double(), inp["last"].double(), f32(inp["far"])
    den = d + al * far
    E_den = (al * far).abs() + den.abs()
    disp = 1 / den
    return Ref(out=dict(depth=(d, torch.zeros_like(d), None), disp=(disp, E_den / den ** 2 + 2 * disp.abs(), None)))


# =======================================================================================================================
# binary32 emulations (plain torch on the CPU) and their mutants
# =======================================================================================================================
def _sp32(z):
    return torch.where(z > 20, z, torch.log1p(torch.exp(torch.clamp(z, max=20.0))))


def _sg32(z):
    return 1.0 / (1.0 + torch.exp(-z))


def _spg32(z, mut=None):
    if mut == "spgrad_nobranch":          # d/dz log1p(exp(z)) as written: the sigmoid form is the branch's value to < 2^-24
        e = torch.exp(z)
        return e / (1.0 + e)
    return torch.where(z > 20, torch.ones_like(z), _sg32(z))


def _on32(T, tiles_on, mut):
    return torch.arange(T) < (tiles_on + 1 if mut == "tiles_on_off_by_one" else tiles_on)


def emu_tone_in_fwd(inp, mut=None):
    T = inp["tiles_all"]
    on = _on32(T, inp["tiles_on"], mut)[:, None, None]
    lin3 = _sp32(inp["z_off"][:, :3])
    lin3 = torch.where(on, _sp32(inp["z_emo"][:, :3]) + lin3, lin3)
    lin = torch.zeros(T, 4, 32)
    lin[:, :3] = lin3
    X = torch.zeros(T, XT_ROWS, 32)
    X[:, :3] = lin3
    f = (2.0 ** torch.arange(5))[None, None, :, None]
    a = lin3[:, :, None, :] * f
    sn, cs = torch.sin(a), torch.cos(a)
    if mut == "sin_cos_swapped":
        sn, cs = sn.clone(), cs.clone()
        sn[:, 1], cs[:, 1] = torch.cos(a[:, 1]), torch.sin(a[:, 1])
    X[:, 3:18], X[:, 18:33] = sn.reshape(T, 15, 32), cs.reshape(T, 15, 32)
    return dict(lin=lin, Xt=X)


def _emu_tone_d(inp, mut):
    rec_ray, w = inp["rec_ray"], inp["rec_w"]
    live = rec_ray >= 0
    ray = rec_ray.clamp_min(0).long()
    dX, X, g = inp["dXt"], inp["Xt"], inp["g_lin"]
    ds = []
    for c in range(3):
        d = w * g[ray, c] + ch(dX, c)
        for i in range(5):
            f = 1.0 if (mut == "freq_factor_dropped" and i == 2) else 2.0 ** i
            s_, c_ = 3 + c * 5 + i, 18 + c * 5 + i
            if mut == "sin_cos_swapped" and c == 1:
                s_, c_ = c_, s_
            d = d + f * (ch(dX, 3 + c * 5 + i) * ch(X, c_) - ch(dX, 18 + c * 5 + i) * ch(X, s_))
        ds.append(torch.where(live, d, torch.zeros_like(d)))
    return ds


def emu_tone_in_bwd(inp, mut=None):
    ds = _emu_tone_d(inp, mut)
    T = inp["tiles_all"]
    on = _on32(T, inp["tiles_on"], mut)[:, None].expand(T, 32).reshape(-1)
    return dict(dz=tm([ds[c] * _spg32(torch.where(on, ch(inp["z_emo"], c), ch(inp["z_off"], c)), mut) for c in range(3)]))


def emu_lts_tone_in_bwd(inp, mut=None):
    ds = _emu_tone_d(inp, mut)
    T = inp["tiles_all"]
    t_on = min(T, inp["tiles_on"] + 1) if mut == "tiles_on_off_by_one" else inp["tiles_on"]
    dz_off = tm([ds[c] * _spg32(ch(inp["z_off"], c), mut) for c in range(3)])
    dz_emo = inp["dz_emo0"].clone()
    dz_emo[:t_on] = tm([ds[c] * _spg32(ch(inp["z_emo"], c), mut) for c in range(3)])[:t_on]
    return dict(dz_off=dz_off, dz_emo=dz_emo)


def emu_seg_sum(rec_ray, n_rays, a, init, mut=None, pad_a=None):
    """per-(ray, 64-slot chunk) partial sums in binary32, then one addition per chunk into init"""
    S = rec_ray.numel()
    j = torch.arange(S)
    ray = rec_ray.long().clone()
    a = a.clone()
    extra_ray, extra_a = None, None
    if mut == "segment_leaks_a_lane":           # the first lane of a segment also takes its left neighbour's addend
        first = (ray >= 0) & (j % 64 != 0)
        first[1:] &= (ray[:-1] >= 0) & (ray[:-1] != ray[1:])
        first[0] = False
        idx = torch.nonzero(first)[:, 0]
        extra_ray, extra_a = ray[idx], a[idx - 1]
    if mut == "wave_last_lane_dropped":
        ray[j % 64 == 63] = -1
    if mut == "padding_lanes_contribute":       # a padding lane joins the ray on its left with its own rec_w
        prev = torch.cummax(torch.where(ray >= 0, j, torch.full_like(j, -1)), 0).values
        pad = (ray < 0) & (prev >= 0)
        ray = torch.where(pad, ray[prev.clamp_min(0)], ray)
        a = torch.where(pad[:, None], pad_a, a)
    live = ray >= 0
    nchunk = S // 64 + 1
    key = ray[live] * nchunk + j[live] // 64
    uk, invk = torch.unique(key, return_inverse=True)
    part = torch.zeros(uk.numel(), a.shape[1]).index_add_(0, invk, a[live])
    out = init.clone().index_add_(0, uk // nchunk, part)
    if extra_ray is not None and extra_ray.numel():
        out.index_add_(0, extra_ray, extra_a)
    return out


def emu_composite_fwd(inp, mut=None):
    T = inp["tiles_all"]
    col = _sg32(inp["zt"][:, :3])
    rgb = torch.zeros(T, 4, 32)
    rgb[:, :3] = col
    live = (inp["rec_ray"] >= 0)[:, None]
    w = inp["rec_w"][:, None]
    cs = torch.stack([ch(rgb, c) for c in range(3)], 1)
    ls = torch.stack([ch(inp["lin"], c) for c in range(3)], 1)
    wz = torch.where(live, w, torch.zeros_like(w))
    return dict(rgb=rgb, srgb_marched=emu_seg_sum(inp["rec_ray"], inp["n_rays"], wz * cs, inp["srgb0"], mut, w * cs),
                lin_marched=emu_seg_sum(inp["rec_ray"], inp["n_rays"], wz * ls, inp["lin0"], mut, w * ls))


def emu_composite_bwd(inp, mut=None):
    rec_ray, w = inp["rec_ray"], inp["rec_w"]
    live = rec_ray >= 0
    ray = rec_ray.clamp_min(0).long()
    dw, dz = torch.zeros_like(w), []
    for c in range(3):
        col, l = ch(inp["rgb"], c), ch(inp["lin"], c)
        gs = inp["g_srgb"][ray, c]
        dw = dw + (gs * col + inp["g_lin"][ray, c] * l)
        dz.append(torch.where(live, w * gs * col * (1.0 - col), torch.zeros_like(w)))
    return dict(dweight=torch.where(live, dw, torch.zeros_like(w)), dzt=tm(dz))


def emu_loss(inp, mut=None):
    n = inp["n_rays"]
    t32 = lambda v: torch.tensor(v, dtype=F32)
    wb, w_lin, w_ent, scale = (t32(inp[k]) for k in ("white_bg", "w_lin", "w_ent", "scale"))
    inv = scale / (3.0 * t32(float(n)))
    if mut != "scale_not_on_entropy":
        w_ent = w_ent * scale
    sm, lm, al, gt = inp["srgb_m"], inp["lin_m"], inp["last"], inp["rgbs"]
    bg = (al * wb)[:, None]
    ps = sm + bg
    xs = ps.clamp(0.0, 1.0)
    t_s = (xs - gt) * (xs - gt) * inv
    gs = torch.where((ps >= 0) & (ps <= 1), 2.0 * (xs - gt) * inv, torch.zeros_like(ps))
    pl = lm + bg
    l0 = pl.clamp_min(0.0)
    sat = gt >= 1.0
    x = torch.where(sat, l0.clamp(max=1.0), l0)
    low = x <= KNEE
    xs_ = torch.where(low, torch.ones_like(x), x)
    y = torch.where(low, 12.92 * x, 1.055 * torch.pow(xs_, t32(1 / 2.4)) - 0.055)
    t_l = w_lin * (y - gt) * (y - gt) * inv
    g = w_lin * 2.0 * (y - gt) * inv
    g = g * torch.where(low, torch.full_like(x, 12.92), t32(1.055) * t32(1 / 2.4) * torch.pow(xs_, t32(1 / 2.4) - 1.0))
    if mut != "saturated_clamp_passes_gradient":
        g = torch.where(sat & ~(l0 <= 1.0), torch.zeros_like(g), g)
    g = torch.where(pl >= 0, g, torch.zeros_like(g))
    gl = ((gs + g) * wb).sum(1)
    r = 0 if mut == "entropy_on_ray_0" else n - 1
    a = al[r]
    p = a.clamp(A_LO, A_HI)
    ent = w_ent * -(p * p.log() + (1.0 - p) * (1.0 - p).log())
    if bool((a >= A_LO) & (a <= A_HI)):
        gl = gl.clone()
        gl[r] = gl[r] + w_ent * -(p.log() - (1.0 - p).log())
    loss = inp["loss0"].reshape(1) + ((t_s + t_l).sum() + ent).reshape(1)
    return dict(loss=loss, g_srgb=gs, g_lin=g, g_last=gl)


def emu_composite3_fwd(inp, mut=None):
    live = (inp["rec_ray"] >= 0)[:, None]
    w = inp["rec_w"][:, None]
    vs = torch.stack([ch(inp["v"], c) for c in range(3)], 1)
    return dict(out=emu_seg_sum(inp["rec_ray"], inp["n_rays"], torch.where(live, w, torch.zeros_like(w)) * vs, inp["out0"], mut,
                                w * vs))


def emu_composite3_bwd(inp, mut=None):
    rec_ray, w, acc = inp["rec_ray"], inp["rec_w"], inp["accumulate"]
    if mut == "accumulate_bits_exchanged":
        acc = ((acc & 1) << 1) | ((acc & 2) >> 1)
    live = rec_ray >= 0
    ray = rec_ray.clamp_min(0).long()
    T = inp["tiles_all"]
    dv, dw = inp["dv0"].clone(), torch.zeros_like(w)
    for c in range(3):
        d = torch.where(live, w * inp["g"][ray, c], torch.zeros_like(w)).reshape(T, 32)
        dv[:, c, :] = dv[:, c, :] + d if acc & 1 else d
        dw = dw + torch.where(live, inp["g"][ray, c] * ch(inp["v"], c), torch.zeros_like(w))
    return dict(dv=dv, dweight=inp["dw0"] + dw if acc & 2 else dw)


def _emu_actgrad(z, act, mut=None):
    if act == 0:
        return _spg32(z, mut)
    sg = _sg32(z)
    return sg * (1.0 - sg)


def emu_act(inp, mut=None):
    z, act = inp["z"], inp["act"]
    zero = _rowmask(z.shape[0], z.shape[1], inp["n_ch"])
    v = _sp32(z) if act == 0 else _sg32(z)
    b = inp["g"] * _emu_actgrad(z, act, mut)
    return dict(fwd=torch.where(zero, torch.zeros_like(v), v), bwd=torch.where(zero, torch.zeros_like(v), b))


def _emu_act_gather32(job, mut=None):
    """the upstream gradient of a backward job gathered in binary32: tile-major part, then the src row, then the extras"""
    z = job["z"]
    T, rows = z.shape[0], z.shape[1]
    g = job["g_tile"].clone() if job.get("g_tile") is not None else torch.zeros(T, rows, 32)
    slot = (torch.arange(T)[:, None] * 32 + torch.arange(32)[None]).reshape(-1)
    if job.get("src") is not None:
        src = job["src"]
        k = slot if (job.get("inv") is None or mut == "act_gather_ignores_inverse_map") else job["inv"].long()[slot]
        ok = (k >= 0) & (k < src.shape[0])
        for c in range(src.shape[1]):
            add = torch.zeros(T * 32)
            add[ok] = src[k[ok], c]
            g[:, c, :] = g[:, c, :] + add.reshape(T, 32)
    if job.get("pt1") is not None:
        p = job["pt1"].long()[slot] - 1
        ok = p >= 0
        for ex, c0 in job["ex"]:
            e = ex.reshape(ex.shape[0], -1)
            for c in range(e.shape[1]):
                add = torch.zeros(T * 32)
                add[ok] = e[p[ok], c]
                g[:, c0 + c, :] = g[:, c0 + c, :] + add.reshape(T, 32)
    return g


def emu_act_batch(inp, mut=None):
    out = {}
    for i, job in enumerate(inp["jobs"]):
        z, act = job["z"], job["act"]
        zero = _rowmask(z.shape[0], z.shape[1], job["n_ch"])
        if not job["bwd"]:
            v = _sp32(z) if act == 0 else _sg32(z)
        else:
            v = _emu_act_gather32(job, mut) * _emu_actgrad(z, act, mut)
        out[f"job{i}"] = torch.where(zero, torch.zeros_like(v), v)
    return out


def _emu_pair_term(job, mut):
    a = job["a"]
    b = job["b"] if job.get("b") is not None else torch.zeros_like(a)
    rows, cols = a.shape
    sel = torch.ones(rows, dtype=torch.bool) if job.get("row_mask") is None else (job["row_mask"].long() == job["mask_value"])
    n_sel = (int(job["count"]) if (job.get("count") is not None and mut != "pair_divides_by_total") else rows) * cols
    inv = torch.tensor(1.0 / n_sel if n_sel > 0 else 0.0, dtype=F32)
    d = torch.where(sel[:, None], a - b, torch.zeros_like(a))
    if job["kind"] == 0:
        t, g = d * d * inv, 2.0 * d * inv
    else:
        t, g = d.abs() * inv, torch.sign(d) * inv
    t32 = lambda v: torch.tensor(v, dtype=F32)
    return t.sum() * t32(job["w_value"]), t32(job["w_a"]) * g, -t32(job["w_b"]) * g


def emu_pair_loss(inp, mut=None):
    v, ga, gb = _emu_pair_term(inp, mut)
    out = dict(loss=inp["loss0"].reshape(1) + v.reshape(1))
    if inp.get("want_ga", True):
        out["ga"] = ga
    if inp.get("want_gb", True):
        out["gb"] = gb
    return out


def emu_pair_batch(inp, mut=None):
    out, loss = {}, inp["loss0"].reshape(1).clone()
    for i, job in enumerate(inp["jobs"]):
        v, ga, gb = _emu_pair_term(job, mut)
        loss = loss + v.reshape(1)
        if job.get("want_ga", True):
            out[f"job{i}_ga"] = ga
        if job.get("want_gb", True):
            out[f"job{i}_gb"] = gb
    out["loss"] = loss
    return out


def emu_coarse_shade_fwd(inp, mut=None):
    T, rec_ray = inp["tiles_all"], inp["rec_ray"]
    on = _on32(T, inp["tiles_on"], mut)[:, None, None]
    v = _sg32(inp["z_off"][:, :3])
    v = torch.where(on, v + _sg32(inp["z_emo"][:, :3]), v)
    rgb = torch.zeros(T, 4, 32)
    rgb[:, :3] = v
    rgb_all = rgb
    rgb = torch.where(_padmask(rec_ray), torch.zeros_like(rgb), rgb)
    w = inp["rec_w"][:, None]
    cs = torch.stack([ch(rgb, c) for c in range(3)], 1)
    ca = torch.stack([ch(rgb_all, c) for c in range(3)], 1)
    return dict(rgb=rgb, srgb_marched=emu_seg_sum(rec_ray, inp["n_rays"], w * cs, inp["srgb0"], mut, w * ca))


def emu_coarse_shade_bwd(inp, mut=None):
    rec_ray, w = inp["rec_ray"], inp["rec_w"]
    T = inp["tiles_all"]
    t_on = min(T, inp["tiles_on"] + 1) if mut == "tiles_on_off_by_one" else inp["tiles_on"]
    live = rec_ray >= 0
    ray = rec_ray.clamp_min(0).long()
    z0 = torch.zeros_like(w)
    res = {}
    for name, zsrc in (("dz_off", inp["z_off"]), ("dz_emo", inp["z_emo"])):
        res[name] = tm([torch.where(live, inp["g_srgb"][ray, c] * w, z0) * _emu_actgrad(ch(zsrc, c), 1) for c in range(3)])
    dz_emo = inp["dz_emo0"].clone()
    dz_emo[:t_on] = res["dz_emo"][:t_on]
    dw = z0
    for c in range(3):
        dw = dw + inp["g_srgb"][ray, c] * ch(inp["rgb"], c)
    return dict(dz_off=res["dz_off"], dz_emo=dz_emo, dweight=torch.where(live, dw - inp["g_wbg"][ray], z0))


def emu_eval_aux(inp, mut=None):
    rec_ray, X = inp["rec_ray"], inp["X"]
    live = rec_ray >= 0
    rt = torch.tensor(inp["rt"], dtype=F32).reshape(3, 3)
    nv = torch.stack([ch(X, r) for r in inp["nrow"]], 1)
    sign = torch.tensor([1.0, -1.0, -1.0])
    v = ((nv[:, 0:1] * rt[0] + nv[:, 1:2] * rt[1] + nv[:, 2:3] * rt[2]) * sign + 1.0) / 2.0
    z0 = torch.zeros(rec_ray.numel())
    depth = inp["rec_step"].float() * torch.tensor(inp["stepdist"], dtype=F32)
    return dict(aux=tm([torch.where(live, v[:, c], z0) for c in range(3)] + [z0, torch.where(live, depth, z0)], 8))


def emu_eval_disp(inp, mut=None):
    d = inp["depth3"][:, 0].clone()
    return dict(depth=d, disp=1.0 / (d + inp["last"] * torch.tensor(inp["far"], dtype=F32)))


# =======================================================================================================================
# the comparison
# =======================================================================================================================
FLOOR = 1e-30


def compare(ref: Ref, got: dict, K: float):
    """worst |got - value| / (U absref) over the outputs and the list of failures (empty: the bound holds)"""
    worst, fails = 0.0, []
    assert set(got) == set(ref.out), (sorted(got), sorted(ref.out))
    for name, (val, absref, zero) in ref.out.items():
        g = got[name].detach().cpu().double().reshape(val.shape)
        if not bool(torch.isfinite(g).all()):
            fails.append(f"{name}: non-finite values")
            continue
        if zero is not None and bool((g[zero] != 0).any()):
            fails.append(f"{name}: {int((g[zero] != 0).sum())} padding values are not exactly 0")
        err = (g - val).abs()
        bad = err > K * U * absref + FLOOR
        ratio = torch.where(absref > 0, (err - FLOOR).clamp_min(0) / (U * absref).clamp_min(1e-300), torch.zeros_like(err))
        worst = max(worst, float(ratio.max()) if ratio.numel() else 0.0)
        if bool(bad.any()):
            i = int(torch.nonzero(bad.reshape(-1))[0])
            fails.append(f"{name}: {int(bad.sum())} of {bad.numel()} values outside the bound; first at flat index {i}: got "
                         f"{float(g.reshape(-1)[i]):.9g}, ref {float(val.reshape(-1)[i]):.9g}, "
                         f"err / (U absref) = {float(err.reshape(-1)[i]) / max(U * float(absref.reshape(-1)[i]), 1e-300):.3g}")
    return worst, fails


# =======================================================================================================================
# input builders (shared by the host test and the GPU test)
# =======================================================================================================================
def layout(on_counts, off_counts, pad_tiles_on=0, pad_tiles_off=0):
    """Record layout as the march leaves it: on rays first from slot 0, off rays from the next multiple of 32, padding -1;
    pad_tiles_*: all-padding tiles appended to a group.  Ray ids: on rays 0.., then off rays."""
    n_on = sum(on_counts)
    t_on = (n_on + 31) // 32 + pad_tiles_on
    n_off = sum(off_counts)
    T = t_on + (n_off + 31) // 32 + pad_tiles_off
    rec = torch.full((T * 32,), -1, dtype=torch.int32)
    pos, r = 0, 0
    for cnt in on_counts:
        rec[pos:pos + cnt] = r
        pos, r = pos + cnt, r + 1
    pos = t_on * 32
    for cnt in off_counts:
        rec[pos:pos + cnt] = r
        pos, r = pos + cnt, r + 1
    return dict(rec_ray=rec, n_rays=r, tiles_on=t_on, tiles_all=T, n_on=n_on)


def tile_census(lay):
    """the classes a layout reaches"""
    rec, T, t_on, n = lay["rec_ray"], lay["tiles_all"], lay["tiles_on"], lay["n_rays"]
    live, ray, n_add, n_atom = seg_counts(rec, n)
    c = set()
    c.add("tiles_all=1" if T == 1 else "tiles_all=2" if T == 2 else "tiles_all odd" if T % 2 else "tiles_all even")
    c.add("tiles_on=0" if t_on == 0 else "tiles_on=tiles_all" if t_on == T else "tiles_on odd" if t_on % 2 else "tiles_on even")
    if lay["n_on"] % 32:
        c.add("on-group ends mid-tile")
    if T * 32 > GRID_CAP * 256:
        c.add("second grid-stride trip")
    for k, nm in ((0, "0 survivors"), (1, "1 survivor"), (32, "32 survivors"), (64, "64 survivors")):
        if bool((n_add == k).any()):
            c.add(nm)
    if bool((n_add > 64).any()):
        c.add("more than 64 survivors")
    if bool((n_atom > 1).any()):
        c.add("several atomics per ray")
    j = torch.arange(rec.numel())
    last = torch.zeros(n, dtype=torch.long).scatter_reduce(0, ray, j[live], "amax", include_self=False)
    for lane in (0, 31, 63):
        if bool(((last % 64 == lane) & (n_add > 0)).any()):
            c.add(f"ray ends in lane {lane}")
    if bool((rec.reshape(T, 32) < 0).all(1).any()):
        c.add("all-padding tile")
    return c


Z_SPECIAL = [20.0, float(torch.nextafter(torch.tensor(20.0), torch.tensor(30.0))),
             float(torch.nextafter(torch.tensor(20.0), torch.tensor(0.0))), 19.5, 20.5, 30.0, -30.0, -100.0, 100.0, 0.0]
Z_CLASSES = {"z == 20": lambda z: z == 20, "z just above 20": lambda z: (z > 20) & (z < 21), "z just below 20": lambda z: (z < 20) & (z > 19),
             "z = 30": lambda z: z == 30, "z = -30": lambda z: z == -30, "z = -100": lambda z: z == -100, "z = 100": lambda z: z == 100}


def z_tiles(g, T, rows=4, spread=4.0):
    """pre-activations with the special values sprinkled over every row (live rows and padding alike)"""
    z = torch.randn(T, rows, 32, generator=g) * spread
    n = z.numel()
    k = max(len(Z_SPECIAL), n // 16)
    idx = torch.randperm(n, generator=g)[:k]
    z.view(-1)[idx] = torch.tensor(Z_SPECIAL).repeat(k // len(Z_SPECIAL) + 1)[:k]
    return z


def plant_specials(z, live_slots, start=0):
    """the special values on live (slot, channel) pairs of the three live rows: every pair of a tiny case, every third else"""
    T = z.shape[0]
    t, s_ = torch.nonzero(live_slots.reshape(T, 32), as_tuple=True)
    n = t.numel() * 3
    stride = 1 if n < 30 else 3
    for k in range(0, min(n, 3000), stride):
        z[t[k // 3], k % 3, s_[k // 3]] = Z_SPECIAL[(start + k // stride) % len(Z_SPECIAL)]


def z_census(z, live_slots=None):
    c = set()
    zz = z[:, :3]
    for nm, f in Z_CLASSES.items():
        m = f(zz)
        if live_slots is not None:
            m = m & live_slots.reshape(z.shape[0], 1, 32)
        if bool(m.any()):
            c.add(nm)
    return c


TILE_CASES = {
    # name: (on counts, off counts, all-padding tiles (on, off), upstream gradient scale, non-zero initial accumulators, claims)
    "t1": ([], [5], (0, 0), 1.0, False, {"tiles_all=1", "tiles_on=0"}),
    "t2": ([32, 20], [], (0, 0), 1.0, True, {"tiles_all=2", "tiles_on=tiles_all", "ray ends in lane 31", "32 survivors"}),
    "odd": ([32, 32, 1, 0, 20], [64, 0, 1, 20], (0, 1), 1e-4, True,
            {"tiles_all odd", "tiles_on odd", "on-group ends mid-tile", "0 survivors", "1 survivor", "32 survivors",
             "64 survivors", "ray ends in lane 31", "ray ends in lane 63", "ray ends in lane 0", "all-padding tile"}),
    "even": ([32, 32, 1, 64, 0, 100, 7], [64, 1, 0, 70, 33], (0, 0), 1e-7, False,
             {"tiles_all even", "tiles_on even", "on-group ends mid-tile", "more than 64 survivors", "several atomics per ray",
              "64 survivors", "ray ends in lane 0", "ray ends in lane 63"}),
    "big": (None, None, (0, 0), 1.0, True, {"second grid-stride trip", "tiles_all odd", "tiles_on odd", "more than 64 survivors"}),
}
SMALL_TILE_CASES = [k for k in TILE_CASES if k != "big"]
_TILE_CACHE = {}


def tile_base(name):
    """layout, weights, pre-activations and upstream gradients of one tile case (CPU binary32)"""
    if name in _TILE_CACHE:
        return _TILE_CACHE[name]
    on_c, off_c, pads, gscale, nonzero, claims = TILE_CASES[name]
    g = torch.Generator().manual_seed(100 + list(TILE_CASES).index(name))
    if on_c is None:                                        # past one grid of GRID_CAP * 256 threads, odd / odd
        on_c, tot = [], 0
        while tot <= 8000 * 32:
            on_c.append(int(torch.randint(0, 400, (1,), generator=g)))
            tot += on_c[-1]
        on_c[-1] -= tot - (8000 * 32 + 9)                   # 8001 on-tiles, the group ends mid-tile
        off_c, tot = [], 0
        while tot <= 8385 * 32:
            off_c.append(int(torch.randint(0, 400, (1,), generator=g)))
            tot += off_c[-1]
        off_c[-1] -= tot - (8385 * 32 + 3)                  # 8386 off-tiles: 16387 in all
    lay = layout(on_c, off_c, *pads)
    T, n, rec = lay["tiles_all"], lay["n_rays"], lay["rec_ray"]
    S = T * 32
    w = torch.rand(S, generator=g)
    live = rec >= 0
    pick = torch.rand(S, generator=g)
    w[pick < 0.05] = 0.0
    w[pick > 0.95] = 1.0
    w[~live] = 7.0                                          # garbage on padding: must not be read into a sum
    d = dict(lay, name=name, rec_w=w, gscale=gscale, claims=set(claims),
             z_off=z_tiles(g, T), z_emo=z_tiles(g, T), zt=z_tiles(g, T, spread=3.0),
             g_srgb=torch.randn(n, 3, generator=g) * gscale, g_lin=torch.randn(n, 3, generator=g) * gscale,
             g_wbg=torch.randn(n, generator=g) * gscale,
             srgb0=torch.randn(n, 3, generator=g) if nonzero else torch.zeros(n, 3),
             lin0=torch.randn(n, 3, generator=g) if nonzero else torch.zeros(n, 3), nonzero=nonzero)
    if name == "t1":                                        # lin of tens: 16 lin is tens to hundreds of radians
        d["z_off"][:, :3, ::3] = torch.rand(T, 3, 11, generator=g) * 18 + 2
    for k, zn in enumerate(("z_off", "z_emo", "zt")):       # (after the override: the classes sit on slots the backwards evaluate)
        plant_specials(d[zn], live, start=3 * k)
    dX = torch.zeros(T, DX_ROWS, 32)
    dX[:, :33] = torch.randn(T, 33, 32, generator=g) * gscale
    dX[:, 33:] = 3.0                                        # rows the kernels never read
    d["dXt"] = dX
    fw = emu_tone_in_fwd(d)
    d["lin"], d["Xt"] = fw["lin"], fw["Xt"]
    rgb = torch.zeros(T, 4, 32)
    rgb[:, :3] = _sg32(d["zt"][:, :3])
    d["rgb"] = rgb
    d["dz_emo0"] = torch.full((T, 4, 32), 123.0)
    on_live = live & (torch.arange(S) < lay["tiles_on"] * 32)       # z_emo counts on the on-tiles only
    d["census"] = tile_census(lay) | z_census(d["z_off"], live) | z_census(d["z_emo"], on_live) | z_census(d["zt"], live)
    if bool(((w == 0) & live).any()) and bool(((w == 1) & live).any()):
        d["census"].add("weights 0 and 1")
    if float(d["lin"].max()) * 16 > 30:
        d["census"].add("16 lin of tens of radians")
    d["census"].add(f"gradient scale {gscale:g}")
    if nonzero:
        d["census"].add("non-zero accumulators")
    _TILE_CACHE[name] = d
    return d


def case_coarse(name):
    d = dict(tile_base(name))
    v = _sg32(d["z_off"][:, :3])
    on = (torch.arange(d["tiles_all"]) < d["tiles_on"])[:, None, None]
    rgb = torch.zeros(d["tiles_all"], 4, 32)
    rgb[:, :3] = torch.where(on, v + _sg32(d["z_emo"][:, :3]), v)
    d["rgb"] = torch.where(_padmask(d["rec_ray"]), torch.zeros_like(rgb), rgb)
    return d


def case_composite3(name, accumulate=0):
    d = dict(tile_base(name))
    g = torch.Generator().manual_seed(300 + list(TILE_CASES).index(name))
    T, n = d["tiles_all"], d["n_rays"]
    d["v"] = torch.randn(T, 8, 32, generator=g)
    d["g"] = d["g_srgb"]
    d["out0"] = d["srgb0"]
    d["accumulate"] = accumulate
    d["dv0"] = torch.randn(T, 8, 32, generator=g)           # rows 3-7 and, without bit 0, nothing else survives
    d["dw0"] = torch.randn(T * 32, generator=g)
    return d


def case_eval_aux(name):
    d = dict(tile_base(name))
    g = torch.Generator().manual_seed(400)
    T = d["tiles_all"]
    d["X"] = torch.randn(T, 9, 32, generator=g)
    d["nrow"] = (6, 2, 5)
    q, _ = torch.linalg.qr(torch.randn(3, 3, generator=g))
    d["rt"] = [float(v) for v in q.reshape(-1)]
    d["stepdist"] = 0.0123
    d["rec_step"] = torch.randint(0, 700, (T * 32,), generator=g, dtype=torch.int32)
    return d


ACT_CASES = {"softplus_4_3": (0, 4, 3, 7), "sigmoid_8_5": (1, 8, 5, 5), "softplus_big": (0, 4, 3, GRID_CAP * 256 // (4 * 32) + 3)}


def case_act(name):
    act, rows, n_ch, T = ACT_CASES[name]
    g = torch.Generator().manual_seed(500 + act + rows)
    z = z_tiles(g, T, rows)
    return dict(name=name, act=act, n_ch=n_ch, tiles=T, rows=rows, z=z, census=z_census(z),
                g=torch.randn(T, rows, 32, generator=g) * (1e-4 if rows == 8 else 1.0))


def case_act_batch(name):
    """full: the maximum job count -- a forward, a backward with every source (inverse map, points, three extras), a backward
    through the identity map, a backward from a tile-major gradient alone; big: past one grid of the batch launch"""
    g = torch.Generator().manual_seed(600)
    lay = tile_base("even")
    rec, T = lay["rec_ray"], lay["tiles_all"]
    live = torch.nonzero(rec >= 0)[:, 0]
    m3 = live.numel()
    jobs = []
    if name == "big":
        Tb = ACT_BATCH_CAP * 256 // (8 * 32) + 5
        jobs.append(dict(z=z_tiles(g, Tb, 8), act=0, n_ch=5, bwd=1, g_tile=torch.randn(Tb, 8, 32, generator=g),
                         src=torch.randn(Tb * 32 - 11, 5, generator=g)))
        return dict(name=name, jobs=jobs)
    perm = live[torch.randperm(m3, generator=g)]
    inv = torch.full((T * 32,), -1, dtype=torch.int32)
    inv[perm] = torch.arange(m3, dtype=torch.int32)
    P = 9
    pt1 = torch.zeros(T * 32, dtype=torch.int32)
    pt1[perm[torch.randperm(m3, generator=g)[:P]]] = torch.arange(1, P + 1, dtype=torch.int32)
    jobs.append(dict(z=z_tiles(g, T, 4), act=0, n_ch=3, bwd=0))
    jobs.append(dict(z=z_tiles(g, T, 8), act=1, n_ch=5, bwd=1, g_tile=torch.randn(T, 8, 32, generator=g),
                     src=torch.randn(m3, 5, generator=g), inv=inv, pt1=pt1,
                     ex=[(torch.randn(P, 3, generator=g), 0), (torch.randn(P, 1, generator=g), 3), (torch.randn(P, 1, generator=g), 4)]))
    jobs.append(dict(z=z_tiles(g, T, 4), act=0, n_ch=3, bwd=1, src=torch.randn(70, 3, generator=g) * 1e-7))
    jobs.append(dict(z=z_tiles(g, 3, 8), act=0, n_ch=8, bwd=1, g_tile=torch.randn(3, 8, 32, generator=g) * 1e-4))
    return dict(name=name, jobs=jobs)


def _loss_inputs(n, white_bg, scale, last_kind, seed, boundary=False, loss0=0.0):
    g = torch.Generator().manual_seed(seed)
    sm = torch.rand(n, 3, generator=g) * 1.4 - 0.2
    lm = torch.rand(n, 3, generator=g) * 1.7 - 0.2
    small = torch.rand(n, 3, generator=g) < 0.25
    lm = torch.where(small, torch.rand(n, 3, generator=g) * 0.008 - 0.001, lm)       # around the sRGB knee and 0
    gt = torch.rand(n, 3, generator=g)
    gt = torch.where(torch.rand(n, 3, generator=g) < 0.3, torch.ones_like(gt), gt)
    al = torch.rand(n, generator=g) * 0.3
    if boundary:                                            # exact-boundary class: white_bg == 0, so ps / pl are inputs
        assert white_bg == 0.0 and n >= 16
        sm[0, 0], sm[1, 1], sm[2, 2] = 0.0, 1.0, 0.0
        lm[3, 0], lm[4, 1], gt[4, 1], lm[5, 2], lm[6, 0], gt[6, 0] = 0.0, 1.0, 1.0, KNEE, 1.0, 0.5
        sm[7, 0], gt[7, 0] = 0.625, 0.625                   # d == 0
        gt[8, 0], lm[8, 0] = 1.0, 1.5                       # saturated target, l0 > 1
    al[n - 1] = dict(inside=0.37, below=1e-9, above=1.0, at_lo=A_LO, at_hi=A_HI)[last_kind]
    return dict(n_rays=n, white_bg=white_bg, w_lin=0.5, w_ent=1e-3, scale=scale, srgb_m=sm, lin_m=lm, last=al, rgbs=gt,
                loss0=torch.tensor(loss0), last_kind=last_kind, boundary=boundary)


LOSS_CASES = {
    "n1": (1, 0.0, 1.0, "inside", False, 0.0), "n63": (63, 1.0, 0.25, "below", False, 0.0),
    "n64": (64, 0.0, 0.25, "above", True, 0.0), "n65": (65, 1.0, 1.0, "inside", False, 2.5),
    "n777": (777, 1.0, 0.25, "inside", False, 0.0), "n777_edges": (777, 0.0, 1.0, "at_lo", True, 1.25),
    "n777_hi": (777, 0.0, 0.25, "at_hi", True, 0.0), "big": (GRID_CAP * 256 + 77, 1.0, 1.0, "inside", False, 0.0),
}


def case_loss(name):
    n, wb, sc, lk, bd, l0 = LOSS_CASES[name]
    d = _loss_inputs(n, wb, sc, lk, 700 + list(LOSS_CASES).index(name), bd, l0)
    d["name"] = name
    return d


def loss_census(inp, ref):
    c = set()
    dec, sat = ref.dec, inp["rgbs"] >= 1
    for k, m in (("ps inside", dec["inside"]), ("pl >= 0", dec["pos"]), ("x below the knee", dec["low"] & dec["pos"])):
        if bool(m.any()):
            c.add(k)
        if bool((~m).any()):
            c.add("not " + k)
    if bool((sat & dec["le1"]).any()):
        c.add("gt >= 1, l0 <= 1")
    if bool((sat & ~dec["le1"]).any()):
        c.add("gt >= 1, l0 > 1")
    ps32 = inp["srgb_m"] + (inp["last"] * torch.tensor(inp["white_bg"], dtype=F32))[:, None]
    if bool(((ps32 == inp["rgbs"]) & dec["inside"]).any()):
        c.add("d == 0")
    c.add("last ray " + inp["last_kind"])
    if inp["boundary"]:
        c.add("exact boundaries")
    return c


def _pair_job(g, rows, kind, b=True, mask=None, count=None, ga=True, gb=True, cols=3, w=(0.7, 1.3, 0.4), zeros_d=False):
    a = torch.randn(rows, cols, generator=g)
    bb = torch.randn(rows, cols, generator=g) if b else None
    if zeros_d and bb is not None:
        bb[::5] = a[::5]                                    # d == 0: sign(0) = 0
    job = dict(a=a, b=bb, kind=kind, w_value=w[0], w_a=w[1], w_b=w[2], want_ga=ga, want_gb=gb and b, mask_value=0,
               census={"d == 0"} if (bb is not None and bool((a == bb).any())) else set())
    if mask is not None:
        m = (torch.rand(rows, generator=g) < 0.4).to(torch.uint8)
        job["row_mask"] = m
        if count == "true":
            job["count"] = int((m == 0).sum())
        elif count == "zero":
            job["row_mask"] = torch.ones(rows, dtype=torch.uint8)
            job["count"] = 0
    return job


def pair_jobs():
    g = torch.Generator().manual_seed(800)
    return dict(
        mse=_pair_job(g, 300, 0), l1=_pair_job(g, 300, 1, zeros_d=True), b_null=_pair_job(g, 301, 0, b=False),
        mask_count=_pair_job(g, 300, 1, mask=True, count="true"), mask_nocount=_pair_job(g, 300, 0, mask=True),
        count_zero=_pair_job(g, 64, 0, mask=True, count="zero"), no_ga=_pair_job(g, 65, 1, ga=False),
        no_gb=_pair_job(g, 63, 0, gb=False), big=_pair_job(g, PAIR_CAP * 256 // 3 + 1000, 0, mask=True, count="true"))


def case_pair(name, loss0=0.0):
    d = dict(pair_jobs()[name])
    d["loss0"] = torch.tensor(loss0)
    d["name"] = name
    return d


def case_pair_batch(name):
    j = pair_jobs()
    if name == "full":                                      # the maximum job count
        jobs = [j[k] for k in ("mse", "l1", "b_null", "mask_count", "mask_nocount", "count_zero")]
        assert len(jobs) == PAIR_MAX_JOBS
        return dict(name=name, jobs=jobs, loss0=torch.tensor(0.75))
    return dict(name=name, jobs=[j["big"], j["no_ga"], j["no_gb"]], loss0=torch.tensor(0.0))


def case_eval_disp(n):
    g = torch.Generator().manual_seed(900 + n)
    return dict(name=f"n{n}", n_rays=n, depth3=torch.rand(n, 3, generator=g) * 4 + 0.01, last=torch.rand(n, generator=g), far=6.5)


# op name -> (case builder, case names, float64 restatement, binary32 emulation, family, C entry points)
OPS = {
    "tone_in_fwd": (tile_base, list(TILE_CASES), ref_tone_in_fwd, emu_tone_in_fwd, "tone", ("esr_fine_tone_in_fwd",)),
    "tone_in_bwd": (tile_base, list(TILE_CASES), ref_tone_in_bwd, emu_tone_in_bwd, "tone", ("esr_fine_tone_in_bwd",)),
    "lts_tone_in_bwd": (tile_base, list(TILE_CASES), ref_lts_tone_in_bwd, emu_lts_tone_in_bwd, "tone", ("esr_lts_tone_in_bwd",)),
    "composite_fwd": (tile_base, list(TILE_CASES), ref_composite_fwd, emu_composite_fwd, "composite", ("esr_fine_composite_fwd",)),
    "composite_bwd": (tile_base, list(TILE_CASES), ref_composite_bwd, emu_composite_bwd, "composite", ("esr_fine_composite_bwd",)),
    "composite3_fwd": (case_composite3, list(TILE_CASES), ref_composite3_fwd, emu_composite3_fwd, "composite", ("esr_composite3_fwd",)),
    "composite3_bwd": (case_composite3, [(n, a) for n in SMALL_TILE_CASES for a in range(4)] + [("big", 3)], ref_composite3_bwd,
                       emu_composite3_bwd, "composite", ("esr_composite3_bwd",)),
    "coarse_shade_fwd": (case_coarse, list(TILE_CASES), ref_coarse_shade_fwd, emu_coarse_shade_fwd, "coarse", ("esr_coarse_shade_fwd",)),
    "coarse_shade_bwd": (case_coarse, list(TILE_CASES), ref_coarse_shade_bwd, emu_coarse_shade_bwd, "coarse", ("esr_coarse_shade_bwd",)),
    "loss": (case_loss, list(LOSS_CASES), ref_loss, emu_loss, "loss", ("esr_fine_loss_fwd_bwd_dp",)),
    "act": (case_act, list(ACT_CASES), ref_act, emu_act, "act", ("esr_act_fwd", "esr_act_bwd")),
    "act_batch": (case_act_batch, ["full", "big"], ref_act_batch, emu_act_batch, "act", ("esr_act_batch",)),
    "pair_loss": (case_pair, list(pair_jobs()) + [("mse", 3.5)], ref_pair_loss, emu_pair_loss, "pair", ("esr_pair_loss_fwd_bwd",)),
    "pair_batch": (case_pair_batch, ["full", "rest"], ref_pair_batch, emu_pair_batch, "pair", ("esr_pair_loss_batch",)),
    "eval_aux": (case_eval_aux, list(TILE_CASES), ref_eval_aux, emu_eval_aux, "eval", ("esr_eval_aux",)),
    "eval_disp": (case_eval_disp, [1, 777, GRID_CAP * 256 + 5], ref_eval_disp, emu_eval_disp, "eval", ("esr_eval_disp",)),
}


def build(op, case):
    return OPS[op][0](*case) if isinstance(case, tuple) else OPS[op][0](case)


def all_cases():
    return [(op, case) for op, spec in OPS.items() for case in spec[1]]


def is_big(case):
    return case == "big" or (isinstance(case, tuple) and case[0] == "big") or (isinstance(case, int) and case > 100000)


def verify(op, inp, got, K):
    """compare one op's outputs with the restatement (decisions forced from the outputs where the op has banded ones)"""
    ref_fn = OPS[op][2]
    ref = force_from_outputs(ref_fn, inp, got) if op == "loss" else ref_fn(inp)
    worst, fails = compare(ref, got, K)
    return ref, worst, fails


FLIP_CAP = 0.01

# K per family of entry points, for both test files: the next power of two at or above twice the worst ratio
# |gpu - ref| / (U absref) measured on the MI355X over every case of test_gpu_shade_ref64.py (printed under -s), so that the order
# of the float atomics has room.  The binary32 emulation reaches the same worst ratios to two digits.
K_FAMILY = {
    "tone": 2,          # measured worst 0.80 (esr_fine_tone_in_fwd: sin / cos of lin 2^i; the two backwards 0.17)
    "composite": 2,     # 0.99 (esr_composite3_bwd accumulating; composite_fwd 0.84, composite_bwd 0.86, composite3_fwd 0.45)
    "coarse": 2,        # 0.83 (esr_coarse_shade_fwd; shade_bwd 0.71)
    "loss": 2,          # 0.99 (esr_fine_loss_fwd_bwd_dp; no decision flipped in any case)
    "act": 1,           # 0.44 (esr_act_fwd / esr_act_bwd; esr_act_batch 0.39)
    "pair": 2,          # 0.71 (esr_pair_loss_fwd_bwd and esr_pair_loss_batch)
    "eval": 2,          # 0.97 (esr_eval_aux; esr_eval_disp 0.49)
}

# mutant of the emulation -> the ops it applies to; each must break the bound on at least one (small) case of those ops
# (spgrad_nobranch: the branch-free derivative in its sigmoid form is 1 to within 2e-9 above z = 20, below binary32 resolution, so
# no bound of this kind can tell it from the branch; the mutant is the exponential form exp(z) / (1 + exp(z)) and is rejected
# only through the overflow at the planted z = 100.  Its rejection says nothing about sensitivity near the threshold itself.)
MUTANTS = {
    "freq_factor_dropped": ["tone_in_bwd", "lts_tone_in_bwd"],
    "sin_cos_swapped": ["tone_in_fwd", "tone_in_bwd"],
    "spgrad_nobranch": ["tone_in_bwd", "lts_tone_in_bwd", "act"],
    "segment_leaks_a_lane": ["composite_fwd", "composite3_fwd", "coarse_shade_fwd"],
    "wave_last_lane_dropped": ["composite_fwd", "composite3_fwd", "coarse_shade_fwd"],
    "padding_lanes_contribute": ["composite_fwd", "composite3_fwd", "coarse_shade_fwd"],
    "tiles_on_off_by_one": ["tone_in_fwd", "tone_in_bwd", "lts_tone_in_bwd", "coarse_shade_fwd", "coarse_shade_bwd"],
    "entropy_on_ray_0": ["loss"],
    "scale_not_on_entropy": ["loss"],
    "saturated_clamp_passes_gradient": ["loss"],
    "accumulate_bits_exchanged": ["composite3_bwd"],
    "pair_divides_by_total": ["pair_loss", "pair_batch"],
    "act_gather_ignores_inverse_map": ["act_batch"],
}
