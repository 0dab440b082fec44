"""Float64 restatement of the arithmetic kernels of the light-transport stage (csrc/lts.hip: the exact SDF gradient and its
scatter, the hemisphere directions, the light-transport combine and the emission edit), with a plain binary32 torch emulation of
each operation and the input builders shared by tests/test_lts_ref64_host.py and tests/test_gpu_lts_ref64.py; never imported by
the product path.

Written from the formulas the kernel header cites and from oracle/lts_path.py:
  exact gradient   f(x) = sum over the 8 corners of w_x w_y w_z g[corner], weights (i0 + 1 - idx, idx - i0) with i0 = floor(idx)
                   taken BEFORE the corners are clamped to the grid (zero_pad: corners off the grid are dropped instead),
                   idx = ((p - min) / (max - min) * 2 - 1 + 1) / 2 * (dims - 1);  df/dx = (X - 1) / (max_x - min_x) * sum (+-) w_y w_z g
  directions       d = normalize(raw, eps 1e-12), flipped into the normal's hemisphere where d . n < 0
  reflection       h = normalize(wi + wo); D = exp(2 / r2 (n.h - 1)) / (pi r2), r2 = max(ro^2, 1e-7); F = F0 + (1 - F0)(1 - wo.h)^5,
                   F0 = 0.04 (1 - m) + a m; V = v(wi.n) v(wo.n), v(c) = 0.5 / max(c (1 - k) + k, 1e-7), k = (1 + ro)^2 / 8;
                   R = ((1 - m) a / pi + D F V) (wi.n) 2 pi, every cosine clamped at 0
  environment      env = softplus(sum_j mu_j exp(|lambda_j| (wi . normalize(lobe_j) - 1)))
  combine          off_hat = mean_r (off_m + env last2) R,  emo_hat = emission + mean_r emo_m R  (pdra: emission + detached mean on
                   uncertain points, the mean alone on certain ones), for the two copies wo = -view and wo = dirs[:, R]
  emission edit    mode 0 off, 2 / 4 intensity scale, 3 / 4 hue and saturation replaced through the hsv sector table.

Every entry returns, per output, (value, absref, zero): a value is checked as |got - value| <= K * U * absref + FLOOR (shade_ref64's
`compare`).  absref is the same computation on magnitudes plus first-order terms of the binary32 intermediates.  Here it is carried
next to the code by `Q`, a pair (v, E) with E a bound of |q_f32 - q| / U:
  a +- b     E = E_a + E_b + |v|          a b        E = |a| E_b + |b| E_a + |v|          a / b      E = E_a / |b| + |a| E_b / b^2 + |v|
  sqrt a     E = E_a / (2 v) + |v|        exp a      E = v E_a + 2 v   (expf, log1pf: 2 ulp of the result)
  max(a, c)  E = E_a, 0 where a is below c by more than its band        a 2^k      E = 2^k E_a   (exact)
  the rounding term |v| is dropped where both operands are exact (E = 0) and v is a binary32 number: such an operation commits no
  error, so planted exact inputs (a point on a face, wi + wo = 0) carry E = 0 through the chain.
  sum of n terms with `r` roundings on the path of an addend: E = sum E_i + r sum |v_i| (every partial sum <= sum |v_i|).
A contracted a * b + c rounds once where the model counts twice: the model is an upper bound for either code.

expgrad.  The sample position is the binary32 input (explicit mode) or the sampler's bit-exact replay (feat_ref64.ray_geom /
  ray_point: every op of esr_ray_geom is a separately rounded binary32 op); everything after it is float64.  E_idx covers the noise
  step (product and sum: either rounding of p + noise eps), the subtract, the two divides and the multiply.  It enters the weights
  as an absolute error.  floor(idx) is a decision: a point whose float64 index lies strictly within DEC_K * U * E_idx of an integer
  may take either cell (`shift`); an exact index has E = 0 and is never exempt.  The value is continuous across the decision, the
  gradient and the backward's target cells are not.  Backward: dense over the (small) grid, cell -> (value, absref, count); one
  rounding per addend of a cell and one float atomic per contribution, each at a magnitude <= |init| + M.
combine.  exp and log1p 2 ulp; the J-term lobe sum J roundings; the exponent 2 / r2 (n.h - 1) carries E of n.h times 2 / r2 (the
  dominant term at small roughness: it comes out of the product rule above); hemisphere means: one rounding per ray of a lane (the
  trips), 6 shuffle levels, 4 wave partials, the divide by R; lobe gradients: 6 shuffle levels, one LDS atomic per wave and trip
  (<= 8), the projection off the unit lobe, one global atomic per point at a magnitude <= |init| + sum_p |contribution|.
  Decisions on inputs or exactly rounded products have no band and follow the kernel's documented convention (a clamp passes the
  gradient at equality, sign(0) = 0): ro^2 >= 1e-7 (on the ROUNDED product), den >= 1e-7, pre > 20 (softplus and its derivative are
  continuous across it to 2e-9 relative), the sign of lambda.  No binary32 ro has a square that rounds to 1e-7f (the two neighbours
  land one ulp below and two above: asserted in the host test), so the r2 clamp's equality convention cannot be observed.  The four
  cosine clamps compare computed quantities; no output differentiates with respect to a direction, so every output is continuous
  across them and the band enters only as the E of max(a, 0).  The hemisphere flip of the directions is banded with DEC_K * U * E_dt.
dirs.  Every element is exactly the flipped or the unflipped quotient; |d| is checked against the restatement's |d| (1 unless
  the raw vector is shorter than the 1e-12 clamp).
emit_edit.  The kernel is `fp contract(off)`: h 6 and the sector arithmetic are replayed in binary32 (a decision on an exactly rounded
  product), the rest is Q arithmetic."""
from __future__ import annotations

import math

import torch

from feat_ref64 import ray_geom, ray_point
from shade_ref64 import DEC_K, FLOOR, U, Ref, compare, softplus64, spgrad64

F32, F64 = torch.float32, torch.float64
FLIP_CAP = 0.01                  # as shade_ref64.FLIP_CAP: the share of values a case may exempt as decision flips
MAX_SG = 64


def f32(v):
    return float(torch.tensor(v, dtype=F32))


PI32, C04_32, EPS32, N12_32 = f32(math.pi), f32(0.04), f32(1e-7), f32(1e-12)


class Consts:
    """the constants as the kernel holds them (binary32) or, for the comparison with the float64 oracle, as written"""
    def __init__(self, exact=False):
        self.pi, self.c04, self.eps, self.n12 = (math.pi, 0.04, 1e-7, 1e-12) if exact else (PI32, C04_32, EPS32, N12_32)


KC = Consts()


# ---- value-and-error arithmetic ---------------------------------------------------------------------------------------
def _is32(v):
    v = v.detach()
    return v.float().double() == v


class Q:
    """value v (float64, may carry autograd) and E >= |binary32 result - v| / U, first order (module docstring)"""
    __slots__ = ("v", "E")

    def __init__(self, v, E=None):
        self.v = v
        self.E = torch.zeros_like(v.detach()) if E is None else E

    @staticmethod
    def lift(x):
        if isinstance(x, Q):
            return x
        if not torch.is_tensor(x):
            x = torch.tensor(float(x), dtype=F64)
        return Q(x.double())

    def _rnd(self, v, Ep):
        exact = (Ep == 0) & _is32(v)
        return Q(v, Ep + torch.where(exact, torch.zeros_like(Ep), v.detach().abs()))

    def __add__(self, o):
        o = Q.lift(o)
        return self._rnd(self.v + o.v, self.E + o.E)

    __radd__ = __add__

    def __sub__(self, o):
        o = Q.lift(o)
        return self._rnd(self.v - o.v, self.E + o.E)

    def __rsub__(self, o):
        return Q.lift(o) - self

    def __neg__(self):
        return Q(-self.v, self.E)

    def __mul__(self, o):
        o = Q.lift(o)
        return self._rnd(self.v * o.v, self.v.detach().abs() * o.E + o.v.detach().abs() * self.E)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = Q.lift(o)
        b = o.v.detach().abs()
        return self._rnd(self.v / o.v, self.E / b + self.v.detach().abs() * o.E / (b * b))

    def __rtruediv__(self, o):
        return Q.lift(o) / self

    def __getitem__(self, k):
        return Q(self.v[k], self.E[k])

    def reshape(self, *shape):
        return Q(self.v.reshape(*shape), self.E.reshape(*shape))

    def scale2(self, f):
        """times a power of two: exact"""
        return Q(self.v * f, self.E * abs(f))

    def abs(self):
        return self.v.detach().abs()


def xexp(a):
    if isinstance(a, Q):
        v = torch.exp(a.v)
        return Q(v, v.detach() * (a.E + 2))
    return torch.exp(a)


def xsqrt(a):
    if isinstance(a, Q):
        v = torch.sqrt(a.v)
        d = v.detach()
        return Q(v, torch.where(d > 0, a.E / (2 * d).clamp_min(1e-300), a.E) + torch.where(_is32(v) & (a.E == 0), 0 * d, d))
    return torch.sqrt(a)


def xmax(a, c):
    """max(a, c), c a constant; the gradient passes at equality"""
    if isinstance(a, Q):
        v = a.v.clamp(min=c)
        dead = a.v.detach() < c - DEC_K * U * a.E
        return Q(v, torch.where(dead, torch.zeros_like(a.E), a.E))
    return a.clamp(min=c)


def xsum(a, dim, rounds):
    """sum over `dim` with `rounds` roundings on the path of an addend"""
    if isinstance(a, Q):
        return Q(a.v.sum(dim), a.E.sum(dim) + rounds * a.v.detach().abs().sum(dim))
    return a.sum(dim)


def xsoftplus(a):
    if isinstance(a, Q):
        sp, E = softplus64(a.v)
        d, _ = spgrad64(a.v.detach())
        return Q(sp, E + d * a.E)
    return torch.where(a > 20, a, torch.log1p(torch.exp(a.clamp(max=20.0))))


def xspgrad(a):
    """softplus'(a) = a > 20 ? 1 : sigmoid(a)"""
    if isinstance(a, Q):
        d, E = spgrad64(a.v)
        return Q(d, E + d * (1 - d) * a.E)
    return torch.where(a > 20, torch.ones_like(a), 1.0 / (1.0 + torch.exp(-a)))


def xval(a):
    return a.v if isinstance(a, Q) else a


def xwhere(m, a, b):
    if isinstance(a, Q) or isinstance(b, Q):
        a, b = Q.lift(a), Q.lift(b)
        return Q(torch.where(m, a.v, b.v), torch.where(m, a.E, b.E))
    return torch.where(m, a, b)


def xstack(xs, dim=-1):
    if any(isinstance(x, Q) for x in xs):
        xs = [Q.lift(x) for x in xs]
        shape = torch.broadcast_shapes(*[x.v.shape for x in xs])
        return Q(torch.stack([x.v.expand(shape) for x in xs], dim), torch.stack([x.E.expand(shape) for x in xs], dim))
    shape = torch.broadcast_shapes(*[x.shape for x in xs])
    return torch.stack([x.expand(shape) for x in xs], dim)


def xdot(a, b):
    """sum over the last axis of a * b (3 terms: the roundings of the two adds are the Q ops' own)"""
    p = a * b
    return (p[..., 0] + p[..., 1]) + p[..., 2]


def lift(x, mode):
    """an input tensor in the number system of `mode`: 'q' -> Q over float64, '64' -> float64, '32' -> binary32"""
    if x is None:
        return None
    if mode == "q":
        return Q(x.double())
    return x.double() if mode == "64" else x.float()


def _out(q, zero=None):
    if isinstance(q, Q):
        return (q.v.detach(), q.E, zero)
    return (q.detach(), torch.zeros_like(q.detach()), zero)


# =======================================================================================================================
# exact SDF gradient
# =======================================================================================================================
def expgrad_points(inp):
    """the sample positions in binary32 [n, 3] and the mask of live rows (explicit mode: every row)"""
    if inp.get("pts") is not None:
        return inp["pts"], torch.ones(inp["pts"].shape[0], dtype=torch.bool)
    r = inp["rec_ray"].long()
    live = r >= 0
    start, dirv, _ = ray_geom(inp["rays_o"][r.clamp_min(0)], inp["rays_d"][r.clamp_min(0)], inp["lo"], inp["hi"], inp["near"],
                              inp["stepdist"])
    p = ray_point(start, dirv, inp["stepdist"], inp["rec_step"])
    return torch.where(live[:, None], p, torch.zeros_like(p)), live


def expgrad_index(inp, p, mode, mut=None):
    """continuous grid index [n, 3] and the gradient scale [3] in the number system of `mode`"""
    x = lift(p, mode)
    if inp.get("noise") is not None:
        x = x + lift(inp["noise"], mode) * lift(torch.tensor(inp["eps"], dtype=F32), mode)
    lo, hi = lift(inp["lo"], mode), lift(inp["hi"], mode)
    top = torch.tensor([d - 1.0 for d in inp["dims"]], dtype=F64 if mode != "32" else F32)
    u = (x - lo) / (hi - lo)
    if mode == "q":
        n = u.scale2(2.0) - 1.0
        idx = (n + 1.0).scale2(0.5) * Q(top)
        scale = Q(top) / (hi - lo)
    else:
        idx = ((u * 2.0 - 1.0) + 1.0) / 2.0 * top
        scale = top / (hi - lo)
    if mut == "scale_wrong_axis":
        scale = scale[[1, 2, 0]] if mode != "q" else Q(scale.v[[1, 2, 0]], scale.E[[1, 2, 0]])
    return idx, scale


def _expgrad_corners(inp, idx, fl, mode, mut=None):
    """per corner [n, 8]: flat cell, kept mask, and the four coefficients c0..c3 (value, d/dx, d/dy, d/dz before the scale)"""
    dims = inp["dims"]
    zero_pad = inp["zero_pad"] and mut != "zero_pad_ignored"
    if mut == "weights_after_clamp":
        fl = torch.minimum(torch.maximum(fl, torch.zeros_like(fl)), torch.tensor([d - 2.0 for d in dims], dtype=fl.dtype))
    w = [(lift_like(fl + 1.0, idx) - idx), (idx - lift_like(fl, idx))]              # w[c][n, 3]
    cells, keep, cs = [], [], [[], [], [], []]
    i0 = fl.long()
    for cx in (0, 1):
        for cy in (0, 1):
            for cz in (0, 1):
                c = (cx, cy, cz)
                ii = [i0[:, a] + c[a] for a in range(3)]
                inb = torch.ones_like(ii[0], dtype=torch.bool)
                for a in range(3):
                    inb &= (ii[a] >= 0) & (ii[a] < dims[a])
                cl = [ii[a].clamp(0, dims[a] - 1) for a in range(3)]
                cells.append((cl[0] * dims[1] + cl[1]) * dims[2] + cl[2])
                keep.append(inb if zero_pad else torch.ones_like(inb))
                wx, wy, wz = w[cx][:, 0], w[cy][:, 1], w[cz][:, 2]
                sx, sy, sz = (1.0 if cx else -1.0), (1.0 if cy else -1.0), (1.0 if cz else -1.0)
                cs[0].append(wx * wy * wz)
                cs[1].append((wy * wz) * sx if mode != "q" else (wy * wz).scale2(sx))
                cs[2].append((wx * wz) * sy if mode != "q" else (wx * wz).scale2(sy))
                cs[3].append((wx * wy) * sz if mode != "q" else (wx * wy).scale2(sz))
    return torch.stack(cells, 1), torch.stack(keep, 1), [xstack(c, 1) for c in cs]


def lift_like(t, like):
    return Q(t.double()) if isinstance(like, Q) else t.to(xval(like).dtype)


def expgrad_band(idx):
    """mask [n, 3] of indices strictly inside the band of an integer and the alternative floor's offset"""
    v = idx.v.detach()
    near = torch.round(v)
    frac = v - near
    band = frac.abs() < DEC_K * U * idx.E
    alt = torch.where(frac < 0, torch.ones_like(v), -torch.ones_like(v))
    return band, alt


def _expgrad_fwd_any(inp, mode, shift=None, mut=None, sdf=None):
    p, live = expgrad_points(inp)
    idx, scale = expgrad_index(inp, p, mode, mut)
    fl = torch.floor(xval(idx).detach())
    if shift is not None:
        fl = fl + shift.to(fl.dtype)
    cell, keep, cs = _expgrad_corners(inp, idx, fl, mode, mut)
    grid = (lift(inp["sdf"], "64" if mode == "q" else mode) if sdf is None else sdf).reshape(-1)
    gc = grid[cell] * keep.to(grid.dtype)
    gq = Q(gc) if mode == "q" else gc
    val = xsum(gq * cs[0], 1, 8)
    d = [xsum(gq * cs[1 + a], 1, 8) * scale[a] for a in range(3)]
    out = xstack([val] + d, 1)
    z = ~live
    if mode == "q":
        out = Q(torch.where(z[:, None], torch.zeros_like(out.v), out.v), torch.where(z[:, None], torch.zeros_like(out.E), out.E))
    else:
        out = torch.where(z[:, None], torch.zeros_like(out), out)
    return out, idx, live


def ref_expgrad_fwd(inp, shift=None, sdf=None):
    out, idx, live = _expgrad_fwd_any(inp, "q", shift, sdf=sdf)
    r = Ref(out=dict(out=_out(out, (~live)[:, None].expand(-1, 4))))
    r.idx, r.q = idx, out
    return r


def _expgrad_contrib(inp, mode, shift=None, mut=None, rows=None):
    """per point and corner [n, 8]: cell, kept mask and the contribution t = gv c0 + sum_a g_a scale_a c_a"""
    p, live = expgrad_points(inp)
    sub = inp
    if rows is not None:
        p, live = p[rows], live[rows]
        sub = dict(inp, noise=None if inp.get("noise") is None else inp["noise"][rows])
    idx, scale = expgrad_index(sub, p, mode, mut)
    fl = torch.floor(xval(idx).detach())
    if shift is not None:
        fl = fl + shift.to(fl.dtype)
    cell, keep, cs = _expgrad_corners(sub, idx, fl, mode, mut)
    g = lift(inp["g"] if rows is None else inp["g"][rows], mode)
    gv = g[:, 0:1]
    gd = [(g[:, 1 + a] * scale[a])[:, None] for a in range(3)]
    t = ((gv * cs[0] + gd[0] * cs[1]) + gd[1] * cs[2]) + gd[2] * cs[3]
    keep = keep & live[:, None]
    return cell, keep, t, idx


def _scatter64(ncell, cell, keep, t, init):
    k = keep.reshape(-1)
    c = cell.reshape(-1)[k]
    tv, tE = t.v.detach().reshape(-1)[k], t.E.reshape(-1)[k]
    z = lambda: torch.zeros(ncell, dtype=F64)
    s, M, E, n = z().index_add_(0, c, tv), z().index_add_(0, c, tv.abs()), z().index_add_(0, c, tE), z().index_add_(0, c, torch.ones_like(tv))
    return s, M, E, n


def ref_expgrad_bwd(inp, shift=None):
    cell, keep, t, idx = _expgrad_contrib(inp, "q", shift)
    init = inp["grad0"].double().reshape(-1)
    s, M, E, n = _scatter64(init.numel(), cell, keep, t, init)
    absref = E + n * (init.abs() + M)
    r = Ref(out=dict(grad_sdf=(init + s, absref, None)))
    r.idx, r.count = idx, n
    return r


def verify_expgrad_fwd(inp, got, K):
    """per point: the restatement's own floor, or -- inside the band -- the alternative that fits"""
    r = ref_expgrad_fwd(inp)
    band, alt = expgrad_band(r.idx)
    band &= expgrad_points(inp)[1][:, None]
    g = got["out"].detach().cpu().double()
    val, absref, zero = r.out["out"]
    val, absref = val.clone(), absref.clone()
    flips = 0
    if bool(band.any()):
        rows = torch.nonzero(band.any(1))[:, 0]
        bad = ((g - val).abs() > K * U * absref + FLOOR).any(1)
        for c in range(1, 8):
            bits = torch.tensor([(c >> a) & 1 for a in range(3)], dtype=torch.bool)
            shift = torch.where(band & bits[None, :], alt, torch.zeros_like(alt))
            use = rows[(shift[rows] != 0).any(1) & bad[rows]]
            if use.numel() == 0:
                continue
            ra = ref_expgrad_fwd(inp, shift)
            va, aa, _ = ra.out["out"]
            fits = ~((g[use] - va[use]).abs() > K * U * aa[use] + FLOOR).any(1)
            take = use[fits]
            val[take], absref[take] = va[take], aa[take]
            bad[take] = False
            flips += int(take.numel())
    r.out["out"] = (val, absref, zero)
    r.band, r.flips = dict(floor=band), dict(floor=flips)
    r.share = flips / max(1, g.shape[0])
    worst, fails = compare(r, got, K)
    return r, worst, fails


def verify_expgrad_bwd(inp, got, K):
    """banded points are resolved one by one: the floor combination whose cells fit the output best"""
    r = ref_expgrad_bwd(inp)
    band, alt = expgrad_band(r.idx)
    p, live = expgrad_points(inp)
    band &= live[:, None]
    g = got["grad_sdf"].detach().cpu().double().reshape(-1)
    init = inp["grad0"].double().reshape(-1)
    flips = 0
    if bool(band.any()):
        cell, keep, t, _ = _expgrad_contrib(inp, "q")
        cur = list(_scatter64(init.numel(), cell, keep, t, init))          # s, M, E, n under the choices taken so far
        opts, choice = {}, {}
        for i in torch.nonzero(band.any(1))[:, 0].tolist():
            opts[i], choice[i] = {}, 0
            for c in range(8):
                bits = torch.tensor([(c >> a) & 1 for a in range(3)], dtype=torch.bool)
                if bool((bits & ~band[i]).any()):
                    continue
                shift = torch.where(bits, alt[i], torch.zeros(3, dtype=F64))[None]
                ct = _expgrad_contrib(inp, "q", shift, rows=torch.tensor([i]))[:3]
                opts[i][c] = (_scatter64(init.numel(), *ct, init), ct[0].reshape(-1))
        for _ in range(3):                                                     # (points that share cells: settle in a few sweeps)
            moved = False
            for i, o in opts.items():
                cells = torch.unique(torch.cat([v[1] for v in o.values()]))
                best, best_c = None, choice[i]
                for c, (d, _) in o.items():
                    s2, M2, E2, n2 = (cur[k] - o[choice[i]][0][k] + d[k] for k in range(4))
                    a2 = E2 + n2 * (init.abs() + M2)
                    score = float((((g - init - s2).abs()[cells] - FLOOR).clamp_min(0) / (U * a2[cells]).clamp_min(1e-300)).max())
                    if best is None or score < best - 1e-9:
                        best, best_c = score, c
                if best_c != choice[i]:
                    cur = [cur[k] - o[choice[i]][0][k] + o[best_c][0][k] for k in range(4)]
                    choice[i], moved = best_c, True
            if not moved:
                break
        flips = sum(1 for c in choice.values() if c != 0)
        s, M, E, n = cur
        r.out["grad_sdf"] = (init + s, E + n * (init.abs() + M), None)
        r.count = n
    r.band, r.flips = dict(floor=band), dict(floor=flips)
    r.share = flips / max(1, int(live.sum()))
    worst, fails = compare(r, got, K)
    return r, worst, fails


def emu_expgrad_fwd(inp, mut=None):
    out, _, _ = _expgrad_fwd_any(inp, "32", mut=mut)
    return dict(out=out)


def emu_expgrad_bwd(inp, mut=None):
    cell, keep, t, _ = _expgrad_contrib(inp, "32", mut=mut)
    k = keep.reshape(-1)
    init = inp["grad0"].reshape(-1).clone()
    if mut == "accumulated_overwritten":
        init[torch.unique(cell.reshape(-1)[k])] = 0.0
    return dict(grad_sdf=init.index_add_(0, cell.reshape(-1)[k], t.reshape(-1)[k]).reshape(inp["grad0"].shape))


# =======================================================================================================================
# hemisphere directions
# =======================================================================================================================
def _dirs_any(inp, mode, force=None, mut=None):
    raw, nrm = lift(inp["raw"], mode), lift(inp["normal"], mode)
    sq = raw * raw
    n = xmax(xsqrt((sq[..., 0] + sq[..., 1]) + sq[..., 2]), KC.n12)
    v, nb = raw / n[..., None], nrm[:, None, :]
    dt = xdot(v, nb)
    flip = xval(dt).detach() < 0
    if mut == "flip_ignored":
        flip = torch.zeros_like(flip)
    if force is not None:
        flip = force
    sg = torch.where(flip, -1.0, 1.0).to(xval(v).dtype)[..., None]
    d = Q(v.v * sg, v.E) if mode == "q" else v * sg
    return d, dt, flip


def ref_lts_dirs(inp, force=None):
    d, dt, flip = _dirs_any(inp, "q", force)
    band = dt.v.abs() < DEC_K * U * dt.E
    out = dict(dirs=_out(d))
    if inp.get("pts") is not None:
        P, R1 = inp["raw"].shape[:2]
        out["d2"] = _out(Q(d.v[:, :R1 - 1].reshape(-1, 3), d.E[:, :R1 - 1].reshape(-1, 3)))
        o2 = inp["pts"].double()[:, None, :].expand(P, R1 - 1, 3).reshape(-1, 3)
        out["o2"] = (o2, torch.zeros_like(o2), None)
        out["v_rand"] = _out(Q(-d.v[:, R1 - 1], d.E[:, R1 - 1]))
    r = Ref(out=out, dec=dict(flip=flip), band=dict(flip=band))
    nv = torch.sqrt((d.v * d.v).sum(-1))
    r.norm = (nv, (d.v.abs() * d.E).sum(-1) / nv.clamp_min(1e-300))      # |d| and its first-order E
    return r


def verify_dirs(inp, got, K):
    r = ref_lts_dirs(inp)
    g = got["dirs"].detach().cpu().double().reshape(r.out["dirs"][0].shape)
    band = r.band["flip"]
    flips = 0
    if bool(band.any()):
        own = r.out["dirs"][0]
        better = ((g + own).abs().sum(-1) < (g - own).abs().sum(-1)) & band
        flips = int(better.sum())
        r = ref_lts_dirs(inp, r.dec["flip"] ^ better)
        r.band = dict(flip=band)
    r.flips = dict(flip=flips)
    r.share = flips / max(1, band.numel())
    worst, fails = compare(r, got, K)
    nv, nE = r.norm
    gn = torch.sqrt((g * g).sum(-1))
    if bool(((gn - nv).abs() > K * U * nE + FLOOR).any()):
        fails.append("dirs: |d| outside the bound of the restatement's |d|")
    return r, worst, fails


def emu_lts_dirs(inp, mut=None):
    d, _, _ = _dirs_any(inp, "32", mut=mut)
    out = dict(dirs=d)
    if inp.get("pts") is not None:
        P, R1 = inp["raw"].shape[:2]
        out["d2"] = d[:, :R1 - 1].reshape(-1, 3).clone()
        out["o2"] = inp["pts"][:, None, :].expand(P, R1 - 1, 3).reshape(-1, 3).clone()
        out["v_rand"] = -d[:, R1 - 1]
    return out


# =======================================================================================================================
# emission edit
# =======================================================================================================================
def _r32(x):
    return x.float().double()


def _emit_any(inp, mode, mut=None):
    e = lift(inp["emit"], mode)
    modes = inp["modes"]
    n = modes.shape[0]
    k = lift(inp["inten"], mode)
    im, cm, off = ((modes == 2) | (modes == 4))[:, None], ((modes == 3) | (modes == 4)), (modes == 0)[:, None]
    if mode == "q":
        kk = Q(k.v[:, None], k.E[:, None])
        e = xwhere(off, Q(torch.zeros(n, 3, dtype=F64)), e)
        e = xwhere(im, e * kk, e)
        v = Q(e.v.max(-1).values, e.E.gather(1, e.v.argmax(-1, keepdim=True))[:, 0])
    else:
        e = torch.where(off, torch.zeros_like(e), e)
        e = torch.where(im, e * k[:, None], e)
        v = e.max(-1).values
    # h 6, the sector and the fraction: binary32, op for op (the remainder of a value in [0, 6] is exact)
    h, sat = inp["colors"][:, 0].double(), lift(inp["colors"][:, 1], mode)
    h6 = _r32(h * 6.0)
    rem = lambda a: _r32(a - _r32(torch.floor(_r32(a / 6.0)) * 6.0))
    sector = rem(torch.floor(h6))
    f = _r32(rem(h6) - sector)
    ks = sector.long()
    if mut == "hue_sector_off_by_one":
        ks = (ks + 1) % 6
    f = lift(f.float(), mode)
    p, q, t = v * (1.0 - sat), v * (1.0 - f * sat), v * (1.0 - (1.0 - f) * sat)
    tab = dict(r=[v, q, p, p, t, v], g=[t, v, v, q, p, p], b=[p, p, t, v, v, q])
    cols = []
    for name in "rgb":
        c = tab[name][5]
        for s in range(4, -1, -1):
            c = xwhere(ks == s, tab[name][s], c)
        cols.append(c)
    hsv = xstack(cols, 1)
    return xwhere(cm[:, None], hsv, e)


def ref_emit_edit(inp):
    return Ref(out=dict(emit=_out(_emit_any(inp, "q"))))


def emu_emit_edit(inp, mut=None):
    return dict(emit=_emit_any(inp, "32", mut))


# =======================================================================================================================
# light-transport combine
# =======================================================================================================================
def _disney(a, ro, m, n, wi, wo, mode, C=KC, want_grads=False, mut=None):
    """R [P, R, 3] for albedo a [P, 1, 3], ro / m [P, 1], normal n [P, 1, 3], wi [P, R, 3], wo [P, 1, 3]; with want_grads also
    dR/da, dR/dro, dR/dm"""
    hv = wi + wo
    hh = hv * hv
    hn = xmax(xsqrt((hh[..., 0] + hh[..., 1]) + hh[..., 2]), C.n12)
    h = hv / hn[..., None]
    noh, ooh = xmax(xdot(n, h), 0.0), xmax(xdot(wo, h), 0.0)
    ion, oon = xmax(xdot(wi, n), 0.0), xmax(xdot(wo, n), 0.0)
    r2raw = ro * ro
    r2 = xmax(r2raw, C.eps)
    D = 1.0 / (r2 * C.pi) * xexp(2.0 / r2 * (noh - 1.0))
    om = 1.0 - ooh
    t5 = om * om * om * om * om
    k = (1.0 + ro) * (1.0 + ro) / 8.0
    den_i, den_o = ion * (1.0 - k) + k, oon * (1.0 - k) + k
    Vi, Vo = 0.5 / xmax(den_i, C.eps), 0.5 / xmax(den_o, C.eps)
    V = Vi * Vo
    lam = (ion * C.pi) * 2.0
    un = lambda x: x[..., None]
    F0 = C.c04 * (1.0 - un(m)) + a * un(m)
    Fr = F0 + (1.0 - F0) * un(t5)
    fd = (1.0 - un(m)) * a / C.pi
    R = (fd + un(D) * Fr * un(V)) * un(lam)
    if not want_grads:
        return R
    # the r2 clamp decides on the ROUNDED product ro * ro (binary32): pass at equality
    r2_32 = (xval(ro).detach().double() ** 2).float()
    passes = r2_32 >= torch.tensor(EPS32, dtype=F32)
    if mut == "r2_clamp_no_grad_at_threshold":
        passes = r2_32 > torch.nextafter(torch.nextafter(torch.tensor(EPS32), torch.tensor(1.0)), torch.tensor(1.0))
    dD_dr2 = D * (-1.0 / r2 - 2.0 * (noh - 1.0) / (r2 * r2))
    dr2 = xwhere(passes, 2.0 * ro, 0.0 * ro)
    dk = (1.0 + ro) / 4.0
    pass_i, pass_o = xval(den_i).detach() >= C.eps, xval(den_o).detach() >= C.eps
    dVi = xwhere(pass_i, -0.5 / (den_i * den_i) * (1.0 - ion), 0.0 * den_i)
    dVo = xwhere(pass_o, -0.5 / (den_o * den_o) * (1.0 - oon), 0.0 * den_o)
    dV = (dVi * Vo + Vi * dVo) * dk
    dR_da = ((1.0 - un(m)) / C.pi + un(D * V) * un(m) * (1.0 - un(t5))) * un(lam)
    dR_dm = (-a / C.pi + un(D * V) * (a - C.c04) * (1.0 - un(t5))) * un(lam)
    dR_dro = Fr * un(dD_dr2 * dr2 * V + D * dV) * un(lam)
    return R, dR_da, dR_dro, dR_dm, dict(noh=noh, r2raw=r2raw, hn=hn, D=D)


def _sg_units(inp, mode, C=KC, lobes=None):
    lb = lift(inp["lobes"], mode) if lobes is None else lobes
    ll = lb * lb
    nn = xmax(xsqrt((ll[..., 0] + ll[..., 1]) + ll[..., 2]), C.n12)
    return lb / nn[..., None], 1.0 / nn


def _trip_mask(R, mut):
    """per ray: whether it is summed (the last lane of a wave dropped under the mutant)"""
    r = torch.arange(R)
    return ~((r % 64) == 63) if mut == "wave_last_lane_dropped" else torch.ones(R, dtype=torch.bool)


def _combine_common(inp, mode, C=KC, mut=None, leaves=None):
    """everything both directions share: per ray the environment colour and its pre-activation, the increments, the reflection of
    the two copies (with gradients)"""
    L = lambda k: (leaves[k] if leaves is not None and k in leaves else lift(inp[k], mode))
    P, R, J = inp["P"], inp["R"], inp["J"]
    un = lambda x, d: x[(slice(None),) * d + (None,)]                # a new axis at position d (tensors and Q alike)
    a, ro, m, n = un(L("base"), 1), un(L("rough"), 1), un(L("metal"), 1), un(L("normal"), 1)
    dirs = L("dirs")
    wi = dirs[:, :R]
    wo0 = un(-L("view"), 1)
    wo1 = dirs[:, R:R + 1] if mut != "wo1_from_view" else wo0
    unit, inv = _sg_units(inp, mode, C, None if leaves is None else leaves.get("lobes"))
    lam_raw = L("lambdas")
    lam = Q(lam_raw.v.abs(), lam_raw.E) if mode == "q" else lam_raw.abs()
    mus = L("mus")
    # [P, R, J]
    wq = un(wi, 2)                                                  # [P, R, 1, 3]
    dtl = xdot(wq, unit)                                            # [P, R, J]
    e = xexp(lam * (dtl - 1.0))
    eq = un(e, 3)                                                   # [P, R, J, 1]
    pre = xsum(mus * eq, 2, J)                                      # [P, R, 3]
    env = xsoftplus(pre)
    last, off_m, emo_m = L("last2").reshape(P, R), L("off_m").reshape(P, R, 3), L("emo_m").reshape(P, R, 3)
    inc_off = off_m + env * un(last, 2)
    d0 = _disney(a, ro, m, n, wi, wo0, mode, C, True, mut)
    d1 = _disney(a, ro, m, n, wi, wo1, mode, C, True, mut)
    return dict(P=P, R=R, J=J, a=a, ro=ro, m=m, wi=wi, unit=unit, inv=inv, lam=lam, lam_raw=lam_raw, mus=mus, dtl=dtl, e=e, pre=pre,
                env=env, last=last, inc_off=inc_off, inc_emo=emo_m, d=(d0, d1), un=un)


def _umask(inp):
    P = inp["P"]
    return torch.zeros(P, dtype=torch.bool) if inp.get("umask") is None else inp["umask"].bool()


def _mean_rounds(R):
    return (R + 255) // 256 + 6 + 4


def _combine_fwd_any(inp, mode, C=KC, mut=None, leaves=None):
    c = _combine_common(inp, mode, C, mut, leaves)
    P, R, un = c["P"], c["R"], c["un"]
    keepr = _trip_mask(R, mut)
    div = 256.0 if mut == "mean_divides_by_256" else float(R)
    um = _umask(inp)
    em = leaves["emission"] if leaves is not None and "emission" in leaves else lift(inp["emission"], mode)
    if inp["pdra"]:
        em = xwhere(um[:, None], em, 0.0 * em)
    off_hat, emo_hat = [], []
    for cpy in (0, 1):
        Rf = c["d"][cpy][0]
        to, te = c["inc_off"] * Rf, c["inc_emo"] * Rf
        if mut == "second_trip_inactive_contribute" and R > 256 and R % 256:
            stale = torch.arange(R % 256, 256) + (R // 256 - 1) * 256     # inactive lanes of the last trip re-add the trip before
            to, te = torch.cat([to, to[:, stale]], 1), torch.cat([te, te[:, stale]], 1)
            kr = torch.cat([keepr, keepr[stale]])
        else:
            kr = keepr
        to, te = to[:, kr], te[:, kr]
        so = xsum(to, 1, _mean_rounds(R)) / div
        sr = xsum(te, 1, _mean_rounds(R)) / div
        if inp["pdra"] and leaves is not None:                          # (autograd form: the reflect term is detached on uncertain points)
            sr = torch.where(um[:, None], sr.detach(), sr)
        off_hat.append(so)
        emo_hat.append(em + sr)
    cat = lambda xs: Q(torch.cat([x.v for x in xs], 0), torch.cat([x.E for x in xs], 0)) if mode == "q" else torch.cat(xs, 0)
    return cat(off_hat), cat(emo_hat), c


def ref_lts_combine_fwd(inp, C=KC):
    oh, eh, c = _combine_fwd_any(inp, "q", C)
    r = Ref(out=dict(off_hat=_out(oh), emo_hat=_out(eh)))
    r.c = c
    return r


def emu_lts_combine_fwd(inp, mut=None):
    oh, eh, _ = _combine_fwd_any(inp, "32", mut=mut)
    return dict(off_hat=oh, emo_hat=eh)


def _combine_bwd_any(inp, mode, C=KC, mut=None):
    c = _combine_common(inp, mode, C, mut)
    P, R, J, un = c["P"], c["R"], c["J"], c["un"]
    um = _umask(inp)
    div = 256.0 if mut == "mean_divides_by_256" else float(R)
    g1, g2 = lift(inp["g_off_hat"], mode), lift(inp["g_emo_hat"], mode)
    detach = (um if inp["pdra"] and mut != "pdra_detach_ignored" else torch.zeros(P, dtype=torch.bool))[:, None]
    goh = [un(g1[cp * P:(cp + 1) * P] / div, 1) for cp in (0, 1)]                       # [P, 1, 3]
    geh = [un(xwhere(detach, 0.0 * g2[cp * P:(cp + 1) * P], g2[cp * P:(cp + 1) * P] / div), 1) for cp in (0, 1)]
    (R0, da0, dro0, dm0, _), (R1, da1, dro1, dm1, _) = c["d"]
    d_inc_off = goh[0] * R0 + goh[1] * R1
    d_emo_m = geh[0] * R0 + geh[1] * R1
    pe = d_inc_off * c["env"]
    d_last2 = (pe[..., 0] + pe[..., 1]) + pe[..., 2]
    denv = d_inc_off * un(c["last"], 2) * xspgrad(c["pre"])
    dR0 = goh[0] * c["inc_off"] + geh[0] * c["inc_emo"]
    dR1 = goh[1] * c["inc_off"] + geh[1] * c["inc_emo"]
    keepr = _trip_mask(R, mut)
    stale = None
    if mut == "second_trip_inactive_contribute" and R > 256 and R % 256:
        stale = torch.arange(R % 256, 256) + (R // 256 - 1) * 256

    def rsum(x, extra=0):
        if stale is not None:
            x = torch.cat([x, x[:, stale]], 1)
            return x[:, torch.cat([keepr, keepr[stale]])].sum(1)
        return xsum(x[:, keepr], 1, _mean_rounds(R) + extra)

    gb = dR0 * da0 + dR1 * da1
    d_base = rsum(gb)
    gr = dR0 * dro0 + dR1 * dro1
    gm = dR0 * dm0 + dR1 * dm1
    trips = (R + 255) // 256                                         # (the three channels join the running sum one by one)
    d_rough = rsum((gr[..., 0] + gr[..., 1]) + gr[..., 2], 2 * trips)
    d_metal = rsum((gm[..., 0] + gm[..., 1]) + gm[..., 2], 2 * trips)
    has_em = ~(torch.full((P,), bool(inp["pdra"])) & ~um)
    if mut == "demission_on_certain":
        has_em = torch.ones(P, dtype=torch.bool)
    d_emission = xwhere(has_em[:, None], g2[:P] + g2[P:], 0.0 * g2[:P])
    # lobe gradients: per point the sums over the rays, then through |lambda| and normalize(lobe), then over the points
    e, dtl, mus, lam, unit = c["e"], c["dtl"], c["mus"], c["lam"], c["unit"]
    lobe_rounds = 6 + 4 * ((R + 255) // 256)
    dq = un(denv, 2)                                                                    # [P, R, 1, 3]
    eq = un(e, 3)
    v_mu = dq * eq                                                                      # [P, R, J, 3]
    dm_ = dq * mus
    de = ((dm_[..., 0] + dm_[..., 1]) + dm_[..., 2]) * e                                # [P, R, J]
    v_lam = de * (dtl - 1.0)
    v_lobe = un(de * lam, 3) * un(c["wi"], 2)                                           # [P, R, J, 3]
    ksum = lambda x: (xsum(x[:, keepr], 1, lobe_rounds) if stale is None else
                      torch.cat([x, x[:, stale]], 1)[:, torch.cat([keepr, keepr[stale]])].sum(1))
    acc_mu, acc_lam, acc_lobe = ksum(v_mu), ksum(v_lam), ksum(v_lobe)                   # [P, J, 3], [P, J], [P, J, 3]
    lr = xval(c["lam_raw"]).detach()
    sgn = torch.sign(lr) if mut != "dlambda_without_sign" else torch.ones_like(lr)
    c_lam = acc_lam * sgn.to(xval(acc_lam).dtype) if mode != "q" else Q(acc_lam.v * sgn, acc_lam.E)
    dotl = xdot(acc_lobe, unit)
    proj = acc_lobe - unit * un(dotl, 2) if mut != "lobe_not_projected" else acc_lobe
    c_lobe = proj * un(c["inv"], 1)
    outs = dict(d_off_m=d_inc_off, d_emo_m=d_emo_m, d_last2=d_last2, d_base=d_base, d_rough=d_rough, d_metal=d_metal,
                d_emission=d_emission)
    accs = dict(d_mus=acc_mu, d_lambdas=c_lam, d_lobes=c_lobe)
    return outs, accs, c, has_em


def ref_lts_combine_bwd(inp, C=KC):
    outs, accs, c, has_em = _combine_bwd_any(inp, "q", C)
    P, R = c["P"], c["R"]
    out = {}
    for k, q in outs.items():
        shape = {"d_off_m": (P * R, 3), "d_emo_m": (P * R, 3), "d_last2": (P * R,)}.get(k, q.v.shape)
        zero = (~has_em)[:, None].expand(P, 3) if k == "d_emission" else None
        out[k] = (q.v.detach().reshape(shape), q.E.reshape(shape), zero)
    for k, q in accs.items():
        init = inp[k + "0"].double()
        M = q.v.detach().abs().sum(0)
        out[k] = (init + q.v.detach().sum(0), q.E.sum(0) + P * (init.abs() + M), None)
    r = Ref(out=out)
    r.c = c
    return r


def emu_lts_combine_bwd(inp, mut=None):
    outs, accs, c, _ = _combine_bwd_any(inp, "32", mut=mut)
    P, R = c["P"], c["R"]
    out = {k: v.reshape({"d_off_m": (P * R, 3), "d_emo_m": (P * R, 3), "d_last2": (P * R,)}.get(k, v.shape)) for k, v in outs.items()}
    for k, v in accs.items():
        out[k] = (0.0 if mut == "accumulated_overwritten" else inp[k + "0"]) + v.sum(0)
    return out


# =======================================================================================================================
# input builders (shared by the host test and the GPU test)
# =======================================================================================================================
EG_LO, EG_HI, EG_DIMS = torch.tensor([-1.0, -1.5, -0.5]), torch.tensor([1.0, 0.5, 2.25]), (7, 9, 11)
# name: (mode, n, noise, zero_pad, claims)
EXPGRAD_CASES = {
    "p1": ("pts", 1, False, 0, {"box corner"}),
    "p255": ("pts", 255, True, 1, {"box corner", "face", "integer index", "outside the box", "pile in one cell", "noise", "zero_pad"}),
    "p257": ("pts", 257, False, 1, {"box corner", "face", "integer index", "outside the box", "pile in one cell", "zero_pad",
                                    "second workgroup"}),
    "p5000": ("pts", 5000, True, 0, {"box corner", "face", "integer index", "outside the box", "pile of 300 in one cell", "noise",
                                     "second workgroup"}),
    "p5000z": ("pts", 5000, False, 1, {"box corner", "face", "integer index", "outside the box", "pile of 300 in one cell",
                                       "zero_pad", "second workgroup"}),
    "ray": ("ray", 0, True, 0, {"ray mode", "step 0", "last step", "rec_ray = -1", "noise"}),
    "rayz": ("ray", 0, False, 1, {"ray mode", "step 0", "last step", "rec_ray = -1", "zero_pad"}),
}
_CACHE = {}


def _expgrad_points_set(g):
    lo, hi = EG_LO, EG_HI
    vox = (hi - lo) / torch.tensor([d - 1.0 for d in EG_DIMS])
    pts = []
    for c in range(8):                                                   # the eight box corners: exact
        pts.append(torch.stack([(hi if (c >> a) & 1 else lo)[a] for a in range(3)]))
    for a in range(3):                                                   # each face exactly
        for side in (lo, hi):
            for _ in range(2):
                p = lo + (hi - lo) * torch.rand(3, generator=g)
                p[a] = side[a]
                pts.append(p)
    for k in range(20):                                                  # integer indices in the interior (y: exact)
        i = torch.tensor([1 + k % 5, 1 + k % 7, 1 + k % 9], dtype=F32)
        p = lo + (hi - lo) * (i / torch.tensor([d - 1.0 for d in EG_DIMS]))
        if k:                                                            # (x, z land beside an integer: inside the band; one point of these)
            r = torch.rand(2, generator=g)
            p[0], p[2] = lo[0] + (hi[0] - lo[0]) * r[0], lo[2] + (hi[2] - lo[2]) * r[1]
        pts.append(p)
    for k in range(40):                                                  # up to 1.5 voxels outside on every side
        p = lo + (hi - lo) * torch.rand(3, generator=g)
        a, side = k % 3, (k // 3) % 2
        d = vox[a] * (1.5 if k < 6 else 1.5 * torch.rand(1, generator=g)[0])
        p[a] = hi[a] + d if side else lo[a] - d
        if k >= 30:                                                      # outside on all three axes
            p = torch.where(torch.rand(3, generator=g) < 0.5, lo - 1.2 * vox * torch.rand(3, generator=g),
                            hi + 1.2 * vox * torch.rand(3, generator=g))
        pts.append(p)
    n_planted = len(pts)
    base = lo + vox * torch.tensor([3.0, 4.0, 5.0])
    pile = base + vox * (0.05 + 0.9 * torch.rand(300, 3, generator=g))   # 300 samples in one cell
    rest = lo + (hi - lo) * torch.rand(5000, 3, generator=g)
    return torch.cat([torch.stack(pts), pile, rest])[:5000].contiguous(), n_planted


def case_expgrad(name):
    if ("eg", name) in _CACHE:
        return _CACHE[("eg", name)]
    mode, n, noise, zero_pad, claims = EXPGRAD_CASES[name]
    g = torch.Generator().manual_seed(1000 + list(EXPGRAD_CASES).index(name))
    sdf = torch.randn(*EG_DIMS, generator=g)
    d = dict(name=name, lo=EG_LO, hi=EG_HI, dims=EG_DIMS, sdf=sdf, zero_pad=zero_pad, eps=0.003, near=0.05, stepdist=0.11,
             claims=set(claims))
    ncell = sdf.numel()
    d["grad0"] = (torch.sin(torch.arange(ncell, dtype=F32)) * 0.5).reshape(EG_DIMS)
    census = set()
    if mode == "pts":
        allp, n_planted = _expgrad_points_set(torch.Generator().manual_seed(77))
        d["pts"] = allp[:n].contiguous()
        if noise:
            nz = torch.randn(n, 3, generator=g)
            nz[:n_planted] = 0.0                                          # the planted points stay exact
            d["noise"] = nz
    else:
        nr = 40
        o = EG_LO + (EG_HI - EG_LO) * (0.2 + 0.6 * torch.rand(nr, 3, generator=g))
        dr = torch.randn(nr, 3, generator=g)
        d["rays_o"], d["rays_d"] = o, dr
        _, _, ns = ray_geom(o, dr, EG_LO, EG_HI, d["near"], d["stepdist"])
        rr, rs = [], []
        for r in range(nr):
            last = int(ns[r]) - 1
            for s in sorted({0, last // 2, last}):
                if len(rr) % 7 == 6:
                    rr.append(-1), rs.append(3)
                rr.append(r), rs.append(s)
        d["rec_ray"], d["rec_step"] = torch.tensor(rr, dtype=torch.int32), torch.tensor(rs, dtype=torch.int32)
        d["n_steps"] = ns
        n = len(rr)
        if noise:
            d["noise"] = torch.randn(n, 3, generator=g)
        census |= {"ray mode", "rec_ray = -1"}
        live = d["rec_ray"] >= 0
        if bool((d["rec_step"][live] == 0).any()):
            census.add("step 0")
        if bool((d["rec_step"][live].long() == ns[d["rec_ray"][live].long()] - 1).any()):
            census.add("last step")
    d["n"] = n
    d["g"] = torch.randn(n, 4, generator=g)
    # census from the restatement's own index
    p, live = expgrad_points(d)
    idx, _ = expgrad_index(d, p, "q")
    v, top = idx.v, torch.tensor([k - 1.0 for k in EG_DIMS], dtype=F64)
    exact = idx.E == 0
    at_lo, at_hi = (v == 0) & exact, (v == top) & exact
    if bool((at_lo | at_hi).all(1).any()):
        census.add("box corner")
    if bool(((at_lo | at_hi).sum(1) == 1).any()):
        census.add("face")
    if bool(((v == torch.round(v)) & exact & (v > 0) & (v < top)).any()):
        census.add("integer index")
    if bool((((v < 0) | (v > top)) & live[:, None]).any()):
        census.add("outside the box")
    fl = torch.floor(v)
    cellid = (fl[:, 0] * 100 + fl[:, 1]) * 100 + fl[:, 2]
    most = int(torch.unique(cellid, return_counts=True)[1].max())
    if most >= 100:
        census.add("pile in one cell")
    if most >= 300:
        census.add("pile of 300 in one cell")
    if n > 256:
        census.add("second workgroup")
    if noise:
        census.add("noise")
    if zero_pad:
        census.add("zero_pad")
    d["census"] = census
    _CACHE[("eg", name)] = d
    return d


DIRS_CASES = {"p1": (1, 2), "p37": (37, 65), "p3": (3, 257)}


def case_dirs(name, rays=False):
    P, R1 = DIRS_CASES[name]
    g = torch.Generator().manual_seed(2000 + P)
    nrm = torch.nn.functional.normalize(torch.randn(P, 3, generator=g), dim=-1)
    raw = torch.randn(P, R1, 3, generator=g)
    nrm[0] = torch.tensor([0.0, 0.0, 1.0])
    raw[0, 0] = 0.0                                                      # norm 0: the 1e-12 clamp
    raw[0, 1] = torch.tensor([3.0, 4.0, 0.0])                            # exactly perpendicular: dt = 0, no flip
    census = {"norm 0", "dt = 0"}
    if R1 > 2:
        raw[0, 2] = torch.tensor([1e-20, -1e-20, 1e-20])
        raw[0, 3] = torch.tensor([0.3, 0.4, -1e-9])                      # dt within a few ulp of 0
        census.add("1e-20 magnitude")
    d = dict(name=name, raw=raw, normal=nrm, P=P, R1=R1, census=census, claims=set(census))
    if rays:
        d["pts"] = torch.randn(P, 3, generator=g)
    return d


def case_dirs_rays(name):
    return case_dirs(name, True)


def case_emit(name="n64"):
    g = torch.Generator().manual_seed(3000)
    n = 64
    emit = torch.rand(n, 3, generator=g) * 4.0 + 1e-3
    emit[:5] = emit[:5, :1]                                              # grey
    modes = torch.arange(n) % 5
    inten = torch.rand(n, generator=g) * 3.0
    cols = torch.rand(n, 2, generator=g)
    hues = [1.0, 0.0, 1.0 / 6, 2.0 / 6, 0.5, 4.0 / 6, 5.0 / 6, 0.999999, 0.25, 0.75]
    cm = torch.nonzero((modes == 3) | (modes == 4))[:, 0]
    for k, h in enumerate(hues + hues):
        cols[cm[k], 0] = h
    cols[cm[0], 1], cols[cm[1], 1], cols[cm[2], 1], cols[cm[3], 1] = 0.0, 1.0, 1.0, 0.0
    census = {f"mode {int(m)}" for m in torch.unique(modes)}
    hc, sc = cols[cm, 0], cols[cm, 1]
    if bool((hc == 1.0).any()):
        census.add("hue 1.0")
    if bool(((hc.double() * 6).float() == torch.round(hc * 6)).any()):
        census.add("hue on a sector boundary")
    if bool((sc == 0).any()) and bool((sc == 1).any()):
        census.add("saturation 0 and 1")
    claims = {"mode 0", "mode 1", "mode 2", "mode 3", "mode 4", "hue 1.0", "hue on a sector boundary", "saturation 0 and 1"}
    return dict(name=name, emit=emit, modes=modes.long(), inten=inten, colors=cols, census=census, claims=claims)


def _ro_above_threshold():
    """the smallest binary32 roughness whose rounded square is above 1e-7f (two ulps above it; none lands on it)"""
    r = torch.tensor(math.sqrt(1e-7), dtype=F32)
    for _ in range(8):
        if float((r.double() ** 2).float()) > EPS32:
            return r
        r = torch.nextafter(r, torch.tensor(1.0))
    raise AssertionError("no roughness above the threshold")


# name: (P, R, J, pdra, umask given)
COMBINE_CASES = {
    "p1r1j1": (1, 1, 1, 0, True), "p3r64j1": (3, 64, 1, 0, False), "p10r8j48": (10, 8, 48, 0, True),
    "p10r8j48_pdra": (10, 8, 48, 1, True), "p5r257j64_pdra": (5, 257, 64, 1, True), "p7r300j48": (7, 300, 48, 0, True),
}


def case_combine(name):
    if ("cb", name) in _CACHE:
        return _CACHE[("cb", name)]
    P, R, J, pdra, has_um = COMBINE_CASES[name]
    g = torch.Generator().manual_seed(4000 + list(COMBINE_CASES).index(name))
    rnd = lambda *s: torch.rand(*s, generator=g)
    nz = lambda *s: torch.randn(*s, generator=g)
    unit = lambda t: torch.nn.functional.normalize(t, dim=-1)
    base, metal = rnd(P, 3), rnd(P)
    rough = torch.exp(math.log(3e-4) + (0.0 - math.log(3e-4)) * rnd(P))                # log-uniform in [3e-4, 1]
    nrm, view = unit(nz(P, 3)), unit(nz(P, 3))
    raw = nz(P, R + 1, 3)
    dirs = unit(raw)
    dirs = torch.where(((dirs * nrm[:, None]).sum(-1) < 0)[..., None], -dirs, dirs)
    census = set()
    if P >= 3:
        nrm[0], view[0] = torch.tensor([0.0, 0.0, 1.0]), torch.tensor([-0.75, 0.0, -0.5])
        dirs[0, 0] = torch.tensor([-0.75, 0.0, 0.5])                     # wi + wo = (0, 0, 1): h = n and n.h = 1 with E = 0
        rough[0] = 1e-5                                                  # r2 < 1e-7: D ~ 3e6 on that ray only
        if R >= 8:
            dirs[1, 1] = view[1]                                         # wi = view: wi + wo = 0, the half-vector clamp
            census.add("wi + wo = 0")
        rough[2] = _ro_above_threshold()                                 # (with n.h = 1 on a ray, or D and its slope are 0 there)
        nrm[2], view[2], dirs[2, 0] = nrm[0], view[0], dirs[0, 0]
        census |= {"r2 < 1e-7 with n.h = 1", "r2 on the first square above 1e-7"}
    mus, lambdas, lobes = nz(J, 3) * 0.3, 10 + 20 * nz(J), nz(J, 3)
    if J >= 48:
        lambdas[0], lambdas[1], lambdas[2], lambdas[3] = 0.0, -7.5, 1e3, 4.0
        lobes[5] = torch.tensor([1e-20, 0.0, -1e-20])
        lobes[3] = nrm[min(3, P - 1)]
        mus[3] = torch.tensor([40.0, 25.0, -40.0])
        census |= {"lambda 0", "lambda negative", "lambda 1e3", "lobe of norm 1e-20"}
    elif name == "p1r1j1":
        lambdas[0] = -3.0
        census.add("lambda negative")
    off_m, emo_m, last2 = rnd(P * R, 3) * 2, rnd(P * R, 3) * 2, rnd(P * R)
    if R >= 300:
        last2.view(P, R)[3, 64:128] = 0.0                                # one full wave with nothing for the lobes
        census.add("last2 = 0 on a whole wave")
    if R % 256 == 1 and R > 256:
        census.add("one ray in the second trip")
    if R > 256:
        census.add("second trip")
    emission = rnd(P, 3)
    umask = (torch.arange(P) % 3 == 0).to(torch.uint8) if has_um else None
    if not has_um:
        census.add("umask NULL")
    if pdra and has_um:
        census |= {"pdra certain points", "pdra uncertain points"}
    census.add(f"n_sg = {J}")
    d = dict(name=name, P=P, R=R, J=J, pdra=pdra, base=base, rough=rough, metal=metal, normal=nrm, view=view, dirs=dirs,
             off_m=off_m, emo_m=emo_m, last2=last2, mus=mus, lambdas=lambdas, lobes=lobes, emission=emission, umask=umask,
             g_off_hat=nz(2 * P, 3), g_emo_hat=nz(2 * P, 3),
             d_mus0=torch.sin(torch.arange(J * 3, dtype=F32)).reshape(J, 3), d_lambdas0=torch.cos(torch.arange(J, dtype=F32)),
             d_lobes0=torch.sin(1.0 + torch.arange(J * 3, dtype=F32)).reshape(J, 3) * 2.0)
    c = _combine_common(d, "64")
    if bool((c["pre"] > 20).any()) and bool((c["pre"] <= 20).any()):
        census.add("pre-activation above 20")
    D0 = c["d"][0][4]["D"]
    live = D0[D0 > 0]
    if live.numel() and float(live.max() / live.min()) > 1e6:
        census.add("D spans decades")
    d["census"] = census
    claims = {f"n_sg = {J}"}
    if J >= 48:
        claims |= {"lambda 0", "lambda negative", "lambda 1e3", "lobe of norm 1e-20", "pre-activation above 20"}
    if P >= 3:
        claims |= {"r2 < 1e-7 with n.h = 1", "D spans decades"}
    if P >= 3 and R >= 8:
        claims.add("wi + wo = 0")
    if name == "p5r257j64_pdra":
        claims |= {"one ray in the second trip", "pdra certain points", "pdra uncertain points"}
    if name == "p7r300j48":
        claims |= {"last2 = 0 on a whole wave", "second trip"}
    if not has_um:
        claims.add("umask NULL")
    d["claims"] = claims
    _CACHE[("cb", name)] = d
    return d


# =======================================================================================================================
# the operations, their families and the mutants
# =======================================================================================================================
def _plain(ref_fn):
    def verify(inp, got, K):
        r = ref_fn(inp)
        worst, fails = compare(r, got, K)
        return r, worst, fails
    return verify


# op -> (case builder, case names, verify(inp, got, K) -> (ref, worst, fails), binary32 emulation, family, C entry points)
OPS = {
    "expgrad_fwd": (case_expgrad, list(EXPGRAD_CASES), verify_expgrad_fwd, emu_expgrad_fwd, "expgrad", ("esr_expgrad_fwd",)),
    "expgrad_bwd": (case_expgrad, list(EXPGRAD_CASES), verify_expgrad_bwd, emu_expgrad_bwd, "expgrad", ("esr_expgrad_bwd",)),
    "lts_dirs": (case_dirs, list(DIRS_CASES), verify_dirs, emu_lts_dirs, "dirs+edit", ("esr_lts_dirs",)),
    "lts_dirs_rays": (case_dirs_rays, list(DIRS_CASES), verify_dirs, emu_lts_dirs, "dirs+edit", ("esr_lts_dirs_rays",)),
    "emit_edit": (case_emit, ["n64"], _plain(ref_emit_edit), emu_emit_edit, "dirs+edit", ("esr_emit_edit",)),
    "lts_combine_fwd": (case_combine, list(COMBINE_CASES), _plain(ref_lts_combine_fwd), emu_lts_combine_fwd, "combine",
                        ("esr_lts_combine_fwd",)),
    "lts_combine_bwd": (case_combine, list(COMBINE_CASES), _plain(ref_lts_combine_bwd), emu_lts_combine_bwd, "combine",
                        ("esr_lts_combine_bwd",)),
}


def build(op, case):
    return OPS[op][0](case)


def all_cases():
    return [(op, case) for op, spec in OPS.items() for case in spec[1]]


def verify(op, inp, got, K):
    r, worst, fails = OPS[op][2](inp, got, K)
    if not hasattr(r, "flips") or r.flips is None:
        r.flips = {}
    return r, worst, fails


# K per family, for both test files: the next power of two at or above twice the worst ratio |gpu - ref| / (U absref) measured on the
# MI355X over every case of test_gpu_lts_ref64.py (printed under -s); the factor two leaves room for the order of the float atomics.
# The binary32 emulation reaches the same worst ratios to two digits (they seeded the constants before the GPU run).
K_FAMILY = {
    "expgrad": 2,       # measured worst 0.652 (esr_expgrad_bwd; esr_expgrad_fwd 0.585; one banded point per explicit-point case flipped)
    "dirs+edit": 2,     # 0.845 (esr_emit_edit; esr_lts_dirs and esr_lts_dirs_rays 0.667; no hemisphere decision flipped)
    "combine": 2,       # 0.977 (esr_lts_combine_bwd; esr_lts_combine_fwd 0.479)
}

# mutant of the emulation -> the ops it applies to; each must break the bound on at least one case of each of those ops.
# r2_clamp_no_grad_at_threshold stands for "the r2 clamp passes no gradient at equality": equality itself is unreachable (module
# docstring), so the mutant blocks the gradient up to the first reachable square above 1e-7f, where a roughness is planted.
MUTANTS = {
    "mean_divides_by_256": ["lts_combine_fwd", "lts_combine_bwd"],
    "wave_last_lane_dropped": ["lts_combine_fwd", "lts_combine_bwd"],
    "second_trip_inactive_contribute": ["lts_combine_fwd", "lts_combine_bwd"],
    "dlambda_without_sign": ["lts_combine_bwd"],
    "lobe_not_projected": ["lts_combine_bwd"],
    "pdra_detach_ignored": ["lts_combine_bwd"],
    "demission_on_certain": ["lts_combine_bwd"],
    "accumulated_overwritten": ["lts_combine_bwd", "expgrad_bwd"],
    "wo1_from_view": ["lts_combine_fwd", "lts_combine_bwd"],
    "r2_clamp_no_grad_at_threshold": ["lts_combine_bwd"],
    "weights_after_clamp": ["expgrad_fwd", "expgrad_bwd"],
    "zero_pad_ignored": ["expgrad_fwd", "expgrad_bwd"],
    "scale_wrong_axis": ["expgrad_fwd", "expgrad_bwd"],
    "hue_sector_off_by_one": ["emit_edit"],
    "flip_ignored": ["lts_dirs", "lts_dirs_rays"],
}
