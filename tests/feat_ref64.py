"""Float64 restatement of the fine feature kernels (csrc/feat.hip: feat_fwd_kernel and feat_bwd_kernel) and a mirror of the
backward's window bookkeeping, used by tests/feat_check.py (the comparison), tests/feat_emu.py (the binary32 emulation) and
their two tests; never imported by the product path.

What the kernels compute in binary32 before any sum is formed -- the sample position (the sampler's replay), its continuous
grid index, the clamped stencil tap coordinates -- is replayed here in binary32, op for op (torch's float32 ops round each
result once, like the kernels' `fp contract(off)` blocks); every weight, product and sum after that is float64.  The kernels'
remaining error is then a few roundings per term, so each cell is checked against K * 2^-24 * absref, where absref is the
same scatter evaluated on magnitudes: every input replaced by its absolute value and every difference by a sum.  That bound
holds for a cell whatever the scale of the rest of the grid.

The backward is a function of what its ABI takes: positions, the forward tile's normal rows and gnorm (binary32, as read by
the kernel), the dX rows of the sources, dsdf_extra, grad4.  Scatter output: a sparse map cell -> (value, absref) per grid.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np
import torch

F32, F64 = torch.float32, torch.float64
XROWS, DXROWS = 104, 64
ROW_SDF, ROW_FEAT, ROW_NRM = 6, 7, 31
ROW_XYZ, ROW_SIN, ROW_COS, ROW_VD, ROW_VSIN, ROW_VCOS = 43, 46, 61, 76, 79, 82
COLOR_ROW = (0, 88, 96)          # first row of the three 6-row colour groups
ZERO_ROWS = (85, 86, 87, 94, 95, 102, 103)
U = 2.0 ** -24
WIN_CELLS = 2560                 # feat.hip: WIN_CELLS
SDF_GID = 0                      # grid id of the SDF gradient; colour grids: colour_gid(src, on)


def colour_gid(src: int, on: bool) -> int:
    return 1 + 2 * src + (0 if on else 1)


# K per family of feat_check: |got - ref| <= K * 2^-24 * absref + FLOOR.  Twice the larger of the two measured worst ratios
# (feat_bwd / feat_fwd kernels on the MI355X, tests/test_gpu_feat_scatter.py -s; the binary32 emulation feat_emu.py on the
# host cases, tests/test_feat_ref64_host.py -s), rounded up to a power of two, never above the 8 that K_BWD = K_FWD = 8 were.
# colour and stencil: twice the measured worst is above 8, so they keep the 8 they had, with a margin of 1.9 and 1.7 instead of 2.
# Their rounding model allows more than was seen: an 8-corner fma chain has three weight differences and two products per
# corner and up to 8 roundings of partial sums, each <= 1 unit of 2^-24 * absref; 4.15 and 4.68 of those 13 were reached, by the
# kernel and by the emulation on the same samples.  pe: the kernel's sincosf reaches 2.008 (just over 1 ulp of the result;
# the emulation's correctly rounded sin / cos: 1.0), which the rule turns into 8.
K_FAMILY = {
    # family            K      measured worst: kernel / emulation
    "colour":           8,   # 4.150 / 4.150   rows 0-5, 88-93, 96-101
    "stencil":          8,   # 4.677 / 4.677   rows 7-30
    "normal":           4,   # 1.018 / 1.018   rows 31-42 (scale: first order through the quotient and F.normalize)
    "gnorm":            8,   # 3.286 / 2.703
    "pe":               8,   # 2.008 / 0.996   rows 46-75, scale |ref|
    "view":             4,   # 1.473 / 0.987   rows 76-84 (the input rows exactly)
    "sdf fit":          8,   # 3.122 / 2.836   cells reached only by terms of lanes whose window fits
    "sdf global":       8,   # 2.947 / 3.097   cells reached by at least one global-atomic term
    "sdf grad4":        8,   # 3.312 / 2.356   cells reached by a grad4 term
    "colour grid":      8,   # 3.150 / 3.092
}
# exact families (no K): "sdf value", "unit", "zero rows", "padding", "x16", "dsdf_out", "untouched", "finite"
EXACT_FAMILIES = ("sdf value", "unit", "zero rows", "padding", "x16", "dsdf_out", "untouched", "finite")


def row_families():
    """family of each of the 104 rows of the X tile"""
    fam = [None] * XROWS
    for r0 in COLOR_ROW:
        fam[r0:r0 + 6] = ["colour"] * 6
    fam[ROW_SDF] = "sdf value"
    fam[ROW_FEAT:ROW_FEAT + 24] = ["stencil"] * 24
    fam[ROW_NRM:ROW_NRM + 12] = ["normal"] * 12
    fam[ROW_XYZ:ROW_XYZ + 3] = ["unit"] * 3
    fam[ROW_SIN:ROW_SIN + 30] = ["pe"] * 30
    fam[ROW_VD:ROW_VD + 9] = ["view"] * 9
    for r in ZERO_ROWS:
        fam[r] = "zero rows"
    assert None not in fam
    return fam


def round_bf16(x64):
    """float64 -> the nearest bfloat16 value (ties to even), as float64; one rounding (no detour through binary32)"""
    m, e = torch.frexp(x64)
    return torch.ldexp(torch.round(m * 256.0) / 256.0, e)


X16_SLOT = [8 * ((s >> 1) & 3) + 2 * (s >> 3) + (s & 1) for s in range(32)]     # sample -> slot of the row-quad tile


def x16_decode(q):
    """esr_fine_feat_fwd_x16's tile [tiles, 26, 32 slots, 4 rows in quad] -> rows 0..95 [tiles, 96, 32 samples] and the two
    alternate quads [tiles, 8, 32] (rows 88..93, 6, 7), as float64"""
    tiles = q.shape[0]
    q = q.double()[:, :, X16_SLOT, :]
    return q[:, :24].permute(0, 1, 3, 2).reshape(tiles, 96, 32), q[:, 24:26].permute(0, 1, 3, 2).reshape(tiles, 8, 32)


@dataclass
class Src:
    dX: torch.Tensor                     # [tiles, 64, 32] float32
    t0: int
    t1: int
    on: bool = False                     # has a grad_color_on grid
    off: bool = False                    # has a grad_color_off grid


@dataclass
class Case:
    """Inputs of one esr_fine_feat_fwd / _bwd pair (CPU tensors)."""
    lo: torch.Tensor                     # xyz_min [3] float32
    hi: torch.Tensor
    dims: tuple
    vox: float
    stepdist: float
    grad_feat: tuple
    tiles_all: int
    tiles_on: int = 0
    near: float = 0.0
    pts: Optional[torch.Tensor] = None   # explicit points [n_pts, 3] ...
    pt_sdf: Optional[torch.Tensor] = None
    rays_o: Optional[torch.Tensor] = None  # ... or march records
    rays_d: Optional[torch.Tensor] = None
    rec_ray: Optional[torch.Tensor] = None
    rec_step: Optional[torch.Tensor] = None
    rec_sdf: Optional[torch.Tensor] = None
    sdf: Optional[torch.Tensor] = None   # [X, Y, Z] float32
    color_on: Optional[torch.Tensor] = None   # group-0 colour grid [X, Y, Z, 6] on on-tiles / other tiles
    color_off: Optional[torch.Tensor] = None
    color_on1: Optional[torch.Tensor] = None  # groups 1 and 2 (rows 88-93, 96-101): any of them absent
    color_on2: Optional[torch.Tensor] = None
    color_off1: Optional[torch.Tensor] = None
    color_off2: Optional[torch.Tensor] = None
    viewdirs: Optional[torch.Tensor] = None   # per ray [R, 3] (record mode; None: rays_d normalised)
    pt_viewdirs: Optional[torch.Tensor] = None  # per point [n_pts, 3] (explicit points; None: zeros)
    srcs: List[Src] = field(default_factory=list)
    grad_sdf: bool = True
    dsdf_extra: Optional[torch.Tensor] = None  # [tiles*32]
    dsdf_out: bool = False
    grad4: Optional[torch.Tensor] = None       # [tiles*32, 4]
    grad4_mode: int = 0

    @property
    def n_pts(self):
        return 0 if self.pts is None else self.pts.shape[0]

    def colour_grids(self, on: bool):
        return [self.color_on, self.color_on1, self.color_on2] if on else [self.color_off, self.color_off1, self.color_off2]

    def view_inputs(self):
        """the view direction per sample slot [tiles*32, 3] binary32 (padding lanes: 0)"""
        n = self.tiles_all * 32
        v = torch.zeros(n, 3, dtype=torch.float32)
        if self.pts is not None:
            if self.pt_viewdirs is not None:
                v[:self.n_pts] = self.pt_viewdirs
            return v
        vd = self.viewdirs if self.viewdirs is not None else torch.nn.functional.normalize(self.rays_d, dim=-1)
        r = self.rec_ray.long()
        return torch.where((r >= 0)[:, None], vd[r.clamp_min(0)], v)

    def launch_range(self):
        """esr_fine_feat_bwd's [t_begin, t_end) (feat.hip, the host entry)."""
        if self.dsdf_extra is not None or self.dsdf_out or self.grad4 is not None:
            return 0, self.tiles_all
        lo = min([self.tiles_all] + [s.t0 for s in self.srcs])
        hi = max([0] + [s.t1 for s in self.srcs])
        return max(lo, 0), min(hi, self.tiles_all)


# ---- binary32 replays -------------------------------------------------------------------------------------------------
# Every binary32 op is formed in float64 and rounded once to binary32: correctly rounded for + - * / and sqrt (53 >= 2 * 24 + 2
# bits), so the replay does not depend on which vector paths the host's torch takes for float32.
def _f(v):
    return torch.tensor(v, dtype=F32)


def _r(x, like=None):
    """round a float64 result to the working precision: binary32, or float64 when `like` is a float64 tensor"""
    return x if (like is not None and like.dtype == F64) else x.to(F32)


def ray_geom(rays_o, rays_d, lo, hi, near, stepdist):
    """esr_ray_geom (esr_common.h, far = 1e9) per ray, binary32: start [N,3], unit direction [N,3] and n_steps [N] int64."""
    o, d = rays_o.double(), rays_d.double()
    lo, hi = lo.double(), hi.double()
    v = torch.where(d == 0, _f(1e-6).double(), d)
    ta, tb = _r(_r(hi - o).double() / v).double(), _r(_r(lo - o).double() / v).double()
    mn, mx = torch.minimum(ta, tb), torch.maximum(ta, tb)
    lo_t = torch.maximum(torch.maximum(mn[:, 0], mn[:, 1]), mn[:, 2])
    hi_t = torch.minimum(torch.minimum(mx[:, 0], mx[:, 1]), mx[:, 2])
    far, nr = _f(1e9).double(), _f(near).double()
    tmin = torch.maximum(torch.minimum(lo_t, far), nr)
    tmax = torch.maximum(torch.minimum(hi_t, far), nr)
    sq = lambda a: _r(a * a).double()
    nrm = _r(torch.sqrt(_r(_r(sq(d[:, 0]) + sq(d[:, 1])).double() + sq(d[:, 2])).double())).double()
    length = _r(_r(_r(tmax - tmin).double() * nrm).double() / _f(stepdist).double())
    n_steps = torch.ceil(length).double().clamp_min(1.0).long()
    start = _r(o + _r(d * tmin[:, None]).double())
    dirv = _r(d / nrm[:, None])
    return start, dirv, n_steps


def ray_point(start, dirv, stepdist, step):
    """esr_ray_point, binary32: sample `step` [M] of rays with start / dirv [M,3]."""
    dist = _r(_f(stepdist).double() * step.double()).double()
    return _r(start.double() + _r(dirv.double() * dist[:, None]).double())


def record_points(case: Case):
    """esr_ray_geom + esr_ray_point (esr_common.h) per record: positions [tiles*32, 3] float32 and the valid mask."""
    r = case.rec_ray.long()
    valid = r >= 0
    start, dirv, _ = ray_geom(case.rays_o[r.clamp_min(0)], case.rays_d[r.clamp_min(0)], case.lo, case.hi, case.near,
                              case.stepdist)
    p = ray_point(start, dirv, case.stepdist, case.rec_step)
    return torch.where(valid[:, None], p, torch.zeros_like(p)), valid


def positions(case: Case):
    n = case.tiles_all * 32
    if case.pts is not None:
        p = torch.zeros(n, 3, dtype=F32)
        p[:case.n_pts] = case.pts
        valid = torch.arange(n) < case.n_pts
        return p, valid
    return record_points(case)


def world_to_index(case: Case, p):
    """esr_world_to_index, binary32."""
    top = torch.tensor([d - 1 for d in case.dims], dtype=F64)
    lo, hi = case.lo.double(), case.hi.double()
    u = _r(_r(p.double() - lo).double() / _r(hi - lo).double()).double()
    n = _r(_r(u * 2.0).double() - 1.0).double()
    return _r(_r(_r(n + 1.0).double() / 2.0).double() * top)


def tap_index(case: Case, ind, axis, disp):
    """tap_index (esr_common.h), binary32: the tap's continuous index [M,3] and its clamped coordinate along `axis`."""
    top = torch.tensor([d - 1 for d in case.dims], dtype=F64)
    t = ind.double().clone()
    t[:, axis] = _r(t[:, axis] + float(_f(disp))).double()
    t = torch.minimum(torch.maximum(t, torch.zeros(3, dtype=F64)), top)
    n = _r(_r(_r(t / top).double() * 2.0).double() - 1.0).double()
    return _r(_r(_r(n + 1.0).double() / 2.0).double() * top), _r(t[:, axis])


# ---- float64 trilinear terms ------------------------------------------------------------------------------------------
def _corners(ix32):
    """8 corners of a trilinear lookup at binary32 indices [M,3]: integer cells [M,8,3] and float64 weights [M,8] in
    ATen's spelling (exact: every factor is a difference of two nearby binary32 values)."""
    fl = torch.floor(ix32)
    i0 = fl.long()
    ix, f = ix32.double(), fl.double()
    cells, ws = [], []
    for cx in (0, 1):
        for cy in (0, 1):
            for cz in (0, 1):
                c = torch.stack([i0[:, 0] + cx, i0[:, 1] + cy, i0[:, 2] + cz], -1)
                w = torch.ones(ix.shape[0], dtype=F64)
                for a, ca in enumerate((cx, cy, cz)):
                    w = w * ((ix[:, a] - f[:, a]) if ca else ((f[:, a] + 1) - ix[:, a]))
                cells.append(c)
                ws.append(w)
    return torch.stack(cells, 1), torch.stack(ws, 1)


def _inb(c, dims):
    return ((c >= 0) & (c < torch.tensor(dims))).all(-1)


def _flat(c, dims):
    return (c[..., 0] * dims[1] + c[..., 1]) * dims[2] + c[..., 2]


def fetch(grid64, dims, ix32, ch=1):
    """Zero-padded trilinear fetch in float64: value and sum of |tap * weight| ([M] or [M, ch])."""
    cells, w = _corners(ix32)
    ok = _inb(cells, dims)
    fl = torch.where(ok, _flat(cells.clamp_min(0), dims), torch.zeros_like(ok, dtype=torch.long))
    fl = torch.minimum(fl, torch.tensor(grid64.shape[0] - 1))
    w = torch.where(ok, w, torch.zeros_like(w))
    g = grid64[fl]                                        # [M, 8] or [M, 8, ch]
    if ch > 1:
        w = w[..., None]
    return (g * w).sum(1), (g * w).abs().sum(1)


# ---- forward ----------------------------------------------------------------------------------------------------------
def forward_rows(case: Case, p, valid):
    """All 104 rows of the X tile and gnorm per sample (valid samples only): float64 values and per-element error scales
    (|x - ref| <= K 2^-24 scale is the check; scale 0: the row is exact).  Normal rows: first-order propagation of the taps'
    scales through the difference quotient and F.normalize (|d n| <= 2 |d g| / |g|).  `unit` is replayed in binary32
    (__fdiv_rn(p - lo, hi - lo)); the sin / cos rows are float64 sin / cos of the binary32 argument unit * 2^i (an exact
    product) with scale |ref|: sinf / cosf are within 2 ulp of the result (shade_ref64.py's model).  View rows: the input and its
    float64 sin / cos.  Zero rows, the SDF value row and the view input rows are exact."""
    dims = case.dims
    ind = world_to_index(case, p[valid])
    M = ind.shape[0]
    t = torch.nonzero(valid)[:, 0] // 32
    on = t < case.tiles_on
    val = torch.zeros(M, XROWS, dtype=F64)
    scl = torch.zeros(M, XROWS, dtype=F64)
    for is_on, sel in ((True, on), (False, ~on)):
        for gi, grid in enumerate(case.colour_grids(is_on)):
            if grid is not None and bool(sel.any()):
                v, a = fetch(grid.double().reshape(-1, 6), dims, ind[sel], ch=6)
                val[sel, COLOR_ROW[gi]:COLOR_ROW[gi] + 6], scl[sel, COLOR_ROW[gi]:COLOR_ROW[gi] + 6] = v, a
    unit = _r(_r(p[valid].double() - case.lo.double()).double() / _r(case.hi.double() - case.lo.double()).double())
    val[:, ROW_XYZ:ROW_XYZ + 3] = unit.double()
    arg = unit.double()[:, :, None] * (2.0 ** torch.arange(5, dtype=F64))          # [M, 3, 5]: coordinate-major
    assert torch.equal(arg, arg.float().double())
    val[:, ROW_SIN:ROW_SIN + 15], val[:, ROW_COS:ROW_COS + 15] = torch.sin(arg).reshape(M, 15), torch.cos(arg).reshape(M, 15)
    vd = case.view_inputs()[valid].double()
    val[:, ROW_VD:ROW_VD + 3], val[:, ROW_VSIN:ROW_VSIN + 3], val[:, ROW_VCOS:ROW_VCOS + 3] = vd, torch.sin(vd), torch.cos(vd)
    for r0, n in ((ROW_SIN, 15), (ROW_COS, 15), (ROW_VSIN, 3), (ROW_VCOS, 3)):
        scl[:, r0:r0 + n] = val[:, r0:r0 + n].abs()
    sdfv = case.pt_sdf if case.pts is not None else case.rec_sdf
    sv = torch.zeros(case.tiles_all * 32, dtype=F32)
    sv[:sdfv.shape[0]] = sdfv
    val[:, ROW_SDF] = sv[valid].double()
    g64 = case.sdf.double().reshape(-1)
    grad = torch.zeros(M, 3, 4, dtype=F64)
    gabs = torch.zeros(M, 3, 4, dtype=F64)
    for ar in range(3):
        axis = 2 - ar
        for k in range(4):
            ixm, cm = tap_index(case, ind, axis, -case.grad_feat[k])
            ixp, cp = tap_index(case, ind, axis, case.grad_feat[k])
            fm, am = fetch(g64, dims, ixm)
            fp, ap = fetch(g64, dims, ixp)
            rm, rp = ROW_FEAT + 2 * ar * 4 + k, ROW_FEAT + (2 * ar + 1) * 4 + k
            val[:, rm], scl[:, rm], val[:, rp], scl[:, rp] = fm, am, fp, ap
            den = ((cp - cm).double() + 1e-12) * case.vox
            grad[:, ar, k] = (fp - fm) / den
            gabs[:, ar, k] = (am + ap) / den
    nrm = grad.norm(dim=1)                                # [M, 4]
    nabs = gabs.norm(dim=1)
    nz = nrm.clamp_min(1e-12)
    val[:, ROW_NRM:ROW_NRM + 12] = (grad / nz[:, None]).reshape(M, 12)
    scl[:, ROW_NRM:ROW_NRM + 12] = (2 * nabs / nz)[:, None, :].expand(M, 3, 4).reshape(M, 12)
    return val, scl, nrm, nabs


# ---- backward ---------------------------------------------------------------------------------------------------------
@dataclass
class Scatter:
    """Sparse result: per grid id, sorted flat indices with value / absref, and the raw terms (for failure reports)."""
    cells: dict
    terms: dict
    dsdf_out: Optional[torch.Tensor]


def _src_rows(case: Case, t, s, rows, absmode):
    """Sum over the sources covering tile t of dX rows (fp32 -> f64) [M, len(rows)]; covered mask [M]."""
    M = t.shape[0]
    acc = torch.zeros(M, len(rows), dtype=F64)
    cov = torch.zeros(M, dtype=torch.bool)
    for src in case.srcs:
        sel = (t >= src.t0) & (t < src.t1)
        if not bool(sel.any()):
            continue
        v = src.dX[t[sel]][:, rows, :].gather(2, s[sel][:, None, None].expand(-1, len(rows), 1))[..., 0].double()
        acc[sel] += v.abs() if absmode else v
        cov |= sel
    return acc, cov


def dsdf_rows32(case: Case, t, s):
    """r_dsdf of the kernel in binary32, summed in its order (sources in index order, then dsdf_extra)."""
    M = t.shape[0]
    r = torch.zeros(M, dtype=F32)
    for src in case.srcs:
        sel = (t >= src.t0) & (t < src.t1)
        r[sel] = r[sel] + src.dX[t[sel], ROW_SDF, s[sel]]
    if case.dsdf_extra is not None:
        r = r + case.dsdf_extra[t * 32 + s]
    return r


def _sdf_terms(case: Case, ind, t, s, nrow, gnrm, absmode):
    """The SDF grid's terms of feat_bwd_kernel phase 1 (value tap, 24 stencil taps through F.normalize, grad4):
    (flat cell, value) pairs [K] for the samples given (valid lanes of the launch range)."""
    dims = case.dims
    M = ind.shape[0]
    sub = (lambda a, b: a + b) if absmode else (lambda a, b: a - b)
    mag = (lambda x: x.abs()) if absmode else (lambda x: x)
    top = torch.tensor([d - 1 for d in dims], dtype=F32)
    indc = torch.minimum(torch.maximum(ind, _f(0.0)), top)
    i0c = torch.floor(indc).long()
    dn, _ = _src_rows(case, t, s, list(range(ROW_NRM, ROW_NRM + 12)), absmode)
    dn = dn.view(M, 3, 4)
    dF, _ = _src_rows(case, t, s, list(range(ROW_FEAT, ROW_FEAT + 24)), absmode)
    dF = dF.view(M, 3, 2, 4)                                      # [ar][minus/plus][k]
    r6, _ = _src_rows(case, t, s, [ROW_SDF], absmode)
    r_dsdf = r6[:, 0]
    j = t * 32 + s
    if case.dsdf_extra is not None:
        r_dsdf = r_dsdf + mag(case.dsdf_extra[j].double())
    self_v = bool(case.grad4_mode & 2)
    d_sdf = torch.zeros_like(r_dsdf) if (case.dsdf_out or self_v) else r_dsdf
    n = mag(nrow.double()).view(M, 3, 4)
    nrm = gnrm.double()                                           # [M, 4] (>= 0)
    big = gnrm > 1e-12
    dot = (n * dn).sum(1)                                         # [M, 4]
    inv = torch.where(big, 1.0 / nrm.clamp_min(1e-30), torch.full_like(nrm, 1e12))
    through = torch.where(big[:, None, :], sub(dn, n * dot[:, None, :]), dn) * inv[:, None, :]   # [M, 3(ar), 4]
    flats, vals = [], []
    for axis in range(3):
        ar = 2 - axis
        pb, pc = (1 if axis == 0 else 0), (1 if axis == 2 else 2)
        taps, ds = [], []
        for k in range(4):
            r = float(_f(case.grad_feat[k]))
            cm = _r(torch.clamp(_r(ind[:, axis].double() - r, ind).double(), 0.0, float(top[axis])), ind)
            cp = _r(torch.clamp(_r(ind[:, axis].double() + r, ind).double(), 0.0, float(top[axis])), ind)
            thr = through[:, ar, k] / ((cp - cm).double() + 1e-12) / case.vox
            taps += [cm, cp]
            ds += [sub(dF[:, ar, 0, k], thr), dF[:, ar, 1, k] + thr]
        if axis == 2:                                             # the value tap rides on the z bar
            taps.append(ind[:, 2])
            ds.append(d_sdf)
        tp = torch.stack(taps, 1).double()                        # [M, T]
        dd = torch.stack(ds, 1)
        iA = i0c[:, axis]
        cA = iA[:, None] - 2 + torch.arange(6)[None]              # [M, 6]
        # the bar's hat weights (feat.hip, deposit): t = ixA - (iA - 2) in binary32 -- exact for iA >= 2, rounded once
        # near the low faces, where t has a larger exponent than ixA -- then 1 - |t - o| exactly
        tb = _r(tp - (iA - 2).double()[:, None], ind).double()
        hat = (1 - (tb[:, :, None] - torch.arange(6, dtype=F64)).abs()).clamp_min(0)    # [M, T, 6]
        acc = (hat * dd[:, :, None]).sum(1)                       # [M, 6]
        ic = indc.double()
        wc = torch.stack([(i0c + 1).double() - ic, ic - i0c.double()], -1)   # [M, 3, 2]
        for b in (0, 1):
            for c in (0, 1):
                wgt = wc[:, pb, b] * wc[:, pc, c]
                cell = torch.zeros(M, 6, 3, dtype=torch.long)
                cell[:, :, axis] = cA
                cell[:, :, pb] = (i0c[:, pb] + b)[:, None]
                cell[:, :, pc] = (i0c[:, pc] + c)[:, None]
                ok = _inb(cell, dims)
                flats.append(torch.where(ok, _flat(cell, dims), -1))
                vals.append(acc * wgt[:, None])
    # folded exact-interpolant scatter (esr_expgrad_bwd's weights)
    if case.grad4 is not None or self_v:
        g4 = case.grad4[j].double() if case.grad4 is not None else torch.zeros(M, 4, dtype=F64)
        g4 = mag(g4)
        gv = g4[:, 0] + r_dsdf if self_v else g4[:, 0]
        scale = torch.tensor([(dims[a] - 1) / (float(case.hi[a]) - float(case.lo[a])) for a in range(3)], dtype=F64)
        gd = g4[:, 1:] * scale
        fl = torch.floor(ind)
        i0 = fl.long()
        ixd, fld = ind.double(), fl.double()
        wq = torch.stack([(fld + 1) - ixd, ixd - fld], -1)        # [M, 3, 2]
        for cx in (0, 1):
            for cy in (0, 1):
                for cz in (0, 1):
                    sx, sy, sz = [(1.0 if cc else -1.0) if not absmode else 1.0 for cc in (cx, cy, cz)]
                    u = torch.stack([i0[:, 0] + cx, i0[:, 1] + cy, i0[:, 2] + cz], -1)
                    cl = torch.minimum(torch.maximum(u, torch.zeros(3, dtype=torch.long)), torch.tensor(dims) - 1)
                    inb = (u == cl).all(-1)
                    wx, wy, wz = wq[:, 0, cx], wq[:, 1, cy], wq[:, 2, cz]
                    tv = gv * (wx * wy * wz) + gd[:, 0] * (sx * wy * wz) + gd[:, 1] * (wx * sy * wz) + gd[:, 2] * (wx * wy * sz)
                    f = _flat(cl, dims)
                    if case.grad4_mode & 1:
                        f = torch.where(inb, f, -1)
                    flats.append(f[:, None])
                    vals.append(tv[:, None])
    fl_all = torch.cat([f.reshape(M, -1) for f in flats], 1)
    v_all = torch.cat([v.reshape(M, -1) for v in vals], 1)
    return fl_all, v_all


def _colour_terms(case: Case, ind, t, s, src: Src, absmode):
    """Phase 2 of feat_bwd_kernel for one source: [M, 48] (flat index into [X,Y,Z,6], value)."""
    dims = case.dims
    M = ind.shape[0]
    d6 = src.dX[t][:, 0:6, :].gather(2, s[:, None, None].expand(-1, 6, 1))[..., 0].double()
    if absmode:
        d6 = d6.abs()
    cells, w = _corners(ind)
    ok = _inb(cells, dims)
    fl = torch.where(ok[..., None], _flat(cells, dims)[..., None] * 6 + torch.arange(6), -1)    # [M, 8, 6]
    return fl.reshape(M, 48), (w[:, :, None] * d6[:, None, :]).reshape(M, 48)


def _accumulate(flat, val, aval, tile, lane, g4):
    """terms -> cells; the raw terms keep their tile, sample slot (tile * 32 + lane) and whether they are grad4 terms"""
    keep = (flat >= 0) & (aval != 0)
    flat, val, aval, tile, lane, g4 = flat[keep], val[keep], aval[keep], tile[keep], lane[keep], g4[keep]
    u, inv = torch.unique(flat, return_inverse=True)
    v = torch.zeros(u.numel(), dtype=F64).index_add_(0, inv, val)
    a = torch.zeros(u.numel(), dtype=F64).index_add_(0, inv, aval)
    return (u, v, a), (flat, val, aval, tile, lane, g4)


def scatter(case: Case, X, gnorm, p=None, valid=None, ind=None):
    """Float64 esr_fine_feat_bwd: {gid: (flat cells, value, absref)} over the touched cells.  X [tiles,104,32] and gnorm
    [tiles,4,32] are the forward's binary32 outputs, read as the kernel reads them.  `ind` [tiles*32, 3] replaces the
    binary32 grid index (a float64 one makes the whole restatement float64)."""
    if p is None:
        p, valid = positions(case)
    tb, te = case.launch_range()
    jj = torch.nonzero(valid)[:, 0]
    t_all = jj // 32
    jj = jj[(t_all >= tb) & (t_all < te)]
    t, s = jj // 32, jj % 32
    ind = world_to_index(case, p[jj]) if ind is None else ind[jj]
    cells, terms = {}, {}
    dsdf = None
    if case.grad_sdf:
        nrow = X[t][:, ROW_NRM:ROW_NRM + 12, :].gather(2, s[:, None, None].expand(-1, 12, 1))[..., 0]
        gn = gnorm[t].gather(2, s[:, None, None].expand(-1, 4, 1))[..., 0]
        f, v = _sdf_terms(case, ind, t, s, nrow, gn, False)
        _, a = _sdf_terms(case, ind, t, s, nrow, gn, True)
        is_g4 = (torch.arange(f.shape[1]) >= 72)[None].expand_as(f)          # 3 bars x 4 corners x 6 cells, then grad4's 8
        cells[SDF_GID], terms[SDF_GID] = _accumulate(f.reshape(-1), v.reshape(-1), a.reshape(-1),
                                                     t[:, None].expand_as(f).reshape(-1),
                                                     jj[:, None].expand_as(f).reshape(-1), is_g4.reshape(-1))
        if case.dsdf_out:
            dsdf = dsdf_rows32(case, t, s), jj
    for k, src in enumerate(case.srcs):
        sel = (t >= src.t0) & (t < src.t1)
        on = t < case.tiles_on
        for is_on, has in ((True, src.on), (False, src.off)):
            m = sel & (on if is_on else ~on)
            if not has or not bool(m.any()):
                continue
            f, v = _colour_terms(case, ind[m], t[m], s[m], src, False)
            _, a = _colour_terms(case, ind[m], t[m], s[m], src, True)
            gid = colour_gid(k, is_on)
            cells[gid], terms[gid] = _accumulate(f.reshape(-1), v.reshape(-1), a.reshape(-1),
                                                 t[m][:, None].expand_as(f).reshape(-1),
                                                 jj[m][:, None].expand_as(f).reshape(-1),
                                                 torch.zeros_like(f, dtype=torch.bool).reshape(-1))
    return Scatter(cells, terms, dsdf)


# ---- path census: feat_bwd_kernel's segments and windows --------------------------------------------------------------
def _segments(key, valid, i0c, cut8):
    """segs_build (feat.hip): [(first, last, mn[3], mx[3])] of one tile."""
    heads = [bool(valid[s]) and (s == 0 or not valid[s - 1] or key[s] != key[s - 1]) for s in range(32)]
    if cut8:
        start = -1
        for s in range(32):
            if heads[s]:
                start = s
            if valid[s] and start >= 0 and (s - start) % 8 == 0:
                heads[s] = True
            # (a valid lane always has a head at or below it: a valid lane after a padding lane is one)
    out = []
    hs = [s for s in range(32) if heads[s]]
    for n, h in enumerate(hs):
        end = hs[n + 1] if n + 1 < len(hs) else 32
        members = [s for s in range(h, end) if valid[s]]
        c = i0c[members]
        out.append((h, members[-1], c.min(0), c.max(0)))
    return out


def _windows(segs, dims, below, above, ch):
    """seg_window (feat.hip): per segment (fits, clipped_lo, clipped_hi), and the tile's total."""
    base, res = 0, []
    for (_, _, mn, mx) in segs:
        lo = np.maximum(mn - below, 0)
        wd = np.maximum(np.minimum(mx + above, np.array(dims) - 1) - lo + 1, 0)
        cells = min(int(np.prod(wd.astype(np.int64))) * ch, WIN_CELLS + 1)
        fits = base + cells <= WIN_CELLS
        res.append((fits, bool((mn - below < 0).any()), bool((mx + above > np.array(dims) - 1).any())))
        base += cells
    return res, base


CLASSES = ("fit", "cut8_fit", "cut8_global", "global", "mixed", "clip_lo", "clip_hi", "colour_only", "small_norm")


def census(case: Case, p=None, valid=None, gnorm=None):
    """Per tile of the launch range: segments, probe total, cut8, window per segment and phase, the `has` flag per lane and
    phase, and the path classes (CLASSES) the tile takes.  `small_norm`: a valid lane of the tile takes the |g| <= 1e-12
    branch of the backward for some radius (needs `gnorm` [tiles, 4, 32], the forward's output; SDF launches only).
    Returns (per-tile list of dicts, {class: tile count})."""
    if p is None:
        p, valid = positions(case)
    dims = case.dims
    ind = world_to_index(case, p)
    top = torch.tensor([d - 1 for d in dims], dtype=F32)
    i0c = torch.floor(torch.minimum(torch.maximum(ind, _f(0.0)), top)).long().numpy()
    valid_np = valid.numpy()
    if case.pts is not None:
        # explicit points: runs split where consecutive valid points jump by more than 3 cells (key = run number)
        prev = np.roll(i0c, 1, 0)
        jump = valid_np & np.roll(valid_np, 1) & (np.abs(i0c - prev) > 3).any(1)
        jump[::32] = False
        keys = np.zeros(len(valid_np), dtype=np.int64)
        for t0 in range(0, len(valid_np), 32):
            keys[t0:t0 + 32] = np.cumsum(jump[t0:t0 + 32])
    else:
        keys = np.where(valid_np, case.rec_ray.numpy(), 0)
    tb, te = case.launch_range()
    phase2 = [any(src.t0 <= t < src.t1 and (src.on if t < case.tiles_on else src.off) for src in case.srcs)
              for t in range(case.tiles_all)]
    tiles, counts = [], {c: 0 for c in CLASSES}
    for t in range(tb, te):
        sl = slice(32 * t, 32 * t + 32)
        v, key, cc = valid_np[sl], keys[sl], i0c[sl]
        if not v.any():
            tiles.append(None)
            continue
        segs = _segments(key, v, cc, False)
        probe = (2, 3, 1) if case.grad_sdf else (0, 1, 6)
        _, total = _windows(segs, dims, *probe)
        cut8 = total > WIN_CELLS
        if cut8:
            segs = _segments(key, v, cc, True)
        phases = {}
        if case.grad_sdf:
            phases["sdf"] = _windows(segs, dims, 2, 3, 1)[0]
        if phase2[t]:
            phases["colour"] = _windows(segs, dims, 0, 1, 6)[0]
        cls = set()
        fit_all = all(f for w in phases.values() for f, _, _ in w)
        cls.add(("cut8_fit" if fit_all else "cut8_global") if cut8 else ("fit" if fit_all else "global"))
        for w in phases.values():
            if any(f for f, _, _ in w) and not all(f for f, _, _ in w):
                cls.add("mixed")
            if any(f and l for f, l, _ in w):
                cls.add("clip_lo")
            if any(f and h for f, _, h in w):
                cls.add("clip_hi")
        if not case.grad_sdf:
            cls.add("colour_only")
        elif gnorm is not None and bool((gnorm[t][:, torch.from_numpy(v)] <= 1e-12).any()):
            cls.add("small_norm")
        for c in cls:
            counts[c] += 1
        heads = [a for a, _, _, _ in segs]
        seg_of = [max([n for n, a in enumerate(heads) if a <= s_], default=-1) if v[s_] else -1 for s_ in range(32)]
        has = {k: [bool(v[s_]) and w[seg_of[s_]][0] for s_ in range(32)] for k, w in phases.items()}
        tiles.append(dict(tile=t, segs=[(a, b) for a, b, _, _ in segs], probe=total, cut8=cut8, has=has,
                          windows={k: [f for f, _, _ in w] for k, w in phases.items()}, classes=sorted(cls)))
    return tiles, counts
