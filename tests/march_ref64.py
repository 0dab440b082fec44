"""Float64 restatement of the ray march (csrc/march.hip: march_kernel, all four (COARSE, GA) variants) and of the plan
(plan_kernel, plan_totals_kernel), used only by the tests: tests/march_check.py (the comparison of a backend with this
restatement, run by tests/test_gpu_march_ref64.py on the kernels and by tests/test_march_ref64_host.py on the CPU),
tests/march_emu.py, tests/test_march_ref64_host.py and tests/test_march_ref64_autograd.py; never imported by the product path.

What the kernel computes before any sum is formed -- ray geometry, sample positions, continuous grid indices and the clamped
"grad"-mode tap indices -- is replayed in binary32, op for op (feat_ref64's replays); trilinear values, the finite differences,
the gg samples, sigmoid, alpha, transmittance and the whole backward are float64.

Decisions (in-box, a >= mask_thres, alpha > fast_thres, the early stop T < 1e-3, w > fast_thres, and relu' = [pc > nc] in the
backward) are the restatement's own unless the caller passes the kernel's (`Force`); a forced decision that differs from the
restatement's must lie on its boundary, within DEC_K * 2^-24 * E of it, where E is the first-order error bound of the quantity
the kernel compares (below).  Such flips are counted in `Fwd.flips`.

Error bounds are in units of U = 2^-24.  Per quantity q the restatement carries E_q, a first-order bound of |q_kernel - q| / U
from the kernel's binary32 evaluation:
  s (trilinear, fma over 8 corners, weights of 2 products)  E = 16 |s|abs          (|.|abs: the fetch on magnitudes)
  ic ("grad": 2 fetches, 2 divides, a 3-term dot, 2 products) E = 32 |ic|abs, coarse (one 3-channel fetch) 16 |ic|abs
  prv / nxt                                                 E = E_s (+ E_ic) + |prv|
  pc = sigmoid(prv s_val)                                   E = pc(1-pc) (s_val E_prv + |x|) + 4 pc      (expf: <= 2 ulp)
  alpha = (relu(pc - nc) + 1e-5) / (pc + 1e-5)             E = (E_num + alpha E_den) / den + alpha
  T (serial product)                                        E = T * sum over earlier visited samples of (E_alpha / (1 - alpha) + 2)
Backward values carry a magnitude M (the same computation on magnitudes: every difference a sum, including pc - nc, den - num
and gw T - back / (1 - alpha)) plus these E terms through first-order products; the kernel's 1 / (1 - alpha + 1e-10) with an
alpha uncertain by E_alpha adds |back| * (1 / (1 - min(1, alpha + U E_alpha) + 1e-10) - 1 / (1 - alpha + 1e-10)) / U, taken
over the whole interval rather than from the derivative, since alpha can round to exactly 1.0f.  A cell is then checked as
|gpu - ref| <= K * U * absref + FLOOR with K = K_FAMILY[family] (below): per family of values the smallest power of two that
is at least twice the larger of the worst ratios measured for the kernel on the MI355X and for the emulation on the CPU;
none exceeds 4 (the E terms are bounds, so most measured ratios are far below 1).

That the bound has teeth is shown without a GPU (tests/test_march_ref64_host.py): march_emu.Emu is a binary32 emulation of all
four variants of COUNT (plain, cached), FILL (plain, from the cache) and BWD (plain, dsdf_rec with accumulate 0 / 1, from the
cache), written from the kernel in its operation order; march_check.check_variant finds it inside every bound with every
flipped decision in its band on the GPU test's scenes, and rejects each of the 29 mutants of march_emu.MUTANTS (neighbours
across gaps and chunk seams, the 1e-5 guards, the float transmittance product, the early stop, the coarse second pass, the
"grad" taps, view directions and channels, the reverse scan's seed, guard, relu' and stopped sample, dsdf_rec, the cached
fill, the record slots and their order, overflow rays) in every family the table lists for it.  Two of the usual errors are not built,
each with its proof of equivalence in march_emu.py (the clamp of alpha at 1, and a folded out-of-range corner on the SDF
grid -- on the mask grid it is built); the `<=` stop is not built because no transmittance of a host scene reaches its value.

Stated limit: relu' = [pc > nc] is not a forced decision.  `near / den` in the backward's magnitudes is a first-order term
(it is multiplied by K U like the rest): it covers a backend whose pc - nc differs in VALUE, not one whose relu' differs.
Where prv == nxt bit for bit (a ray's only survivor, equal neighbours, ic == 0) restatement and kernel both see pc == nc
and agree on relu' = 0, and a backend with relu' = [pc >= nc] is rejected (mutant bwd_relu_ge, host scene `flat`).  Where
prv != nxt but the binary32 sigmoids tie -- e.g. a locally constant non-zero SDF whose fetched values differ by an ulp, under
the backward from the cache -- a correct binary32 backend takes relu' = 0 where float64 takes 1 and is rejected; the scenes
of both test files hold no such sample with a gradient that shows: kernel and emulation pass on all of them.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from types import SimpleNamespace
from typing import Optional

import numpy as np
import torch
import torch.nn.functional as F

import feat_ref64 as FR

F32, F64 = torch.float32, torch.float64
U = 2.0 ** -24
DEC_K = 16                       # decision bands: DEC_K * U * E around the threshold
T_STOP = float(torch.tensor(1e-3, dtype=F32))   # the kernel compares a binary32 T with 1e-3f
KEY = 1 << 20                    # key = ray * KEY + step


# K per family of march_check._bound: the smallest power of two that is at least twice the larger of the two measured worst
# ratios |got - ref| / (2^-24 absref) -- the kernel's on the MI355X over the three scenes of test_march_against_float64 and
# every cap of test_march_lds_regimes_and_refusal, and the emulation's (march_emu.Emu) over the seven host scenes of
# test_march_ref64_host.py.  Families that measure alike share a line (the line's worst sets its K).  absref's E terms are
# first-order BOUNDS, so most measured ratios are well below 1 and so is K.
#                                                                                    measured worst:   kernel    emulation
_K_GROUPS = [
    (1, ["fine count last", "fine_ga count last", "coarse count last", "coarse_ga count last"]),     # 0.325     0.365
    (0.5, ["coarse count cumw", "coarse_ga count cumw"]),                                            # 0.101     0.178
    (0.5, ["fine cache sdf", "fine fill sdf", "fine_ga fill sdf", "coarse fill sdf", "coarse_ga fill sdf"]),   # 0.246     0.212
    (1, ["fine cache alpha", "fine fill w", "fine_ga fill w", "coarse fill w", "coarse_ga fill w"]),  # 0.486     0.486
    (0.125, ["fine bwd", "coarse bwd"]),                                                             # 0.041     0.061
    (0.0625, ["fine_ga bwd", "coarse_ga bwd", "coarse_ga bwd grad_gg"]),                             # 0.018     0.022
    (0.25, ["fine bwd_rec"]),                                                                        # 0.058     0.070
    (1, ["fine bwd_cached"]),                            # (T and alpha binary32 inputs here: absref has no E of them)  0.397     0.405
    (2, ["fine bwd_rec dsdf_rec"]),                                                                  # 0.749     0.763
    (4, ["fine bwd_cached dsdf_rec"]),                                                               # 1.406     1.406
]
K_FAMILY = {f: k for k, fs in _K_GROUPS for f in fs}


@dataclass
class Scene:
    lo: torch.Tensor                 # xyz_min [3] float32
    hi: torch.Tensor
    mlo: torch.Tensor                # mask_min / mask_max
    mhi: torch.Tensor
    dims: tuple
    mdims: tuple
    near: float
    stepdist: float
    vox: float
    act_shift: float
    mask_thres: float
    fast_thres: float
    s_val: float
    max_steps: int

    @property
    def cap(self):
        return (self.max_steps + 63) // 64 * 64


def f32(v):
    """the binary32 value of a python float (scene constants are stored as binary32)"""
    return float(torch.tensor(v, dtype=F32))


@dataclass
class Inputs:
    rays_o: torch.Tensor             # [N,3] float32
    rays_d: torch.Tensor
    viewdirs: torch.Tensor           # [N,3] float32 ("grad" variants)
    mask: torch.Tensor               # [mx,my,mz] float32
    sdf: torch.Tensor                # [X,Y,Z] float32
    gg: Optional[torch.Tensor] = None    # [X,Y,Z,3] float32 (coarse "grad")


@dataclass
class Force:
    """The kernel's decisions, where it exposes them: mask-cache survivor keys (cached COUNT), per-survivor info words
    (cached COUNT: bit 0 alpha > thres, bit 1 visited), record keys (FILL)."""
    mask_keys: Optional[torch.Tensor] = None
    info: Optional[torch.Tensor] = None          # [n1 total] in survivor order
    rec_keys: Optional[torch.Tensor] = None


@dataclass
class Fwd:
    coarse: bool
    ga: bool
    N: int
    n_steps: torch.Tensor
    overflow: torch.Tensor
    n0: torch.Tensor
    n1: torch.Tensor
    n2: torch.Tensor
    n3: torch.Tensor
    last: torch.Tensor               # alphainv_last (float64 restatement) and its E
    last_E: torch.Tensor
    cumw: Optional[torch.Tensor]
    cumw_M: Optional[torch.Tensor]
    # survivors in (ray, step) order, padded per ray: [N, L]
    live: torch.Tensor
    step: torch.Tensor
    s: torch.Tensor
    s_E: torch.Tensor
    alpha: torch.Tensor
    alpha_E: torch.Tensor
    T: torch.Tensor
    T_E: torch.Tensor
    v2: torch.Tensor
    proc: torch.Tensor
    v3: torch.Tensor
    rank: torch.Tensor               # record rank within the ray (-1: none)
    w: torch.Tensor
    w_E: torch.Tensor
    ind: torch.Tensor                # [N, L, 3] binary32 grid index
    ic: Optional[torch.Tensor]
    ic_E: Optional[torch.Tensor]
    pc: torch.Tensor
    nc: torch.Tensor
    pc_E: torch.Tensor
    nc_E: torch.Tensor
    prv: torch.Tensor
    nxt: torch.Tensor
    flips: dict = field(default_factory=dict)
    census: dict = field(default_factory=dict)

    def records(self):
        """(ray, rank, step, w, w_E, sdf, sdf_E) of every record, in (ray, rank) order."""
        r, j = torch.nonzero(self.v3, as_tuple=True)
        return dict(ray=r, rank=self.rank[r, j], step=self.step[r, j], w=self.w[r, j], w_E=self.w_E[r, j],
                    sdf=self.s[r, j], sdf_E=self.s_E[r, j], j=j)


def _grid_ns(lo, hi, dims):
    return SimpleNamespace(lo=lo, hi=hi, dims=dims)


def _flip(name, fw, ref_dec, forced, dist, band):
    """Adopt the forced decision; every differing one must lie within its band (dist <= band)."""
    d = ref_dec != forced
    n = int(d.sum())
    if n:
        worst = float((dist[d] / band[d].clamp_min(1e-300)).max())
        assert worst <= 1.0, f"{name}: {n} kernel decisions off the boundary (worst |q - thres| / band = {worst:.3g})"
    fw.flips[name] = fw.flips.get(name, 0) + n
    return forced


def _pad(ray, vals, N, fill=0.0):
    """Samples in ray order -> [N, L] padded per ray (and the position of each sample)."""
    n = torch.bincount(ray, minlength=N)
    L = int(n.max()) if N and ray.numel() else 0
    first = torch.cumsum(n, 0) - n
    pos = torch.arange(ray.numel()) - first[ray]
    out = []
    for v in vals:
        shape = (N, max(L, 1)) + tuple(v.shape[1:])
        o = torch.full(shape, fill, dtype=v.dtype)
        o[ray, pos] = v
        out.append(o)
    return out, n, pos


def _chain64(alpha, todo):
    """The serial transmittance in float64 over the `todo` samples of each row: T before each sample, visited mask,
    T after the last visited sample, and T after each sample (for the stop band)."""
    om = torch.where(todo, 1.0 - alpha, torch.ones_like(alpha))
    after = torch.cumprod(om, 1)
    before = torch.cat([torch.ones_like(after[:, :1]), after[:, :-1]], 1)
    stop_here = todo & (after < T_STOP)
    first = torch.where(stop_here.any(1), stop_here.float().argmax(1), torch.full((alpha.shape[0],), alpha.shape[1]))
    pos = torch.arange(alpha.shape[1])[None]
    proc = todo & (pos <= first[:, None])
    last_pos = torch.where(proc.any(1), (proc * (pos + 1)).max(1).values - 1, torch.full_like(first, -1))
    Tlast = torch.where(last_pos >= 0, after.gather(1, last_pos.clamp_min(0)[:, None])[:, 0], torch.ones(alpha.shape[0], dtype=F64))
    return torch.where(proc, before, torch.ones_like(before)), proc, Tlast, after, last_pos


def chain32(alpha32, todo):
    """The kernel's serial transmittance replayed bit for bit from its binary32 alphas: T = float(double(T) * (1 - alpha)),
    stop once T < 1e-3f.  Returns T of each visited sample (1 elsewhere), the visited mask and the final T."""
    N, L = alpha32.shape
    T = torch.ones(N, dtype=F32)
    stopped = torch.zeros(N, dtype=torch.bool)
    mine = torch.ones(N, L, dtype=F32)
    proc = torch.zeros(N, L, dtype=torch.bool)
    thr = torch.tensor(T_STOP, dtype=F32)
    for j in range(L):
        act = todo[:, j] & ~stopped
        if not bool(act.any()):
            continue
        mine[:, j] = torch.where(act, T, mine[:, j])
        proc[:, j] = act
        T = torch.where(act, (T.double() * (1.0 - alpha32[:, j].double())).float(), T)
        stopped |= act & (T < thr)
    return mine, proc, T


def _alpha_terms(prv, nxt, prv_E, nxt_E, s_val):
    """NeuS alpha in float64 with the E bounds of pc, nc, alpha (module docstring)."""
    xp, xn = prv * s_val, nxt * s_val
    pc, nc = torch.sigmoid(xp), torch.sigmoid(xn)
    pc_E = pc * (1 - pc) * (s_val * prv_E + xp.abs()) + 4 * pc
    nc_E = nc * (1 - nc) * (s_val * nxt_E + xn.abs()) + 4 * nc
    num = F.relu(pc - nc) + 1e-5
    den = pc + 1e-5
    alpha = (num / den).clamp(0.0, 1.0)
    num_E = pc_E + nc_E + 2 * num
    den_E = pc_E + den
    alpha_E = (num_E + alpha * den_E) / den + alpha
    return pc, nc, pc_E, nc_E, alpha, alpha_E


def forward(sc: Scene, inp: Inputs, coarse: bool, ga: bool, force: Optional[Force] = None, alpha_in=None, s_in=None) -> Fwd:
    """march_kernel's COUNT / FILL restatement.  alpha_in / s_in ([n1 total] binary32, survivor order): the kernel's own
    cached values; the transmittance is then its bit-exact replay and the backward consumes them (interp variants)."""
    force = force or Force()
    N = inp.rays_o.shape[0]
    start, dirv, n_steps = FR.ray_geom(inp.rays_o, inp.rays_d, sc.lo, sc.hi, sc.near, sc.stepdist)
    overflow = n_steps > sc.cap
    ns = torch.where(overflow, torch.zeros_like(n_steps), n_steps)
    ray = torch.repeat_interleave(torch.arange(N), ns)
    first = torch.cumsum(ns, 0) - ns
    step = torch.arange(ray.numel()) - first[ray]
    p = FR.ray_point(start[ray], dirv[ray], sc.stepdist, step)
    inbox = ~(((sc.lo > p) | (sc.hi < p)).any(1))
    n0 = torch.bincount(ray[inbox], minlength=N)
    ray, step, p = ray[inbox], step[inbox], p[inbox]
    # mask cache
    mind = FR.world_to_index(_grid_ns(sc.mlo, sc.mhi, sc.mdims), p)
    dens, dens_abs = FR.fetch(inp.mask.double().reshape(-1), sc.mdims, mind)
    xarg = dens + sc.act_shift
    sp = F.softplus(xarg, beta=1, threshold=20)
    a = 1 - torch.exp(-sp)
    a_E = 1 + (1 - a) * (8 + 4 * sp + 16 * torch.sigmoid(xarg) * (dens_abs + abs(sc.act_shift)))
    keep = a >= sc.mask_thres
    fw_flips = {}
    tmp = SimpleNamespace(flips=fw_flips)
    if force.mask_keys is not None:
        k = ray * KEY + step
        kern = torch.isin(k, force.mask_keys)
        assert int(kern.sum()) == force.mask_keys.numel(), "kernel mask-cache survivors outside the in-box samples"
        keep = _flip("mask", tmp, keep, kern, (a - sc.mask_thres).abs(), DEC_K * U * a_E)
    ray, step, p = ray[keep], step[keep], p[keep]
    ind = FR.world_to_index(_grid_ns(sc.lo, sc.hi, sc.dims), p)
    s64, s_abs = FR.fetch(inp.sdf.double().reshape(-1), sc.dims, ind)
    s_E = 16 * s_abs
    if s_in is not None:
        s64, s_E = s_in.double(), torch.zeros_like(s64)
    ic = ic_E = None
    if ga:
        vd = inp.viewdirs[ray].double()
        if coarse:
            gv, gabs = FR.fetch(inp.gg.double().reshape(-1, 3), sc.dims, ind, ch=3)
            icE_k = 16
        else:
            g64 = inp.sdf.double().reshape(-1)
            gv, gabs = torch.zeros(ind.shape[0], 3, dtype=F64), torch.zeros(ind.shape[0], 3, dtype=F64)
            case = _grid_ns(sc.lo, sc.hi, sc.dims)
            for ax in range(3):
                ixp, apx = FR.tap_index(case, ind, ax, 1.0)
                ixm, amx = FR.tap_index(case, ind, ax, -1.0)
                fp_, ap_ = FR.fetch(g64, sc.dims, ixp)
                fm_, am_ = FR.fetch(g64, sc.dims, ixm)
                den = (apx - amx).double() * sc.vox
                gv[:, ax], gabs[:, ax] = (fp_ - fm_) / den, (ap_ + am_) / den
            icE_k = 32
        ic = (vd * gv).sum(1) * sc.stepdist * 0.5
        ic_E = icE_k * (vd.abs() * gabs).sum(1) * sc.stepdist * 0.5
    vals = [ray * 0 + step, s64, s_E, ind]
    if ic is not None:
        vals += [ic, ic_E]
    if alpha_in is not None:
        vals.append(alpha_in.float())
    padded, n1, pos = _pad(ray, vals, N)
    stp, S, SE, IND = padded[:4]
    IC, ICE = (padded[4], padded[5]) if ic is not None else (None, None)
    A32 = padded[-1] if alpha_in is not None else None
    L = S.shape[1]
    P = torch.arange(L)[None]
    live = P < n1[:, None]
    if ga:
        prv, nxt = S - IC, S + IC
        prv_E = SE + ICE + prv.abs()
        nxt_E = SE + ICE + nxt.abs()
    else:
        Sm = torch.cat([S[:, :1], S[:, :-1]], 1)
        Sp = torch.cat([S[:, 1:], S[:, -1:]], 1)
        SEm = torch.cat([SE[:, :1], SE[:, :-1]], 1)
        SEp = torch.cat([SE[:, 1:], SE[:, -1:]], 1)
        hasp, hasn = P > 0, P < n1[:, None] - 1
        prv = torch.where(hasp, (Sm + S) * 0.5, S)
        nxt = torch.where(hasn, (S + Sp) * 0.5, S)
        prv_E = torch.where(hasp, 0.5 * (SEm + SE) + prv.abs(), SE)
        nxt_E = torch.where(hasn, 0.5 * (SE + SEp) + nxt.abs(), SE)
    pc, nc, pc_E, nc_E, alpha, alpha_E = _alpha_terms(prv, nxt, prv_E, nxt_E, sc.s_val)
    if A32 is not None:                                   # the kernel's alphas: check, then adopt
        alpha_k = A32.double()
    v2 = live & (True if coarse else (alpha > sc.fast_thres))
    if force.info is not None:
        INFO = _pad(ray, [force.info.long()], N)[0][0]
        v2 = _flip("alpha>thres", tmp, v2, live & ((INFO & 1) == 1), (alpha - sc.fast_thres).abs(), DEC_K * U * alpha_E)
    # transmittance (first pass)
    if A32 is not None:
        T, proc, Tl32 = chain32(A32, v2)
        T = T.double()
        T_E = torch.zeros_like(T)
        Tlast, Tlast_E = Tl32.double(), torch.zeros(N, dtype=F64)
        achain = alpha_k
        achain_E = (1 - achain).abs()
    else:
        T, proc, Tlast, after, last_pos = _chain64(alpha, v2)
        rel = torch.where(proc, alpha_E / (1 - alpha).clamp_min(1e-300) + 2, torch.zeros_like(alpha))
        relc = torch.cumsum(rel, 1)
        T_E = T * (relc - rel)
        Tlast_E = Tlast * relc[:, -1]
        if force.info is not None:
            kproc = live & ((INFO & 2) == 2)
            band = DEC_K * U * after * relc
            proc = _flip("early stop", tmp, proc, kproc, (after - T_STOP).abs(), band.clamp_min(0)) if bool((proc != kproc).any()) else proc
        achain, achain_E = alpha, alpha_E
    w = torch.where(proc, T * achain, torch.zeros_like(T))
    w_E = torch.where(proc, T_E * achain + T * achain_E + w, torch.zeros_like(T))
    v3 = proc & (w > sc.fast_thres)
    if force.rec_keys is not None:
        kk = torch.where(live, torch.arange(N)[:, None] * KEY + stp, -1)
        kv3 = live & torch.isin(kk, force.rec_keys)
        v3 = _flip("w>thres", tmp, v3, kv3, (w - sc.fast_thres).abs(), DEC_K * U * w_E)
    n2 = v2.sum(1)
    cumw = cumw_M = None
    if coarse:                                            # second pass over the survivors
        if A32 is not None:
            T, proc, Tl32 = chain32(A32, v3)
            T, T_E = T.double(), torch.zeros(N, L, dtype=F64)
            Tlast, Tlast_E = Tl32.double(), torch.zeros(N, dtype=F64)
        else:
            T, proc, Tlast, after, _ = _chain64(alpha, v3)
            rel = torch.where(proc, alpha_E / (1 - alpha).clamp_min(1e-300) + 2, torch.zeros_like(alpha))
            relc = torch.cumsum(rel, 1)
            T_E = T * (relc - rel)
            Tlast_E = Tlast * relc[:, -1]
        w = torch.where(proc, T * achain, torch.zeros_like(T))
        w_E = torch.where(proc, T_E * achain + T * achain_E + w, torch.zeros_like(T))
        cumw = torch.where(v3, w, torch.zeros_like(w)).sum(1)
        cumw_M = torch.where(v3, w_E + w * 8, torch.zeros_like(w)).sum(1)
    rank = torch.where(v3, torch.cumsum(v3.long(), 1) - 1, torch.full_like(stp, -1))
    fw = Fwd(coarse=coarse, ga=ga, N=N, n_steps=n_steps, overflow=overflow, n0=n0, n1=n1, n2=n2, n3=v3.sum(1),
             last=Tlast, last_E=Tlast_E, cumw=cumw, cumw_M=cumw_M, live=live, step=stp, s=S, s_E=SE,
             alpha=achain, alpha_E=achain_E, T=T, T_E=T_E, v2=v2, proc=proc, v3=v3, rank=rank, w=w, w_E=w_E, ind=IND,
             ic=IC, ic_E=ICE, pc=pc, nc=nc, pc_E=pc_E, nc_E=nc_E, prv=prv, nxt=nxt, flips=fw_flips)
    fw.alpha64, fw.alpha64_E = alpha, alpha_E
    return fw


# ---- backward ---------------------------------------------------------------------------------------------------------
@dataclass
class Bwd:
    grad_sdf: dict                   # flat cell -> (value, absref) as three tensors (cells, value, absref)
    grad_gg: Optional[tuple]         # (flat index into [X,Y,Z,3], value, absref)
    dsdf: Optional[tuple]            # (record (ray, rank) pairs [R,2], value, absref)
    rec_only_cells: torch.Tensor     # cells touched only by recorded samples' value taps (dsdf_rec mode)


def _cells(ind, vals, mags, dims):
    """Trilinear scatter terms of per-sample values at binary32 indices [M,3]: flat cells [M,8], values, magnitudes."""
    cells, w = FR._corners(ind)
    ok = FR._inb(cells, dims) & (w != 0)
    fl = torch.where(ok, FR._flat(cells, dims), -1)
    return fl, vals[:, None] * w, mags[:, None] * w


def _sum_cells(fl, v, m):
    fl, v, m = fl.reshape(-1), v.reshape(-1), m.reshape(-1)
    keep = fl >= 0
    fl, v, m = fl[keep], v[keep], m[keep]
    u, inv = torch.unique(fl, return_inverse=True)
    return (u, torch.zeros(u.numel(), dtype=F64).index_add_(0, inv, v),
            torch.zeros(u.numel(), dtype=F64).index_add_(0, inv, m))


def backward(sc: Scene, inp: Inputs, fw: Fwd, gw, dlast, rec_mode: bool = False, eps: float = 1e-10) -> Bwd:
    """march_kernel's BWD restatement.  gw [N, L]: dweight of each record (0 elsewhere), dlast [N] float32.  eps: the guard
    of 1 / (1 - alpha + eps) (the kernel's 1e-10; 0 gives the exact derivative)."""
    N, L = fw.s.shape
    proc = fw.proc
    T, T_E, al, al_E = fw.T, fw.T_E, fw.alpha, fw.alpha_E
    gw = torch.where(fw.v3, gw.double(), torch.zeros_like(T))
    dl = dlast.double()
    x = torch.where(proc, gw * T * al, torch.zeros_like(T))
    xM = torch.where(proc, gw.abs() * (T * al + T_E * al + T * al_E), torch.zeros_like(T))
    suf = lambda v: v.flip(1).cumsum(1).flip(1)
    back = dl[:, None] * fw.last[:, None] + suf(x) - x
    nchunk = (fw.n1 + 63) // 64
    backM = (dl.abs() * (fw.last + fw.last_E))[:, None] + suf(xM) - xM
    backM = backM * (8 + nchunk.double())[:, None]
    inv = 1.0 / (1.0 - al + eps)
    inv_hi = 1.0 / (1.0 - (al + U * al_E).clamp(max=1.0) + eps)
    S_E = (inv_hi - inv) / U
    dalpha = torch.where(proc, gw * T - back * inv, torch.zeros_like(T))
    dalM = torch.where(proc, gw.abs() * (T + T_E) + backM * inv + back.abs() * S_E, torch.zeros_like(T))
    pc, nc, pc_E, nc_E = fw.pc, fw.nc, fw.pc_E, fw.nc_E
    num, den = F.relu(pc - nc) + 1e-5, pc + 1e-5
    pos = (pc - nc > 0).double()
    near = (pc - nc).abs() <= DEC_K * U * (pc_E + nc_E)
    fw.census["relu_kink"] = int((near & proc).sum())
    num_E, den_E = pc_E + nc_E + 2 * num, pc_E + den
    drp = (pos * den - num) / den ** 2
    drn = -pos / den
    drpM = (pos * den + num + num_E + den_E) / den ** 2 + 2 * (pos * den - num).abs() * den_E / den ** 3 + near / den
    drnM = pos / den + pos * den_E / den ** 2 + near / den
    s = sc.s_val
    spp, spn = s * pc * (1 - pc), s * nc * (1 - nc)
    sppM = s * (3 * pc * (1 - pc) + pc + pc_E * (1 - 2 * pc).abs())
    spnM = s * (3 * nc * (1 - nc) + nc + nc_E * (1 - 2 * nc).abs())
    z = torch.zeros_like(T)
    dprev = torch.where(proc, dalpha * drp * spp, z)
    dnext = torch.where(proc, dalpha * drn * spn, z)
    dprevM = torch.where(proc, dalM * drpM * sppM, z)
    dnextM = torch.where(proc, dalM * drnM * spnM, z)
    live = fw.live
    sel = lambda t: t[live]
    gg = None
    rec_only = torch.zeros(0, dtype=torch.long)
    dsdf = None
    if fw.ga:
        ds, dsM = dprev + dnext, dprevM + dnextM
        dic, dicM = dnext - dprev, dprevM + dnextM
        ind = fw.ind[live]
        fl, v, m = _cells(ind, sel(ds), sel(dsM), sc.dims)
        fls, vs, ms = [fl], [v], [m]
        vd = inp.viewdirs[torch.nonzero(live)[:, 0]].double()
        if fw.coarse:
            k, kM = sel(dic) * 0.5 * sc.stepdist, sel(dicM) * 0.5 * sc.stepdist
            cells, wt = FR._corners(ind)
            ok = FR._inb(cells, sc.dims) & (wt != 0)
            base = FR._flat(cells, sc.dims) * 3
            gfl, gv, gm = [], [], []
            for a in range(3):
                nz = ok & (vd[:, a] != 0)[:, None]
                gfl.append(torch.where(nz, base + a, -1))
                gv.append(k[:, None] * vd[:, a:a + 1] * wt)
                gm.append(kM[:, None] * vd[:, a:a + 1].abs() * wt)
            gg = _sum_cells(torch.cat(gfl, 1), torch.cat(gv, 1), torch.cat(gm, 1))
        else:
            case = _grid_ns(sc.lo, sc.hi, sc.dims)
            for a in range(3):
                ixp, apx = FR.tap_index(case, ind, a, 1.0)
                ixm, amx = FR.tap_index(case, ind, a, -1.0)
                c = sel(dic) * 0.5 * sc.stepdist * vd[:, a] / (apx - amx).double() / sc.vox
                cM = sel(dicM) * 0.5 * sc.stepdist * vd[:, a].abs() / (apx - amx).double() / sc.vox
                for ix, sg in ((ixp, 1.0), (ixm, -1.0)):
                    f_, v_, m_ = _cells(ix, sg * c, cM, sc.dims)
                    fls.append(f_); vs.append(v_); ms.append(m_)
        g = _sum_cells(torch.cat(fls, 1), torch.cat(vs, 1), torch.cat(ms, 1))
        return Bwd(grad_sdf=g, grad_gg=gg, dsdf=None, rec_only_cells=rec_only)
    P = torch.arange(L)[None]
    hasp, hasn = P > 0, P < fw.n1[:, None] - 1
    shl = lambda t: torch.cat([t[:, 1:], torch.zeros_like(t[:, :1])], 1)        # t[j + 1]
    shr = lambda t: torch.cat([torch.zeros_like(t[:, :1]), t[:, :-1]], 1)       # t[j - 1]
    ds = dprev * torch.where(hasp, 0.5, 1.0) + dnext * torch.where(hasn, 0.5, 1.0) + \
        torch.where(hasn, 0.5 * shl(dprev), z) + torch.where(hasp, 0.5 * shr(dnext), z)
    dsM = dprevM + dnextM + torch.where(hasn, 0.5 * shl(dprevM), z) + torch.where(hasp, 0.5 * shr(dnextM), z)
    scat = live & ~(fw.v3 if rec_mode else torch.zeros_like(live))
    fl, v, m = _cells(fw.ind[scat], ds[scat], dsM[scat], sc.dims)
    g = _sum_cells(fl, v, m)
    if rec_mode:
        r, j = torch.nonzero(fw.v3, as_tuple=True)
        dsdf = (torch.stack([r, fw.rank[r, j]], 1), ds[r, j], dsM[r, j])
        flr, _, mr = _cells(fw.ind[fw.v3], ds[fw.v3], dsM[fw.v3], sc.dims)
        ur = torch.unique(flr[(flr >= 0) & (mr != 0)])
        rec_only = ur[~torch.isin(ur, g[0])]
    return Bwd(grad_sdf=g, grad_gg=None, dsdf=dsdf, rec_only_cells=rec_only)


# ---- plan -------------------------------------------------------------------------------------------------------------
def plan(cnt3, em_modes, stats):
    """esr_fine_plan in numpy: (off3 [n], header [n_on, n_off, tiles_on, tiles_all, m0, m1, m2]).  On rays (em_modes == 1)
    first in ray order, off rays from the next multiple of 32."""
    cnt3 = np.asarray(cnt3, dtype=np.int64)
    on = np.asarray(em_modes) == 1
    off3 = np.zeros(cnt3.shape[0], dtype=np.int64)
    c_on, c_off = np.where(on, cnt3, 0), np.where(on, 0, cnt3)
    n_on, n_off = int(c_on.sum()), int(c_off.sum())
    base = (n_on + 31) // 32 * 32
    off3 = np.where(on, np.cumsum(c_on) - c_on, base + np.cumsum(c_off) - c_off)
    st = np.asarray(stats, dtype=np.int64).reshape(-1, 3)
    tiles_on = (n_on + 31) // 32
    return off3, [n_on, n_off, tiles_on, tiles_on + (n_off + 31) // 32, *[int(v) for v in st.sum(0)]]


# ---- scenes -----------------------------------------------------------------------------------------------------------
def box_scene(dims, vox=1.0 / 32, s_val=40.0, fast_thres=1e-4, mask_thres=1e-3, max_steps=None, mdims=None):
    """A box centred on 0 with `dims` grid points (voxel `vox`), the mask grid over the same box."""
    half = torch.tensor([(d - 1) * vox / 2 for d in dims], dtype=F32)
    lo, hi = -half, half
    if max_steps is None:
        diag = float(((hi - lo).double() ** 2).sum().sqrt())
        max_steps = int(diag / f32(0.5 * vox)) + 4
    return Scene(lo=lo, hi=hi, mlo=lo.clone(), mhi=hi.clone(), dims=tuple(dims), mdims=tuple(mdims or dims), near=0.0,
                 stepdist=f32(0.5 * vox), vox=f32(vox), act_shift=0.0, mask_thres=f32(mask_thres), fast_thres=f32(fast_thres),
                 s_val=f32(s_val), max_steps=int(max_steps))
