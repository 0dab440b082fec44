"""Binary32 emulation of csrc/march.hip's march_kernel on the CPU (all four (COARSE, GA) variants; COUNT plain and cached,
FILL plain and from the cache, BWD plain / dsdf_rec / from the cache) with the methods of the GPU test's `Run`, and the
mutants of it that march_check.check_variant has to reject (tests/test_march_ref64_host.py).  Written from the kernel in its
operation order; it shares with the restatement march_ref64.py only what that replays bit for bit in binary32 (feat_ref64's
ray geometry, sample positions, continuous indices and clamped tap indices).  Everything from the trilinear fetch onwards is
this file's: torch binary32 elementwise operations (each rounded once), the fetch's fma as a float64 product-sum rounded to
binary32, the serial transmittance as float(double(T) * (1.0 - alpha)), float32 index_add_ for the atomics (the kernel's
order is not defined).  torch's expf / log1pf differ from the device's by an ulp here and there, so decisions differ from the
restatement's as the kernel's do; the checker's Force and bands take them."""
from types import SimpleNamespace

import numpy as np
import torch

import feat_ref64 as FR
import march_ref64 as R

F32, F64 = torch.float32, torch.float64

# name -> the families of march_check.Check.fails it must show up in (on at least one small scene each).
#   "... exact": a count, step, info word, ray id or bit-exact value.
#   "<variant> decisions": any AssertionError of march_ref64.forward under the backend's forced decisions -- a decision off
#   its band, or mask-cache survivors that are no in-box samples at all (not a band check).  A mutant listed ONLY for such
#   families (end_rule_swapped, eps_den_only, stop_before_multiply, ga_viewdir_wrong_ray, ga_half_dist_one_side,
#   coarse_gg_permuted, corner_folded_mask, rec_at_survivor_index, overflow_keeps_counts) shows that Force and DEC_K have
#   teeth; it says nothing about K_FAMILY, whose teeth are the value families of the other rows.
# Not in the table, with the reason:
#   * "neus_alpha is not clamped at 1": equivalent on every admissible input.  nc = 1 / (1 + expf(-x)) >= 0, so by the
#     monotonicity of rounding fl(max(pc - nc, 0)) <= pc, fl(. + 1e-5f) <= fl(pc + 1e-5f), and a correctly rounded quotient of
#     num <= den is <= 1; num >= 1e-5f > 0 keeps it above 0.  The clamp never acts.
#   * "the stop uses <= against the double 1e-3 rounded down": differs from `T < 1e-3f` only for a T equal to that one
#     binary32 value, which no transmittance of any host scene and variant reaches (asserted by
#     test_no_transmittance_on_the_value_below_the_stop), so it cannot be told from the kernel's test there.
#   * "an out-of-range corner folded back", on the SDF and gradient grids: an in-box sample has 0 <= idx <= dims - 1, taps
#     are clamped there, so an out-of-range corner has weight exactly 0 in the fetch (0 * finite) and is skipped by the
#     scatter's w != 0.  It is live on the mask grid when the mask box is smaller than the scene box: scene "mbox".
MUTANTS = {
    "nbr_adjacent_step": ["fine decisions", "coarse decisions", "fine bwd_rec", "fine bwd_cached"],
    "seam_carry_lost": ["fine decisions", "coarse decisions", "fine cache alpha", "fine count last", "fine fill w", "coarse fill w"],
    "end_rule_swapped": ["fine decisions", "coarse decisions"],
    "eps_num_only": ["fine decisions", "fine_ga decisions", "coarse decisions", "coarse_ga decisions", "fine cache alpha", "coarse fill w"],
    "eps_den_only": ["fine decisions", "fine_ga decisions", "coarse decisions", "coarse_ga decisions"],
    "T_float_product": ["fine cache exact"],
    "stop_before_multiply": ["fine decisions", "fine_ga decisions", "coarse decisions", "coarse_ga decisions"],
    "coarse_first_pass": ["coarse count last", "coarse fill w", "coarse bwd", "coarse_ga count last"],
    "coarse_cumw_first_pass": ["coarse count cumw", "coarse_ga count cumw"],
    "coarse_alpha_thres": ["coarse count exact", "coarse_ga count exact"],
    "ga_div_2": ["fine_ga decisions", "fine_ga count last", "fine_ga fill w", "fine_ga bwd"],
    "ga_div_2_bwd": ["fine_ga bwd"],
    "ga_viewdir_wrong_ray": ["fine_ga decisions", "coarse_ga decisions"],
    "ga_viewdir_wrong_ray_bwd": ["fine_ga bwd", "coarse_ga bwd grad_gg"],
    "ga_half_dist_one_side": ["fine_ga decisions", "coarse_ga decisions"],
    "coarse_gg_permuted": ["coarse_ga decisions"],
    "coarse_gg_permuted_bwd": ["coarse_ga bwd grad_gg"],
    "corner_folded_mask": ["fine decisions", "fine_ga decisions", "coarse decisions", "coarse_ga decisions"],
    "bwd_no_dlast": ["fine bwd", "fine_ga bwd", "coarse bwd", "coarse_ga bwd", "fine bwd_rec", "fine bwd_cached"],
    "bwd_no_eps": ["fine bwd", "fine_ga bwd", "coarse bwd", "coarse_ga bwd", "fine bwd_rec", "fine bwd_cached"],
    "bwd_relu_ge": ["fine bwd", "fine_ga bwd", "coarse bwd", "coarse_ga bwd grad_gg", "fine bwd_rec dsdf_rec",
                    "fine bwd_cached dsdf_rec"],         # (exact ties prv == nxt with neighbours: scene "flat")
    "bwd_stop_term_dropped": ["fine bwd", "fine_ga bwd", "coarse bwd", "coarse_ga bwd", "fine bwd_rec", "fine bwd_cached"],
    "rec_overwrite_acc": ["fine bwd_rec dsdf_rec", "fine bwd_cached dsdf_rec"],
    "rec_scatters_recorded": ["fine bwd_rec", "fine bwd_cached"],
    "rec_unrecorded_slot_written": ["fine bwd_rec dsdf_rec", "fine bwd_cached dsdf_rec"],
    "fill_cached_w_from_alpha64": ["fine fill_cached exact"],
    "rec_at_survivor_index": ["fine decisions", "fine_ga decisions", "coarse decisions", "coarse_ga decisions"],
    "rec_reversed_in_ray": ["fine fill exact", "fine_ga fill exact", "coarse fill exact", "coarse_ga fill exact"],
    "overflow_keeps_counts": ["fine decisions", "fine_ga decisions", "coarse decisions", "coarse_ga decisions"],
}


def _f(v):
    return torch.tensor(v, dtype=F32)


def _tri(ind, dims, fold=False):
    """esr_tri_setup + esr_corner_w in binary32: cells [M,8,3], weights (wz * wy) * wx [M,8], in-grid flags [M,8]."""
    fl = torch.floor(ind)
    i0 = fl.long()
    lo_w, hi_w = (fl + 1.0) - ind, ind - fl                 # (x1 - ix), (ix - x0)
    cells, ws = [], []
    for cx in (0, 1):
        for cy in (0, 1):
            for cz in (0, 1):
                cells.append(torch.stack([i0[:, 0] + cx, i0[:, 1] + cy, i0[:, 2] + cz], -1))
                wx, wy, wz = [(hi_w if c else lo_w)[:, a] for a, c in enumerate((cx, cy, cz))]
                ws.append((wz * wy) * wx)
    cells, w = torch.stack(cells, 1), torch.stack(ws, 1)
    top = torch.tensor(dims) - 1
    if fold:                                                # mutant: an out-of-range corner folded onto the last node
        cells = torch.minimum(cells.clamp_min(0), top)
    inb = ((cells >= 0) & (cells <= top)).all(-1)
    return cells, w, inb


def _flat(cells, dims):
    return (cells[..., 0] * dims[1] + cells[..., 1]) * dims[2] + cells[..., 2]


def _fetch1(grid, dims, ind, fold=False):
    """esr_tri_fetch1: acc = fmaf(g or 0, w, acc) over the 8 corners in (cx, cy, cz) order."""
    cells, w, inb = _tri(ind, dims, fold)
    fl = torch.where(inb, _flat(cells, dims), torch.zeros_like(inb, dtype=torch.long))
    acc = torch.zeros(ind.shape[0], dtype=F32)
    for c in range(8):
        g = torch.where(inb[:, c], grid[fl[:, c]], torch.zeros((), dtype=F32))
        acc = (g.double() * w[:, c].double() + acc.double()).float()
    return acc


def _fetch3(gg, dims, ind):
    """coarse_alpha_ic's 3-channel fetch: gv[c] += q[c] * w, product and sum rounded separately (contraction off)."""
    cells, w, inb = _tri(ind, dims)
    fl = torch.where(inb, _flat(cells, dims), torch.zeros_like(inb, dtype=torch.long))
    gv = torch.zeros(ind.shape[0], 3, dtype=F32)
    for c in range(8):
        q = torch.where(inb[:, c, None], gg[fl[:, c]], torch.zeros((), dtype=F32))
        gv = gv + q * w[:, c, None]
    return gv


def _sigmoid(x):
    return 1.0 / (1.0 + torch.exp(-x))


def _pad(ray, pos, N, L, v, fill=0):
    o = torch.full((N, L) + tuple(v.shape[1:]), fill, dtype=v.dtype)
    o[ray, pos] = v
    return o


class Emu:
    def __init__(self, sc, inp, coarse, ga, mut=None):
        assert mut is None or mut in MUTANTS, mut
        self.sc, self.inp, self.coarse, self.ga, self.mut = sc, inp, coarse, ga, mut
        self.n = inp.rays_o.shape[0]
        self.grid = SimpleNamespace(lo=sc.lo, hi=sc.hi, dims=sc.dims)
        self._walked = self._p2 = None

    # ---- phase 1: the walk ----------------------------------------------------------------------------------------
    def _vd(self, ray, bwd=False):
        wrong = self.mut == ("ga_viewdir_wrong_ray_bwd" if bwd else "ga_viewdir_wrong_ray")
        return self.inp.viewdirs[(ray + 1) % self.n if wrong else ray]

    def _taps(self, ind, bwd=False):
        """per axis: the two clamped tap indices and the divisor ap - am"""
        out = []
        for a in range(3):
            ixp, ap = FR.tap_index(self.grid, ind, a, 1.0)
            ixm, am = FR.tap_index(self.grid, ind, a, -1.0)
            den = ap - am
            if self.mut == ("ga_div_2_bwd" if bwd else "ga_div_2"):
                den = torch.full_like(den, 2.0)
            out.append((ixp, ixm, den))
        return out

    def walk(self):
        if self._walked is not None:
            return self._walked
        sc, inp, N = self.sc, self.inp, self.n
        start, dirv, n_steps = FR.ray_geom(inp.rays_o, inp.rays_d, sc.lo, sc.hi, sc.near, sc.stepdist)
        overflow = n_steps > sc.cap
        ns = n_steps if self.mut == "overflow_keeps_counts" else torch.where(overflow, torch.zeros_like(n_steps), n_steps)
        ray = torch.repeat_interleave(torch.arange(N), ns)
        step = torch.arange(ray.numel()) - (torch.cumsum(ns, 0) - ns)[ray]
        p = FR.ray_point(start[ray], dirv[ray], sc.stepdist, step)
        ok = ~(((sc.lo > p) | (sc.hi < p)).any(1))
        n0 = torch.bincount(ray[ok], minlength=N)
        ray, step, p = ray[ok], step[ok], p[ok]
        midx = FR.world_to_index(SimpleNamespace(lo=sc.mlo, hi=sc.mhi, dims=sc.mdims), p)
        dens = _fetch1(inp.mask.reshape(-1), sc.mdims, midx, fold=self.mut == "corner_folded_mask")
        x = dens + _f(sc.act_shift)
        sp = torch.where(x > 20.0, x, torch.log1p(torch.exp(x)))
        a = 1.0 - torch.exp(-sp)
        ok = a >= _f(sc.mask_thres)
        ray, step, p = ray[ok], step[ok], p[ok]
        ind = FR.world_to_index(self.grid, p)
        sdf = inp.sdf.reshape(-1)
        s = _fetch1(sdf, sc.dims, ind)
        ic = None
        if self.ga:
            vd = self._vd(ray)
            dist = _f(sc.stepdist)
            if self.coarse:
                gv = _fetch3(inp.gg.reshape(-1, 3), sc.dims, ind)
                if self.mut == "coarse_gg_permuted":
                    gv = gv[:, [1, 2, 0]]
            else:
                gv = torch.stack([((_fetch1(sdf, sc.dims, ixp) - _fetch1(sdf, sc.dims, ixm)) / den) / _f(sc.vox)
                                  for ixp, ixm, den in self._taps(ind)], 1)
            dotp = (vd[:, 0] * gv[:, 0] + vd[:, 1] * gv[:, 1]) + vd[:, 2] * gv[:, 2]
            ic = (dotp * dist) * 0.5
        n1 = torch.bincount(ray, minlength=N)
        L = max(int(n1.max()) if N else 0, 1)
        pos = torch.arange(ray.numel()) - (torch.cumsum(n1, 0) - n1)[ray]
        w = SimpleNamespace(overflow=overflow, n0=n0, n1=n1, L=L,
                            S=_pad(ray, pos, N, L, s), STEP=_pad(ray, pos, N, L, step), IND=_pad(ray, pos, N, L, ind),
                            IC=_pad(ray, pos, N, L, ic) if ic is not None else None)
        self._walked = w
        return w

    # ---- phase 2: alpha, thresholds, transmittance ----------------------------------------------------------------
    def _sections(self, S, IC, STEP, n1):
        """prv / nxt: the SDF at the two ends of a sample's section"""
        L = S.shape[1]
        P = torch.arange(L)[None]
        if self.ga:
            if self.mut == "ga_half_dist_one_side":
                return S - IC, S + (IC + IC)
            return S - IC, S + IC
        hasp, hasn = P > 0, P < n1[:, None] - 1
        Sm = torch.cat([S[:, :1], S[:, :-1]], 1)
        Sp = torch.where(hasn, torch.cat([S[:, 1:], S[:, -1:]], 1), S)
        if self.mut == "nbr_adjacent_step":                 # the lane of step +- 1: holds 0 when that step is no survivor
            Tm = torch.cat([STEP[:, :1], STEP[:, :-1]], 1)
            Tp = torch.cat([STEP[:, 1:], STEP[:, -1:]], 1)
            Sm = torch.where(STEP - Tm == 1, Sm, torch.zeros_like(S))
            Sp = torch.where(Tp - STEP == 1, Sp, torch.zeros_like(S))
        if self.mut == "seam_carry_lost":
            hasp, hasn = hasp & (P % 64 != 0), hasn & (P % 64 != 63)
        if self.mut == "end_rule_swapped":
            hasp, hasn = hasn, hasp
        return torch.where(hasp, (Sm + S) * 0.5, S), torch.where(hasn, (S + Sp) * 0.5, S)

    def _numden(self, pc, nc):
        e = _f(1e-5)
        num, den = torch.clamp_min(pc - nc, 0.0) + e, pc + e
        if self.mut == "eps_num_only":
            den = pc
        if self.mut == "eps_den_only":
            num = torch.clamp_min(pc - nc, 0.0)
        return num, den

    def _alpha(self, S, IC, STEP, n1):
        prv, nxt = self._sections(S, IC, STEP, n1)
        sv = _f(self.sc.s_val) if S.dtype == F32 else self.sc.s_val
        pc, nc = _sigmoid(prv * sv), _sigmoid(nxt * sv)
        num, den = self._numden(pc, nc)
        return torch.clamp(num / den, 0.0, 1.0), pc, nc

    def _chain(self, alpha, todo):
        """serial_transmittance over the `todo` samples in order: T of each visited sample, visited, final T"""
        N, L = alpha.shape
        T = torch.ones(N, dtype=F32)
        stopped = torch.zeros(N, dtype=torch.bool)
        mine, proc = torch.ones(N, L, dtype=F32), torch.zeros(N, L, dtype=torch.bool)
        thr = _f(1e-3)
        for j in range(L):
            act = todo[:, j] & ~stopped
            if not bool(act.any()):
                continue
            if self.mut == "T_float_product":
                Tn = T * (1.0 - alpha[:, j])
            else:
                Tn = (T.double() * (1.0 - alpha[:, j].double())).float()
            stop = act & (Tn < thr)
            vis = act & ~stop if self.mut == "stop_before_multiply" else act
            mine[:, j] = torch.where(vis, T, mine[:, j])
            proc[:, j] = vis
            T = torch.where(act, Tn, T)
            stopped |= stop
        return mine, proc, T

    def phase2(self):
        if self._p2 is not None:
            return self._p2
        w, ft = self.walk(), _f(self.sc.fast_thres)
        live = torch.arange(w.L)[None] < w.n1[:, None]
        alpha, _, _ = self._alpha(w.S, w.IC, w.STEP, w.n1)
        alpha = torch.where(live, alpha, torch.zeros_like(alpha))
        thres = (not self.coarse) or self.mut == "coarse_alpha_thres"
        v2 = live & ((alpha > ft) if thres else True)
        T, proc, tc = self._chain(alpha, v2)
        wt = torch.where(proc, T * alpha, torch.zeros_like(T))
        v3 = proc & (wt > ft)
        rank = torch.cumsum(v3.long(), 1) - 1
        cumw = None
        if self.coarse:
            first = wt
            if self.mut != "coarse_first_pass":
                T, proc, tc = self._chain(alpha, v3)
                wt = torch.where(proc, T * alpha, torch.zeros_like(T))
            cumw = torch.where(v3, first if self.mut == "coarse_cumw_first_pass" else wt, torch.zeros_like(wt)).sum(1)
        info = v2.int() | (proc.int() << 1) | torch.where(v3, (rank.int() + 1) << 8, torch.zeros_like(rank, dtype=torch.int32))
        self._p2 = SimpleNamespace(live=live, alpha=alpha, T=T, info=info, v3=v3, rank=rank, w=wt, last=tc, cumw=cumw,
                                   n2=v2.sum(1), n3=v3.sum(1))
        return self._p2

    # ---- the entry points ---------------------------------------------------------------------------------------------
    def count(self, cached=False):
        w, q, n, cap = self.walk(), self.phase2(), self.n, self.sc.cap
        zero = w.overflow & (self.mut != "overflow_keeps_counts")
        z = lambda t: torch.where(zero, torch.zeros_like(t), t).int()
        out = dict(cnt3=z(q.n3), stats=torch.stack([z(w.n0), z(w.n1), z(q.n2)], 1).reshape(-1).contiguous(),
                   last=torch.where(w.overflow, torch.ones_like(q.last), q.last),
                   cumw=torch.where(w.overflow, _f(-7.0), q.cumw) if self.coarse else torch.full((n,), -7.0),
                   plan=torch.zeros(8, dtype=torch.int32))
        out["plan"][7] = int(bool(w.overflow.any()))
        if cached:
            c = torch.full((n, 5, cap), -7.0)
            ci = c.view(torch.int32)
            Lc = min(w.L, cap)
            lv = q.live[:, :Lc] & ~w.overflow[:, None]
            for row, v in ((0, w.S), (2, q.alpha), (3, q.T)):
                c[:, row, :Lc][lv] = v[:, :Lc][lv]
            ci[:, 1, :Lc][lv] = w.STEP[:, :Lc][lv].int()
            ci[:, 4, :Lc][lv] = q.info[:, :Lc][lv]
            out["cache"] = c.reshape(-1)
        return out

    def plan(self, cnt3, stats, em):
        off3, hdr = R.plan(cnt3.numpy(), em.numpy(), stats.numpy())
        return torch.from_numpy(np.asarray(off3)).int(), hdr + [0]

    def _cache(self, cached):
        """the LDS arrays of the cached FILL / BWD: sdf, step, alpha, T, info [n, L] and n1"""
        n, cap = self.n, self.sc.cap
        c = cached["cache"].view(n, 5, cap)
        n1 = cached["stats"].view(n, 3)[:, 1].long()
        L = max(int(n1.max()) if n else 0, 1)
        live = torch.arange(L)[None] < n1[:, None]
        i32 = lambda row: torch.where(live, c[:, row, :L].contiguous().view(torch.int32), torch.zeros((), dtype=torch.int32))
        f = lambda row: torch.where(live, c[:, row, :L], torch.zeros((), dtype=F32))
        return SimpleNamespace(S=f(0), STEP=i32(1).long(), alpha=f(2), T=f(3), info=i32(4), n1=n1, live=live)

    def fill(self, off3, tiles, cached=None):
        m = max(tiles, 1) * 32
        out = dict(ray=torch.full((m,), -1, dtype=torch.int32), step=torch.full((m,), -7, dtype=torch.int32),
                   w=torch.full((m,), -7.0), sdf=torch.full((m,), -7.0))
        if cached is not None:
            c = self._cache(cached)
            rec = c.info >> 8
            r, j = torch.nonzero(rec, as_tuple=True)
            slot = off3.long()[r] + rec[r, j].long() - 1
            wt = c.T * c.alpha
            if self.mut == "fill_cached_w_from_alpha64":
                a64 = self._alpha(c.S.double(), None, c.STEP, c.n1)[0]
                wt = c.T * a64.float()
            S, STEP = c.S, c.STEP
        else:
            w, q = self.walk(), self.phase2()
            r, j = torch.nonzero(q.v3, as_tuple=True)
            slot = off3.long()[r] + (j if self.mut == "rec_at_survivor_index" else q.rank[r, j])
            if self.mut == "rec_reversed_in_ray":           # every record written, in the ray's own slots, last first
                slot = off3.long()[r] + (q.n3[r] - 1 - q.rank[r, j])
            wt, S, STEP = q.w, w.S, w.STEP
        inside = (slot >= 0) & (slot < m)                    # (a mutant's slots only; the kernel's lie inside by the plan)
        r, j, slot = r[inside], j[inside], slot[inside]
        out["ray"][slot], out["step"][slot] = r.int(), STEP[r, j].int()
        out["w"][slot], out["sdf"][slot] = wt[r, j], S[r, j]
        return out

    def _scatter(self, flat, ind, v):
        """esr_tri_scatter1 of the samples with v != 0"""
        cells, w, inb = _tri(ind, self.sc.dims)
        ok = inb & (w != 0) & (v != 0)[:, None]
        flat.index_add_(0, _flat(cells, self.sc.dims)[ok], (v[:, None] * w)[ok])

    def bwd(self, off3, dweight, dlast, rec=None, acc=0, cached=None):
        sc, n = self.sc, self.n
        grad = torch.zeros(int(np.prod(sc.dims)), dtype=F32)
        ggrad = torch.zeros(int(np.prod(sc.dims)) * 3, dtype=F32)
        w = self.walk()
        if cached is not None:
            c = self._cache(cached)
            S, STEP, alpha, T, info, n1, live, IC = c.S, c.STEP, c.alpha, c.T, c.info, c.n1, c.live, None
            IND = w.IND[:, :S.shape[1]]                      # (the kernel recomputes it from the cached step)
            last = cached["last"]
        else:
            q = self.phase2()
            S, STEP, alpha, T, info, n1, live, IC, IND, last = w.S, w.STEP, q.alpha, q.T, q.info, w.n1, q.live, w.IC, w.IND, q.last
        N, L = S.shape
        proc = (info & 2) != 0
        recno = (info >> 8).long()
        slot = (off3.long()[:, None] + recno - 1).clamp_min(0)
        gw = torch.where(recno > 0, dweight[slot.clamp_max(dweight.numel() - 1)], torch.zeros((), dtype=F32))
        if self.mut == "bwd_stop_term_dropped":
            P = torch.arange(L)[None]
            lastp = (proc * (P + 1)).max(1).values - 1
            proc = proc & ~((P == lastp[:, None]) & (last < _f(1e-3))[:, None])
        x = torch.where(proc, gw * (T * alpha), torch.zeros_like(T))
        back = dlast * last if self.mut != "bwd_no_dlast" else torch.zeros_like(last)
        myback = torch.zeros_like(T)
        for c0 in range((L - 1) // 64 * 64, -1, -64):        # the reverse scan, chunk by chunk
            xs = x[:, c0:c0 + 64]
            v = xs.flip(1).cumsum(1).flip(1)                 # inclusive suffix sum
            myback[:, c0:c0 + 64] = back[:, None] + (v - xs)
            back = back + v[:, 0]
        eps = 0.0 if self.mut == "bwd_no_eps" else 1e-10
        dalpha = ((gw * T).double() - myback.double() / ((1.0 - alpha).double() + eps)).float()
        prv, nxt = self._sections(S, IC, STEP, n1)
        sv = _f(sc.s_val)
        pc, nc = _sigmoid(prv * sv), _sigmoid(nxt * sv)
        num, den = self._numden(pc, nc)
        ratio = num / den
        pos = ((pc - nc >= 0) if self.mut == "bwd_relu_ge" else (pc - nc > 0)).float()
        on = proc & (ratio >= 0) & (ratio <= 1)
        zero = torch.zeros_like(T)
        dprev = torch.where(on, dalpha * ((pos * den - num) / (den * den)) * sv * pc * (1.0 - pc), zero)
        dnext = torch.where(on, dalpha * (-pos / den) * sv * nc * (1.0 - nc), zero)
        if self.ga:
            ds, dic = (dprev + dnext)[live], (dnext - dprev)[live]
            ind = IND[live]
            vd = self._vd(torch.nonzero(live)[:, 0], bwd=True)
            dist = _f(sc.stepdist)
            self._scatter(grad, ind, ds)
            if self.coarse:
                k = dic * 0.5 * dist
                cells, wt, inb = _tri(ind, sc.dims)
                base = _flat(cells, sc.dims) * 3
                order = [1, 2, 0] if self.mut == "coarse_gg_permuted_bwd" else [0, 1, 2]
                for a in range(3):
                    ok = inb & (wt != 0) & ((vd[:, a] != 0) & (dic != 0))[:, None]
                    ggrad.index_add_(0, (base + order[a])[ok], ((k * vd[:, a])[:, None] * wt)[ok])
            else:
                for a, (ixp, ixm, dn) in enumerate(self._taps(ind, bwd=True)):
                    coef = dic * 0.5 * dist * vd[:, a] / dn / _f(sc.vox)
                    self._scatter(grad, ixp, coef)
                    self._scatter(grad, ixm, -coef)
            return grad.view(sc.dims), ggrad.view(*sc.dims, 3), None
        P = torch.arange(L)[None]
        hasp, hasn = P > 0, P < n1[:, None] - 1
        half = lambda h: torch.where(h, _f(0.5), _f(1.0))
        ds = dprev * half(hasp) + dnext * half(hasn)
        ds = torch.where(hasn, ds + 0.5 * torch.cat([dprev[:, 1:], zero[:, :1]], 1), ds)
        ds = torch.where(hasp, ds + 0.5 * torch.cat([zero[:, :1], dnext[:, :-1]], 1), ds)
        dsdf = None
        to_grid = live
        if rec is not None:
            dsdf = rec.clone()
            r, j = torch.nonzero(live & (recno > 0), as_tuple=True)
            sl = slot[r, j]
            dsdf[sl] = dsdf[sl] + ds[r, j] if (acc and self.mut != "rec_overwrite_acc") else ds[r, j]
            if self.mut == "rec_unrecorded_slot_written":
                free = torch.ones(dsdf.numel(), dtype=torch.bool)
                free[sl] = False
                dsdf[free] = 0.0
            if self.mut != "rec_scatters_recorded":
                to_grid = live & (recno == 0)
        self._scatter(grad, IND[to_grid], ds[to_grid])
        return grad.view(sc.dims), ggrad.view(*sc.dims, 3), dsdf
