"""Binary32 emulation of feat_fwd_kernel, feat_fwd16_kernel and feat_bwd_kernel (csrc/feat.hip) in vectorised torch, a backend of
feat_check.py (fwd / fwd16 / bwd) that needs no device: tests/test_feat_ref64_host.py runs the comparison on it -- the bound of
feat_ref64.K_FAMILY is not too tight -- and on every mutant of MUTANTS -- the bound has teeth.

Every binary32 op is formed in float64 and rounded once (_r); fmaf is one rounding (its float64 product is exact; the sum's
double rounding is far below the bound); v_rcp_f32 is modelled as the correctly rounded reciprocal and sinf / cosf as the
correctly rounded functions -- their 1 resp. 2 ulp are terms of K.  Where the source leaves contraction to the compiler
(`out += a * w`, the dot product, grad4's four-term sum) the fused form is taken, as esr_tri_fetch1 spells it.

Forward: the direct form (the bar form is bit-identical by construction, and the GPU test runs both) and the x16 packing.
Positions, indices and tap indices are feat_ref64's replays; the fetches sum corner by corner in the kernel's order.

Backward: the kernel's bookkeeping as well as its arithmetic -- segs_build (heads, cut8), seg_window for both phases (box,
clipping, prefix sum, has), the LDS word offsets (cell0 + (o - 2) sA + b sB + c sC, the colour phase's * 6 + 3h + c, grad4's)
and the flush's decode of a word index through r_row and r_wy.  A window is a float64 array per wave, rounded to binary32 once
at the flush; global-path terms and flushed words are added in binary32 in a fixed order (tile, then ascending lane, then
program order, then the flush).  A word offset outside [0, cells) of its window is recorded in `Emu.misses` (on the GPU it
corrupts a neighbour's window; here it lands in the wave's LDS the same way, or is dropped outside it).  `Emu.book` keeps
the segments and `has` flags per tile: feat_ref64.census must agree with it."""
import numpy as np
import torch

import feat_ref64 as R

F64 = torch.float64
WIN = R.WIN_CELLS


def _r(x):
    return x.float().double()


def _f(v):
    return float(torch.tensor(v, dtype=torch.float32))


def _fma(a, b, c):
    return _r(a * b + c)


def _rcp(x):
    return _r(1.0 / x)


# name -> families it must break (feat_check's families; "window": a word offset outside its window, "bookkeeping": the
# census no longer agrees with the emulation's segments / has flags -- both host-only, tests/test_feat_ref64_host.py)
MUTANTS = {
    # forward
    "axis_order_xyz": ["stencil", "normal"],
    "tap_clamp_displaced_only": ["stencil"],
    "den_two_r": ["normal", "gnorm"],
    "voxel_dropped": ["gnorm"],
    "zero_pad_replicates": ["colour"],
    "tiles_on_le": ["colour"],
    "group1_rows_96": ["colour"],
    "pe_freq_2i": ["pe"],
    "pe_freq_major": ["pe"],
    "pe_of_world": ["pe"],
    "sin_cos_swapped": ["pe", "view"],
    "view_from_rays_d": ["view"],
    "padding_keeps_sdf": ["padding"],
    "x16_slot_identity": ["x16"],
    "x16_alt_quads_group0": ["x16"],
    "unit_by_multiply": ["unit"],
    "gnorm_clamped": ["gnorm"],
    # backward terms
    "no_projection": ["sdf fit", "sdf global"],
    "projection_sign": ["sdf fit", "sdf global"],
    "small_norm_projects": ["sdf fit"],
    "small_norm_inv_norm": ["sdf fit"],
    "thr_sign_swapped": ["sdf fit", "sdf global"],
    "bwd_den_two_r": ["sdf fit"],
    "inv_vox_dropped": ["sdf fit", "sdf global"],
    "value_tap_dropped": ["sdf fit", "sdf global"],
    "value_tap_kept_with_dsdf_out": ["sdf fit", "sdf global"],
    "dsdf_extra_dropped": ["sdf fit", "dsdf_out"],
    "extra_on_covered_tiles_only": ["sdf fit"],
    "second_source_overwrites": ["sdf fit", "sdf global"],
    "uncovered_tile_reads_stale_rows": ["sdf fit"],
    "anchor_unclamped": ["sdf fit"],
    "xbar_cell3_twice": ["sdf fit", "sdf global"],
    "xbar_cell3_never": ["sdf fit", "sdf global"],
    "perp_weights_swapped": ["sdf fit", "sdf global"],
    "g4_scale_inverted": ["sdf grad4"],
    "g4_sign_x": ["sdf grad4"],
    "g4_zero_pad_ignored": ["sdf grad4"],
    "g4_self_drops_dsdf": ["sdf grad4"],
    "g4_corner_from_clamped_base": ["sdf grad4"],
    "colour_both_halves_low_channels": ["colour grid"],
    "colour_on_off_swapped": ["colour grid", "untouched"],
    "colour_rows_of_source0": ["colour grid"],
    # backward bookkeeping
    "sdf_margin_above_2": ["window"],
    "sdf_margin_below_1": ["window"],
    "colour_margin_above_0": ["window"],
    "clip_hi_off_by_one": ["window"],
    "cut8_from_tile_start": ["bookkeeping"],
    "head_ignores_padding_gap": ["bookkeeping"],
    "points_jump_gt_4": ["bookkeeping"],
    "prefix_counts_every_lane": ["bookkeeping"],
    "bwd_tap_round_trip": ["sdf fit"],
    "hat_t_unrounded": ["sdf fit"],
    "flush_row_decode_wd2": ["colour grid"],
    "launch_range_sources_only": ["sdf fit"],
}
# Left out, with the reason:
#   flush_skips_fitting_window_after_overflow (windows_flush `break`s where it `continue`s).  Not a mutant: seg_window's bases are
#   an inclusive prefix sum of the cells over the heads in lane order, cells >= 0.  If a window overflows, base_k + cells_k >
#   WIN_CELLS, then base_(k+1) = base_k + cells_k > WIN_CELLS, so every later window of the tile overflows too: no fitting window
#   follows an overflowing one, and leaving the loop there flushes exactly the same words.  (`mixed` tiles are a fitting prefix
#   followed by an overflowing suffix.)
# Not left out, against expectation: bwd_tap_round_trip, the backward with tap_index's normalise / de-normalise round trip
# (the FEAT_EXP_BWD_ROUNDTRIP build) in place of `ixm = cm`.  The round trip moves a tap by up to 2 ulp OF THE INDEX, i.e. a hat
# weight by up to 2^-22 * index absolutely, and the bound is K 2^-24 of the cell's absref: where the tap sits within an ulp of
# an integer the far cell's whole contribution is that shift, thousands of times its absref-scaled bound already at indices
# of 10-60 (ratios 20 - 3e6 on every host case but the forward-only ones; c2's 255 only makes it larger).  feat_ref64 replays
# `cm` itself, so the check pins the shortcut as the backward's definition: a kernel that switched to the round trip would
# have to change the restatement with it.


# ---- the kernel's bookkeeping, one tile at a time (numpy, lane s = 0..31; both lane halves hold the same values) ---------
def segs_build(key, valid, cut8, i0c, mut=None):
    """segs_build: heads [32] bool, start / last [32], mn / mx [32, 3] per lane (meaningful on valid lanes)"""
    s = np.arange(32)
    pk, pv = np.roll(key, 1), np.roll(valid, 1)
    head = valid & ((s == 0) | ~pv | (key != pk))
    if mut == "head_ignores_padding_gap":
        head = valid & ((s == 0) | (key != pk))

    def starts(head):
        idx = np.where(head, s, -1)
        run = np.maximum.accumulate(idx)
        return np.where(run >= 0, run, s)

    start = starts(head)
    if cut8:
        head = head | (valid & ((((s if mut == "cut8_from_tile_start" else s - start)) & 7) == 0))
        start = starts(head)
    hs = np.nonzero(head)[0]
    endx = np.array([hs[hs > q][0] if (hs > q).any() else 32 for q in s])
    last, mn, mx = s.copy(), np.zeros((32, 3), dtype=np.int64), np.zeros((32, 3), dtype=np.int64)
    for q in s:
        m = valid & (s >= start[q]) & (s < endx[q])
        if m.any():
            last[q] = s[m].max()
            # the segmented scan runs from the segment's start to its last valid sample
            mm = valid & (s >= start[q]) & (s <= last[q])
            mn[q], mx[q] = i0c[mm].min(0), i0c[mm].max(0)
    return head, start, last, mn, mx


def seg_window(start, mn, mx, valid, dims, below, above, ch, mut=None):
    """seg_window: lo / wd [32, 3], cells, base [32], total, has [32]"""
    dm = np.array(dims)
    lo = np.maximum(mn - below, 0)
    top = dm - 1 - (1 if mut == "clip_hi_off_by_one" else 0)
    wd = np.maximum(np.minimum(mx + above, top) - lo + 1, 0)
    want = np.where(valid, wd[:, 0] * wd[:, 1] * wd[:, 2] * ch, 0)
    cells = np.minimum(want, WIN + 1)
    s = np.arange(32)
    inc = np.where(valid & ((s == start) | (mut == "prefix_counts_every_lane")), cells, 0)
    pre = np.cumsum(inc)
    base = pre[start] - cells
    has = valid & (base + cells <= WIN)
    return lo, wd, cells, base, int(pre[31]), has


class Emu:
    def __init__(self, case, mut=None, nwaves=2048):
        assert mut is None or mut in MUTANTS, mut
        self.case, self.mut, self.nwaves = case, mut, nwaves
        self.misses, self.book = [], {}

    def m(self, name):
        return self.mut == name

    # ---- forward ------------------------------------------------------------------------------------------------------
    def _fetch(self, grid, ix, ch):
        """tri_fetch6 / esr_tri_fetch1: fma per corner in the order cx, cy, cz; an out-of-grid corner: value 0, weight 0"""
        dims = self.case.dims
        fl = torch.floor(ix)
        i0 = fl.long()
        x, f = ix.double(), fl.double()
        lo_w, hi_w = _r((f + 1) - x), _r(x - f)
        acc = torch.zeros(ix.shape[0], ch, dtype=F64)
        dm = torch.tensor(dims)
        for cx in (0, 1):
            for cy in (0, 1):
                for cz in (0, 1):
                    c = torch.stack([i0[:, 0] + cx, i0[:, 1] + cy, i0[:, 2] + cz], -1)
                    inb = ((c >= 0) & (c < dm)).all(-1)
                    wx, wy, wz = [(hi_w if cc else lo_w)[:, a] for a, cc in enumerate((cx, cy, cz))]
                    w = _r(_r(wz * wy) * wx)
                    if self.m("zero_pad_replicates"):
                        c, inb = torch.minimum(c.clamp_min(0), dm - 1), torch.ones_like(inb)
                    w = torch.where(inb, w, torch.zeros_like(w))
                    fi = torch.where(inb, R._flat(c, dims), torch.zeros_like(inb, dtype=torch.long))
                    acc = _fma(grid[fi].double().view(-1, ch), w[:, None], acc)
        return acc

    def _tap(self, case, ind, axis, disp):
        if not self.m("tap_clamp_displaced_only"):
            return R.tap_index(case, ind, axis, disp)
        top = torch.tensor([d - 1 for d in case.dims], dtype=F64)
        t = ind.double().clone()
        t[:, axis] = torch.minimum(torch.maximum(_r(t[:, axis] + _f(disp)), torch.zeros(1, dtype=F64)), top[axis])
        n = _r(_r(_r(t / top) * 2.0) - 1.0)
        return _r(_r(_r(n + 1.0) / 2.0) * top).float(), t[:, axis].float()

    def _rows(self, radii):
        """rows [tiles*32, 104] and gnorm [tiles*32, 4] as float64 holding binary32 values"""
        case = self.case if radii is None else R.Case(**{**self.case.__dict__, "grad_feat": radii})
        p, valid = R.positions(case)
        n = case.tiles_all * 32
        X, G = torch.zeros(n, R.XROWS, dtype=F64), torch.zeros(n, 4, dtype=F64)
        jj = torch.nonzero(valid)[:, 0]
        ind = R.world_to_index(case, p[jj])
        M = ind.shape[0]
        t = jj // 32
        on = (t <= case.tiles_on) if self.m("tiles_on_le") else (t < case.tiles_on)
        out = torch.zeros(M, R.XROWS, dtype=F64)
        rows_of = (0, 96, 88) if self.m("group1_rows_96") else R.COLOR_ROW
        for is_on, sel in ((True, on), (False, ~on)):
            for gi, grid in enumerate(case.colour_grids(is_on)):
                if grid is not None and bool(sel.any()):
                    out[sel, rows_of[gi]:rows_of[gi] + 6] = self._fetch(grid.reshape(-1, 6), ind[sel], 6)
        sdfv = case.pt_sdf if case.pts is not None else case.rec_sdf
        sv = torch.zeros(n, dtype=torch.float32)
        sv[:sdfv.shape[0]] = sdfv
        out[:, R.ROW_SDF] = sv[jj].double()
        vox = _f(case.vox)
        sdf = case.sdf.reshape(-1, 1)
        grad = torch.zeros(M, 3, 4, dtype=F64)
        for ar in range(3):
            axis = ar if self.m("axis_order_xyz") else 2 - ar
            for k in range(4):
                ixm, cm = self._tap(case, ind, axis, -case.grad_feat[k])
                ixp, cp = self._tap(case, ind, axis, case.grad_feat[k])
                fm, fp = self._fetch(sdf, ixm, 1)[:, 0], self._fetch(sdf, ixp, 1)[:, 0]
                out[:, R.ROW_FEAT + 2 * ar * 4 + k], out[:, R.ROW_FEAT + (2 * ar + 1) * 4 + k] = fm, fp
                den = _r(_r(cp.double() - cm.double()) + _f(1e-12))
                if self.m("den_two_r"):
                    den = torch.full_like(den, 2.0 * _f(case.grad_feat[k]))
                q = _r(_r(fp - fm) / den)
                grad[:, ar, k] = q if self.m("voxel_dropped") else _r(q / vox)
        g0, g1, g2 = grad[:, 0], grad[:, 1], grad[:, 2]
        nrm = _r(torch.sqrt(_fma(g2, g2, _fma(g1, g1, _r(g0 * g0)))))
        den = nrm.clamp_min(_f(1e-12))
        G[jj] = den if self.m("gnorm_clamped") else nrm
        out[:, R.ROW_NRM:R.ROW_NRM + 12] = _r(grad / den[:, None, :]).reshape(M, 12)
        lo, hi = case.lo.double(), case.hi.double()
        unit = _r(_r(p[jj].double() - lo) / _r(hi - lo))
        if self.m("unit_by_multiply"):
            unit = _r(_r(p[jj].double() - lo) * _rcp(_r(hi - lo)))
        out[:, R.ROW_XYZ:R.ROW_XYZ + 3] = unit
        src = p[jj].double() if self.m("pe_of_world") else unit
        freq = (2.0 * torch.arange(5, dtype=F64)) if self.m("pe_freq_2i") else 2.0 ** torch.arange(5, dtype=F64)
        arg = _r(src[:, :, None] * freq)                                    # [M, 3, 5]
        sn, cs = _r(torch.sin(arg)), _r(torch.cos(arg))
        vd = case.view_inputs()[jj].double()
        if self.m("view_from_rays_d") and case.pts is None:
            vd = case.rays_d[case.rec_ray.long()[jj]].double()
        vs, vc = _r(torch.sin(vd)), _r(torch.cos(vd))
        if self.m("sin_cos_swapped"):
            sn, cs, vs, vc = cs, sn, vc, vs
        if self.m("pe_freq_major"):
            sn, cs = sn.permute(0, 2, 1), cs.permute(0, 2, 1)
        out[:, R.ROW_SIN:R.ROW_SIN + 15], out[:, R.ROW_COS:R.ROW_COS + 15] = sn.reshape(M, 15), cs.reshape(M, 15)
        out[:, R.ROW_VD:R.ROW_VD + 3], out[:, R.ROW_VSIN:R.ROW_VSIN + 3], out[:, R.ROW_VCOS:R.ROW_VCOS + 3] = vd, vs, vc
        X[jj] = out
        if self.m("padding_keeps_sdf"):
            X[~valid, R.ROW_SDF] = sv[~valid].double()
        return X, G

    def fwd(self, radii=None):
        X, G = self._rows(radii)
        T = self.case.tiles_all
        return X.float().view(T, 32, R.XROWS).permute(0, 2, 1).contiguous(), G.float().view(T, 32, 4).permute(0, 2, 1).contiguous()

    def fwd16(self):
        X, G = self._rows(None)
        T = self.case.tiles_all
        Xs = X.float().view(T, 32, R.XROWS)                                 # [tile][sample][row]
        main = Xs[:, :, :96].to(torch.bfloat16).view(T, 32, 24, 4).permute(0, 2, 1, 3)          # [tile][quad][sample][4]
        a0 = 0 if self.m("x16_alt_quads_group0") else 88
        alt = torch.cat([Xs[:, :, a0:a0 + 6], Xs[:, :, 6:8]], 2).to(torch.bfloat16).view(T, 32, 2, 4).permute(0, 2, 1, 3)
        byq = torch.cat([main, alt], 1)
        q = torch.zeros(T, 26, 32, 4, dtype=torch.bfloat16)
        slot = list(range(32)) if self.m("x16_slot_identity") else R.X16_SLOT
        q[:, :, slot, :] = byq
        Xn = torch.full((T, R.XROWS, 32), float("nan"))
        Xn[:, R.ROW_NRM:R.ROW_NRM + 12] = Xs[:, :, R.ROW_NRM:R.ROW_NRM + 12].permute(0, 2, 1)
        return q, Xn, G.float().view(T, 32, 4).permute(0, 2, 1).contiguous()

    # ---- backward -----------------------------------------------------------------------------------------------------
    def _launch_range(self):
        case = self.case
        if self.m("launch_range_sources_only"):
            lo = min([case.tiles_all] + [s.t0 for s in case.srcs])
            hi = max([0] + [s.t1 for s in case.srcs])
            return max(lo, 0), min(hi, case.tiles_all)
        return case.launch_range()

    def _bookkeeping(self, tb, te, valid, i0c, keys_in):
        """per slot of the launch range and phase: has, base, cells, lo, wd; per tile: the flush list"""
        case, dims, mut = self.case, self.case.dims, self.mut
        n = case.tiles_all * 32
        v_np, c_np = valid.numpy(), i0c.numpy()
        lane = {ph: dict(has=np.zeros(n, dtype=bool), base=np.zeros(n, dtype=np.int64), cells=np.zeros(n, dtype=np.int64),
                         lo=np.zeros((n, 3), dtype=np.int64), wd=np.zeros((n, 3), dtype=np.int64)) for ph in ("sdf", "colour")}
        flush = {ph: {} for ph in ("sdf", "colour")}
        book = {}
        marg = {"sdf": (1 if mut == "sdf_margin_below_1" else 2, 2 if mut == "sdf_margin_above_2" else 3, 1),
                "colour": (0, 0 if mut == "colour_margin_above_0" else 1, 6)}
        for t in range(tb, te):
            sl = slice(32 * t, 32 * t + 32)
            v, cc = v_np[sl], c_np[sl]
            if not v.any():
                continue
            if case.pts is not None:
                prev = np.roll(cc, 1, 0)
                pv = np.roll(v, 1)
                jump = v & (np.arange(32) > 0) & pv & (np.abs(cc - prev) > (4 if mut == "points_jump_gt_4" else 3)).any(1)
                key = np.cumsum(jump)
            else:
                key = np.where(v, keys_in[sl], 0)
            head, start, last, mn, mx = segs_build(key, v, False, cc, mut)
            probe = seg_window(start, mn, mx, v, dims, *(marg["sdf"] if case.grad_sdf else marg["colour"]), mut)
            cut8 = probe[4] > WIN
            if cut8:
                head, start, last, mn, mx = segs_build(key, v, True, cc, mut)
            hs = np.nonzero(head)[0]
            book[t] = dict(segs=[(int(h), int(last[h])) for h in hs], cut8=bool(cut8), has={})
            for ph in ("sdf", "colour"):
                if ph == "sdf" and not case.grad_sdf:
                    continue
                lo, wd, cells, base, total, has = seg_window(start, mn, mx, v, dims, *marg[ph], mut)
                L = lane[ph]
                L["has"][sl], L["base"][sl], L["cells"][sl], L["lo"][sl], L["wd"][sl] = has, base, cells, lo, wd
                book[t]["has"][ph] = [bool(x) for x in has]
                flush[ph][t] = [(int(base[h]), int(cells[h]), lo[h].copy(), wd[h].copy()) for h in hs]
        return lane, flush, book

    def _apply(self, grid, tiles, ch, terms, flush, tag):
        """One phase of the launch on one grid.  terms: dict of [K] tensors (tile, order, has, base, cells, off, gidx, val) in
        any order; LDS windows in float64 per tile, flushed in binary32; everything reaches `grid` in a fixed order."""
        dims = self.case.dims
        tix = {t: i for i, t in enumerate(tiles)}
        lds = torch.zeros(len(tiles), WIN, dtype=F64)
        keep = terms["val"] != 0
        T = {k: v[keep] for k, v in terms.items()}
        inw = T["has"]
        bad = inw & ((T["off"] < 0) | (T["off"] >= T["cells"]))
        if bool(bad.any()):
            i = int(torch.nonzero(bad)[0, 0])
            self.misses.append(f"{tag}: {int(bad.sum())} word offsets outside their window, first: tile {int(T['tile'][i])}, "
                               f"offset {int(T['off'][i])} of a window of {int(T['cells'][i])} words (grid index {int(T['gidx'][i])})")
        word = T["base"] + T["off"]
        ok = inw & (word >= 0) & (word < WIN)                                # outside the wave's LDS: dropped here
        trow = torch.tensor([tix[int(t)] for t in T["tile"][ok].tolist()], dtype=torch.long)
        lds.view(-1).index_add_(0, trow * WIN + word[ok], T["val"][ok])
        # global order: tile, then (global-path terms by lane and program order), then the flush
        g_tile, g_ord, g_idx, g_val = [T["tile"][~inw]], [T["order"][~inw]], [T["gidx"][~inw]], [T["val"][~inw]]
        for t in tiles:
            n_seg = 0
            for base, n, lo, wd in flush.get(t, []):
                n_seg += 1
                if base + n > WIN:
                    continue
                v = lds[tix[t], base:base + n].float()
                i = torch.nonzero(v != 0)[:, 0]
                if not i.numel():
                    continue
                row = int(wd[2]) * (1 if self.m("flush_row_decode_wd2") else ch)
                r_row, r_wy = _f(1.0 / _f(float(max(row, 1)))), _f(1.0 / _f(float(max(int(wd[1]), 1))))
                xy = _r(_r(i.double() + 0.5) * r_row).long()
                r = i - xy * row
                wx = _r(_r(xy.double() + 0.5) * r_wy).long()
                wy = xy - wx * int(wd[1])
                gi = (((int(lo[0]) + wx) * dims[1] + (int(lo[1]) + wy)) * dims[2] + int(lo[2])) * ch + r
                g_tile.append(torch.full_like(i, t)); g_ord.append(10 ** 9 + 10 ** 6 * n_seg + i); g_idx.append(gi); g_val.append(v[i].double())
        g_tile, g_ord, g_idx, g_val = torch.cat(g_tile), torch.cat(g_ord), torch.cat(g_idx), torch.cat(g_val)
        oob = (g_idx < 0) | (g_idx >= grid.numel())
        if bool(oob.any()):
            self.misses.append(f"{tag}: {int(oob.sum())} global indices outside the grid, first {int(g_idx[oob][0])}")
            g_tile, g_ord, g_idx, g_val = g_tile[~oob], g_ord[~oob], g_idx[~oob], g_val[~oob]
        if not g_idx.numel():
            return
        o = np.lexsort((g_ord.numpy(), g_tile.numpy(), g_idx.numpy()))      # by cell, then tile, then order
        o = torch.from_numpy(o)
        gi, gv = g_idx[o], g_val[o]
        first = torch.ones(gi.numel(), dtype=torch.bool)
        first[1:] = gi[1:] != gi[:-1]
        pos = torch.arange(gi.numel())
        rank = pos - torch.cummax(torch.where(first, pos, torch.zeros_like(pos)), 0).values
        o2 = torch.argsort(rank, stable=True)
        gi, gv, rank = gi[o2], gv[o2], rank[o2]
        cnt = torch.bincount(rank)
        a = 0
        for c in cnt.tolist():
            grid[gi[a:a + c]] = _r(grid[gi[a:a + c]] + gv[a:a + c])
            a += c

    def bwd(self, X, gnorm):
        case, dims = self.case, self.case.dims
        X, gnorm = X.double(), gnorm.double()
        ncell = dims[0] * dims[1] * dims[2]
        tb, te = self._launch_range()
        p, valid = R.positions(case)
        n = case.tiles_all * 32
        ind_all = R.world_to_index(case, p)
        top32 = torch.tensor([d - 1 for d in dims], dtype=torch.float32)
        indc_all = torch.minimum(torch.maximum(ind_all, torch.zeros(1)), top32)
        i0c_all = torch.where(valid[:, None], torch.floor(indc_all).long(), torch.zeros(n, 3, dtype=torch.long))
        keys = case.rec_ray.numpy() if case.pts is None else None
        lane, flush, self.book = self._bookkeeping(tb, te, valid, i0c_all, keys)
        slots = torch.arange(n)
        jj = slots[valid & (slots // 32 >= tb) & (slots // 32 < te)]
        out = {}
        for i, s in enumerate(case.srcs):
            if s.on:
                out[R.colour_gid(i, True)] = torch.zeros(ncell * 6, dtype=F64)
            if s.off:
                out[R.colour_gid(i, False)] = torch.zeros(ncell * 6, dtype=F64)
        dsdf = torch.full((n,), 12345.0, dtype=F64) if case.dsdf_out else None
        t, s = jj // 32, jj % 32
        ind, indc, i0c = ind_all[jj].double(), indc_all[jj].double(), i0c_all[jj]
        i0 = torch.floor(ind).long()
        tiles = sorted(set(t.tolist()))
        L = lambda ph, k: torch.from_numpy(lane[ph][k])[jj]
        if case.grad_sdf:
            out[R.SDF_GID] = torch.zeros(ncell, dtype=F64)
            self._sdf_phase(out[R.SDF_GID], X, gnorm, jj, t, s, ind, indc, i0, i0c, L, flush["sdf"], tiles, dsdf)
        for k, src in enumerate(case.srcs):
            for is_on in (True, False):
                want_on = (not is_on) if self.m("colour_on_off_swapped") else is_on
                if not (src.on if want_on else src.off):
                    continue
                sel = (t >= src.t0) & (t < src.t1) & ((t < case.tiles_on) == is_on)
                if not bool(sel.any()):
                    continue
                grid = out[R.colour_gid(k, want_on)]
                self._colour_phase(grid, k, sel, jj, t, s, ind, i0, L, flush["colour"], f"colour grid {k} {'on' if want_on else 'off'}")
        out = {g: v.float() for g, v in out.items()}
        return out, (None if dsdf is None else dsdf.float())

    def _dx(self, k, t, s, rows):
        return self.case.srcs[k].dX[t][:, rows, :].gather(2, s[:, None, None].expand(-1, len(rows), 1))[..., 0].double()

    def _sum_rows(self, t, s, rows):
        """rows of dX summed over the covering sources in index order, in binary32; the covered mask"""
        M = t.shape[0]
        acc = torch.zeros(M, len(rows), dtype=F64)
        cov = torch.zeros(M, dtype=torch.bool)
        for k, src in enumerate(self.case.srcs):
            sel = (t >= src.t0) & (t < src.t1)
            if not bool(sel.any()):
                continue
            v = self._dx(k, t[sel], s[sel], rows)
            if self.m("second_source_overwrites"):
                acc[sel] = v
            else:
                acc[sel] = _r(acc[sel] + v)
            cov |= sel
        return acc, cov

    def _sdf_phase(self, grid, X, gnorm, jj, t, s, ind, indc, i0, i0c, L, flush, tiles, dsdf):
        case, dims = self.case, self.case.dims
        M = jj.numel()
        gat = lambda A, rows: A[t][:, rows, :].gather(2, s[:, None, None].expand(-1, len(rows), 1))[..., 0]
        r_n = gat(X, list(range(R.ROW_NRM, R.ROW_NRM + 12))).view(M, 3, 4)
        r_nrm = gat(gnorm, [0, 1, 2, 3])
        r_dn, cov = self._sum_rows(t, s, list(range(R.ROW_NRM, R.ROW_NRM + 12)))
        r_dn = r_dn.view(M, 3, 4)
        r_df, _ = self._sum_rows(t, s, list(range(R.ROW_FEAT, R.ROW_FEAT + 24)))
        r_df = r_df.view(M, 3, 2, 4)
        r6, _ = self._sum_rows(t, s, [R.ROW_SDF])
        r_dsdf = r6[:, 0]
        if self.m("uncovered_tile_reads_stale_rows"):
            # the rows of the tile the wave handled before (t - nwaves), where this one is uncovered
            slot = {int(j): i for i, j in enumerate(jj.tolist())}
            prev = torch.tensor([slot.get(int(j) - 32 * self.nwaves, -1) for j in jj.tolist()])
            st = ~cov & (prev >= 0)
            r_dn[st], r_df[st] = r_dn[prev[st]], r_df[prev[st]]
        if case.dsdf_extra is not None and not self.m("dsdf_extra_dropped"):
            ex = case.dsdf_extra[jj].double()
            if self.m("extra_on_covered_tiles_only"):
                ex = torch.where(cov, ex, torch.zeros_like(ex))
            r_dsdf = _r(r_dsdf + ex)
        g4_self, zero_pad = bool(case.grad4_mode & 2), bool(case.grad4_mode & 1)
        d_sdf = r_dsdf
        if case.dsdf_out or g4_self:
            if case.dsdf_out:
                dsdf[jj] = r_dsdf
            if not self.m("value_tap_kept_with_dsdf_out"):
                d_sdf = torch.zeros_like(r_dsdf)
        if self.m("value_tap_dropped"):
            d_sdf = torch.zeros_like(r_dsdf)
        # through F.normalize
        dot = _fma(r_n[:, 2], r_dn[:, 2], _fma(r_n[:, 1], r_dn[:, 1], _r(r_n[:, 0] * r_dn[:, 0])))       # [M, 4]
        big = r_nrm > _f(1e-12)
        inv = torch.where(big, _rcp(r_nrm.clamp_min(1e-45)), torch.full_like(r_nrm, _f(1e12)))
        if self.m("small_norm_inv_norm"):
            inv = _rcp(r_nrm.clamp_min(_f(1e-30)))
        proj = _fma(r_n if self.m("projection_sign") else -r_n, dot[:, None, :], r_dn)
        use = big | self.m("small_norm_projects")
        if self.m("no_projection"):
            use = torch.zeros_like(big)
        through = _r(torch.where(use[:, None, :], proj, r_dn) * inv[:, None, :])         # [M, 3 (ar), 4]
        vox = _f(case.vox)
        inv_vox = 1.0 if self.m("inv_vox_dropped") else _rcp(torch.tensor(vox, dtype=F64))
        anc_i = i0 if self.m("anchor_unclamped") else i0c
        anc_x = ind if self.m("anchor_unclamped") else indc
        wc = torch.stack([_r((anc_i + 1).double() - anc_x), _r(anc_x - anc_i.double())], -1)       # [M, 3, 2]
        if self.m("perp_weights_swapped"):
            wc = wc.flip(-1)
        has, base, cells, lo, wd = L("sdf", "has"), L("sdf", "base"), L("sdf", "cells"), L("sdf", "lo"), L("sdf", "wd")
        st = [wd[:, 1] * wd[:, 2], wd[:, 2], torch.ones_like(wd[:, 2])]
        gst = [dims[1] * dims[2], dims[2], 1]
        cell0 = ((i0c[:, 0] - lo[:, 0]) * wd[:, 1] + (i0c[:, 1] - lo[:, 1])) * wd[:, 2] + (i0c[:, 2] - lo[:, 2])
        cols = []                                                            # (half, order, off, gidx, val [M])
        order = 0
        for h, bars in ((0, (0, 2)), (1, (1, 2))):                           # lane half h: bar 0 = ar h, bar 1 = ar 2 (x)
            for ar in bars:
                axis = 2 - ar
                iA, dimA, indA = anc_i[:, axis], dims[axis], ind[:, axis]
                baseA = (iA - 2).double()
                acc6 = torch.zeros(M, 6, dtype=F64)
                o6 = torch.arange(6, dtype=F64)

                def deposit(ixA, d):
                    nonlocal acc6
                    tt = (ixA - baseA) if self.m("hat_t_unrounded") else _r(ixA - baseA)
                    hat = _r(1.0 - _r(tt[:, None] - o6).abs()).clamp_min(0.0)
                    acc6 = _fma(hat, d[:, None], acc6)

                if ar == 0:
                    deposit(indA, d_sdf)
                topA = float(dimA - 1)
                for k in range(4):
                    rk = _f(case.grad_feat[k])
                    cm = _r(indA - rk).clamp(0.0, topA)
                    cp = _r(indA + rk).clamp(0.0, topA)
                    den = _r(_r(cp - cm) + _f(1e-12))
                    if self.m("bwd_den_two_r"):
                        den = torch.full_like(den, 2.0 * rk)
                    thr = _r(_r(through[:, ar, k] * _rcp(den)) * inv_vox)
                    if self.m("thr_sign_swapped"):
                        thr = -thr
                    ixm, ixp = cm, cp
                    if self.m("bwd_tap_round_trip"):                 # tap_index's normalise / de-normalise, not `ixm = cm`
                        ixm, ixp = [_r(_r(_r(_r(_r(_r(c / topA) * 2.0) - 1.0) + 1.0) / 2.0) * topA) for c in (cm, cp)]
                    deposit(ixm, _r(r_df[:, ar, 0, k] - thr))
                    deposit(ixp, _r(r_df[:, ar, 1, k] + thr))
                pb, pc = (1 if axis == 0 else 0), (1 if axis == 2 else 2)
                o_lo, o_hi = 0, 6
                if ar == 2:
                    o_lo, o_hi = (3, 6) if h else (0, 3)
                    if self.m("xbar_cell3_twice") and h == 0:
                        o_hi = 4
                    if self.m("xbar_cell3_never") and h == 1:
                        o_lo = 4
                for o in range(o_lo, o_hi):
                    cA = iA - 2 + o
                    okA = (acc6[:, o] != 0) & (cA >= 0) & (cA < dimA)
                    for b in (0, 1):
                        for c in (0, 1):
                            wgt = _r(wc[:, pb, b] * wc[:, pc, c])
                            qb, qc = anc_i[:, pb] + b, anc_i[:, pc] + c
                            ok = okA & (qb < dims[pb]) & (qc < dims[pc]) & (wgt != 0)
                            off = cell0 + ((o - 2) * st[axis] + b * st[pb] + c * st[pc])
                            gi = cA * gst[axis] + qb * gst[pb] + qc * gst[pc]
                            val = torch.where(ok, _r(acc6[:, o] * wgt), torch.zeros(M, dtype=F64))
                            cols.append((h, order, off, gi, val))
                            order += 1
        if case.grad4 is not None or g4_self:
            g4 = case.grad4[jj].double() if case.grad4 is not None else torch.zeros(M, 4, dtype=F64)
            fl = torch.floor(ind)
            wq = torch.stack([_r((fl + 1.0) - ind), _r(ind - fl)], -1)                  # [M, 3, 2]
            ext = _r(case.hi.double() - case.lo.double())
            scale = _r((dm_f(dims) - 1.0) / ext)
            if self.m("g4_scale_inverted"):
                scale = _r(ext / (dm_f(dims) - 1.0))
            gd = _r(g4[:, 1:] * scale)
            gv = _r(g4[:, 0] + r_dsdf) if (g4_self and not self.m("g4_self_drops_dsdf")) else g4[:, 0]
            ub = i0c if self.m("g4_corner_from_clamped_base") else i0
            for cx in (0, 1):
                for cy in (0, 1):
                    for cz in (0, 1):
                        u = torch.stack([ub[:, 0] + cx, ub[:, 1] + cy, ub[:, 2] + cz], -1)
                        cl = torch.minimum(u.clamp_min(0), torch.tensor(dims) - 1)
                        inb = (u == cl).all(-1)
                        sx, sy, sz = [(1.0 if cc else -1.0) for cc in (cx, cy, cz)]
                        if self.m("g4_sign_x"):
                            sx = -sx
                        wx, wy, wz = wq[:, 0, cx], wq[:, 1, cy], wq[:, 2, cz]
                        c0, c1 = _r(_r(wx * wy) * wz), _r(_r(sx * wy) * wz)
                        c2, c3 = _r(_r(wx * sy) * wz), _r(_r(wx * wy) * sz)
                        tv = _fma(gd[:, 2], c3, _fma(gd[:, 1], c2, _fma(gd[:, 0], c1, _r(gv * c0))))
                        if zero_pad and not self.m("g4_zero_pad_ignored"):
                            tv = torch.where(inb, tv, torch.zeros_like(tv))
                        off = cell0 + ((cl[:, 0] - i0c[:, 0]) * wd[:, 1] + (cl[:, 1] - i0c[:, 1])) * wd[:, 2] + (cl[:, 2] - i0c[:, 2])
                        cols.append((cx, order, off, R._flat(cl, dims), tv))
                        order += 1
        self._apply(grid, tiles, 1, self._terms(cols, t, s, has, base, cells), flush, "sdf grid")

    def _terms(self, cols, t, s, has, base, cells):
        C = len(cols)
        hh = torch.tensor([c[0] for c in cols])
        oo = torch.tensor([c[1] for c in cols])
        ex = lambda a: a[:, None].expand(-1, C).reshape(-1)
        order = ((hh[None] * 32 + s[:, None]) * 100000 + oo[None]).reshape(-1)           # lane (s + 32 h), then program order
        return dict(tile=ex(t), order=order, has=ex(has), base=ex(base), cells=ex(cells),
                    off=torch.stack([c[2] for c in cols], 1).reshape(-1), gidx=torch.stack([c[3] for c in cols], 1).reshape(-1),
                    val=torch.stack([c[4] for c in cols], 1).reshape(-1))

    def _colour_phase(self, grid, k, sel, jj, t, s, ind, i0, L, flush, tag):
        dims = self.case.dims
        t, s, ind, i0 = t[sel], s[sel], ind[sel], i0[sel]
        M = t.numel()
        g = lambda key: L("colour", key)[sel]
        has, base, cells, lo, wd = g("has"), g("base"), g("cells"), g("lo"), g("wd")
        d6 = self._dx(0 if self.m("colour_rows_of_source0") else k, t, s, list(range(6)))
        fl = i0.double()
        lo_w, hi_w = _r((fl + 1) - ind), _r(ind - fl)
        sx, sy = wd[:, 1] * wd[:, 2] * 6, wd[:, 2] * 6
        cols, order = [], 0
        dm = torch.tensor(dims)
        for h in (0, 1):
            hc = 0 if self.m("colour_both_halves_low_channels") else 3 * h
            cell0 = (((i0[:, 0] - lo[:, 0]) * wd[:, 1] + (i0[:, 1] - lo[:, 1])) * wd[:, 2] + (i0[:, 2] - lo[:, 2])) * 6 + hc
            for cx in (0, 1):
                for cy in (0, 1):
                    for cz in (0, 1):
                        c = torch.stack([i0[:, 0] + cx, i0[:, 1] + cy, i0[:, 2] + cz], -1)
                        inb = ((c >= 0) & (c < dm)).all(-1)
                        wx, wy, wz = [(hi_w if cc else lo_w)[:, a] for a, cc in enumerate((cx, cy, cz))]
                        w = _r(_r(wz * wy) * wx)
                        ok = inb & (w != 0)
                        for ch in range(3):
                            val = torch.where(ok, _r(d6[:, 3 * h + ch] * w), torch.zeros(M, dtype=F64))
                            cols.append((h, order, cell0 + (cx * sx + cy * sy + cz * 6 + ch), R._flat(c, dims) * 6 + hc + ch, val))
                            order += 1
        self._apply(grid, sorted(set(t.tolist())), 6, self._terms(cols, t, s, has, base, cells), flush, tag)


def dm_f(dims):
    return torch.tensor([float(d) for d in dims], dtype=F64)
