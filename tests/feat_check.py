"""The comparison of one feature-kernel backend with the float64 restatement feat_ref64.py: case builders, the flows of the
cases, the census requirements and the per-value checks.  No device and no library here: a backend is any object with

    fwd(radii=None) -> (X [tiles, 104, 32], gnorm [tiles, 4, 32])
    fwd16()         -> (X16 [tiles, 26, 32, 4] bfloat16, X, gnorm)            esr_fine_feat_fwd_x16: X holds rows 31..42 only
    bwd(X, gnorm)   -> ({gid: flat grid}, dsdf_out or None)

returning CPU tensors in the ABI's layout and reading the case's fields when called (the flows change srcs, dsdf_extra, ...
between launches); `make(case)` builds one: the ctypes launches (tests/test_gpu_feat_scatter.py) or the binary32 emulation
(feat_emu.Emu; tests/test_feat_ref64_host.py).

Per-cell / per-value bound: |got - ref| <= K * 2^-24 * absref + FLOOR with K = feat_ref64.K_FAMILY[family]; absref: the same
sum on magnitudes (feat_ref64's docstring).  Exact families have no K: the SDF value row, `unit` (a binary32 replay), the
zero rows, padding lanes, dsdf_out, untouched cells (exactly 0) and finiteness.  Families:
  forward   colour (rows 0-5, 88-93, 96-101), sdf value, stencil (7-30), normal (31-42), gnorm, unit (43-45), pe (46-75),
            view (76-84), zero rows (85-87, 94, 95, 102, 103), padding, x16 (the bf16 row-quad tile)
  backward  sdf fit (cells reached only by terms of lanes whose window fits: one rounding at the flush), sdf global (at least
            one term went through a global atomic: one binary32 add per term), sdf grad4 (reached by a grad4 term), colour
            grid, dsdf_out, untouched, finite
Nothing raises: every miss is appended to `Check.fails` as (family, message) with the cell or row named (and the path
classes of the tiles that reach a cell), the worst ratios |got - ref| / (2^-24 absref) per family go to `Check.worst`."""
import numpy as np
import torch

import feat_ref64 as R

FLOOR = 1e-30
DEFAULT_RADII = (0.5, 1.0, 1.5, 2.0)
DIRECT_RADII = (0.5, 1.0, 1.5, 2.5)        # a radius beyond the bars' reach: esr_fine_feat_fwd runs the direct form
GRIDS = {"tiny": (64, 64, 16), "odd": (37, 61, 23), "c2": (256, 256, 64), "g256": (256, 256, 256)}
VOX = 1.0 / 64
ROW_FAMILY = R.row_families()


class Check:
    """What one or more checks found."""

    def __init__(self, K=None):
        self.K = dict(R.K_FAMILY) if K is None else K
        self.fails, self.worst, self.census = [], {}, {}

    def fail(self, family, msg):
        self.fails.append((family, msg))

    def exact(self, family, cond, msg):
        if not bool(cond):
            self.fail(family, msg)
        return bool(cond)

    def ratio(self, family, r):
        self.worst[family] = max(self.worst.get(family, 0.0), float(r))

    def families(self):
        return {f for f, _ in self.fails}

    def report(self):
        return "\n".join(f"[{f}] {m}" for f, m in self.fails)


def _box(dims):
    half = torch.tensor([(d - 1) * VOX / 2 for d in dims], dtype=torch.float32)
    return -half, half


def _base_case(dims, tiles_all, radii=DEFAULT_RADII, seed=0):
    lo, hi = _box(dims)
    g = torch.Generator().manual_seed(seed)
    return R.Case(lo=lo, hi=hi, dims=dims, vox=VOX, stepdist=0.5 * VOX, grad_feat=radii, tiles_all=tiles_all,
                  sdf=torch.randn(*dims, generator=g), color_on=torch.randn(*dims, 6, generator=g) * 0.3,
                  color_off=torch.randn(*dims, 6, generator=g) * 0.3)


def _to_world(case, idx):
    """continuous grid index -> world point (binary32)"""
    lo, hi = case.lo.double(), case.hi.double()
    top = torch.tensor([d - 1 for d in case.dims], dtype=torch.float64)
    return (lo + idx.double() / top * (hi - lo)).float()


# ---- geometries -------------------------------------------------------------------------------------------------------
def _inside(case, p, margin=0.0):
    return ((p >= case.lo - margin) & (p <= case.hi + margin)).all(-1)


def ray_records(case, kinds, g):
    """March records of the record-mode geometries, in tile order; returns rays_o, rays_d, rec_ray, rec_step, tiles.  Each
    geometry starts a fresh tile, so a geometry's last tile is a partial one (padding lanes at its end)."""
    dims = case.dims
    lo, hi = case.lo, case.hi
    rays_o, rays_d, recs = [], [], []

    def add_ray(o, d, steps, pad_after=False):
        r = len(rays_o)
        rays_o.append(o); rays_d.append(d)
        tmp = R.Case(lo=lo, hi=hi, dims=dims, vox=case.vox, stepdist=case.stepdist, grad_feat=case.grad_feat, tiles_all=1,
                     rays_o=o[None].float(), rays_d=d[None].float(), rec_ray=torch.zeros(len(steps), dtype=torch.int32),
                     rec_step=torch.tensor(steps, dtype=torch.int32))
        p, _ = R.record_points(tmp)
        ok = _inside(case, p)
        for q, st in enumerate(steps):
            if ok[q]:
                recs.append((r, st))
        if pad_after:
            recs.append((-1, 0))

    ext = (hi - lo)
    for kind, n in kinds:
        for i in range(n):
            if kind == "axis":                        # primary rays along -z, walking the whole box
                o = torch.cat([lo[:2] + ext[:2] * (0.05 + 0.9 * torch.rand(2, generator=g)), hi[2:] + 0.5])
                add_ray(o, torch.tensor([0.0, 0.0, -1.0]), list(range(2 * dims[2] + 4)))
            elif kind == "diag":                      # along (1,1,1): 32 samples span 9 cells per axis
                c = lo + ext * (0.3 + 0.4 * torch.rand(3, generator=g))
                d = torch.tensor([1.0, 1.0, 1.0])
                o = c - d * 0.5 * float(ext.min())
                add_ray(o, d, list(range(0, 2 * int(ext.min() / case.vox * 1.7))))
            elif kind == "graze":                     # along x, within 1e-3 voxel of a y face (low or high)
                side = i % 2
                y = (lo[1] + 1e-3 * case.vox) if side == 0 else (hi[1] - 1e-3 * case.vox)
                z = lo[2] + ext[2] * (0.1 + 0.8 * torch.rand(1, generator=g))
                o = torch.stack([lo[0] - 0.5, torch.as_tensor(y), z[0]])
                add_ray(o, torch.tensor([1.0, 0.0, 0.0]), list(range(64)))
            elif kind == "pieces":                    # 2-6 steps from random interior points: LTS secondary rays
                o = lo + ext * (0.1 + 0.8 * torch.rand(3, generator=g))
                d = torch.nn.functional.normalize(torch.randn(3, generator=g), dim=0)
                k = int(torch.randint(2, 7, (1,), generator=g))
                first = int(torch.randint(0, 3, (1,), generator=g))
                add_ray(o, d, list(range(first, first + k)), pad_after=(i % 7 == 3))
            elif kind == "corner":                    # short pieces at the lowest and highest cells of the grid
                at_hi = i % 2
                o = (hi - ext * 0.02 * torch.rand(3, generator=g)) if at_hi else (lo + ext * 0.02 * torch.rand(3, generator=g))
                d = torch.tensor([-1.0, -1.0, -1.0]) if at_hi else torch.tensor([1.0, 1.0, 1.0])
                add_ray(o, d, list(range(3)))
        # each geometry starts on a fresh tile (a tile's path class then belongs to one geometry)
        while len(recs) % 32:
            recs.append((-1, 0))
    tiles = (len(recs) + 31) // 32
    recs += [(-1, 0)] * (tiles * 32 - len(recs))
    rr = torch.tensor([a for a, _ in recs], dtype=torch.int32)
    rs = torch.tensor([b for _, b in recs], dtype=torch.int32)
    return torch.stack(rays_o).float(), torch.stack(rays_d).float(), rr, rs, tiles


def point_runs(case, kinds, g):
    """Explicit points in ray order: runs with jumps of exactly 3 cells (one run) and 4 cells (split), scattered
    singletons, points up to 1 voxel outside the box, runs over the whole box."""
    dims = torch.tensor(case.dims)
    out = []
    for kind, n in kinds:
        pts = []
        if kind == "jumps":
            for i in range(n):
                c = (torch.rand(3, generator=g) * (dims - 16).clamp_min(1)).floor() + 2
                for run in range(4):
                    for q in range(8):
                        pts.append(c + torch.tensor([0.3, 0.3, 0.25 + 0.5 * q / 4]))
                    c = c + torch.tensor([3.0 if run % 2 == 0 else 4.0, 0.0, 0.0])
        elif kind == "scatter":
            pts = list(torch.rand(n * 32, 3, generator=g) * (dims - 1))
        elif kind == "outside":                         # around / beyond a face, up to 1 voxel
            for i in range(n * 32):
                p = torch.rand(3, generator=g) * (dims - 1)
                a = int(torch.randint(0, 3, (1,), generator=g))
                p[a] = (dims[a] - 1 if i % 2 else 0) + (torch.rand(1, generator=g)[0] * 2 - 1)
                pts.append(p)
        elif kind == "runs":                             # 8-sample runs at random places over the whole box
            for i in range(n * 4):
                c = 4 + torch.rand(3, generator=g) * (dims - 9)
                d = torch.nn.functional.normalize(torch.randn(3, generator=g), dim=0) * 0.5
                pts += [c + d * q for q in range(8)]
            pts[-1] = (dims - 1).double() - 1e-3         # the very last cell: the largest flush indices
        idx = torch.stack(pts).float()
        pad = (-idx.shape[0]) % 32                       # each geometry fills whole tiles: repeats of its last point
        out.append(torch.cat([idx, idx[-1:].expand(pad, 3)]))
    return torch.cat(out)


def _dX(tiles, g):
    dX = torch.randn(tiles, 64, 32, generator=g)
    dX[:, 43:] = 0.0
    return dX


def _set_points(case, pts, g, view=True):
    n = pts.shape[0]
    tiles = (n + 31) // 32
    case.pts, case.pt_sdf, case.tiles_all = pts, torch.randn(n, generator=g), tiles
    if view:                                             # (generator of its own: the cases' other draws stay as they were)
        gv = torch.Generator().manual_seed(n)
        case.pt_viewdirs = torch.nn.functional.normalize(torch.randn(n, 3, generator=gv), dim=-1)
    return tiles


def _zero_far_stencil_rows(case, dXs):
    """stencil rows of points more than half a voxel outside: their +-0.5 taps clamp onto each other, where the difference
    quotient is 0 / 1e-12 (the reference's own gradient is noise there); colour and value rows stay"""
    far = ~_inside(case, case.pts, 0.5 * case.vox * 0.999)
    jf = torch.nonzero(far)[:, 0]
    for d in dXs:
        d[jf // 32, 7:43, jf % 32] = 0.0


# ---- checks -----------------------------------------------------------------------------------------------------------
def _cell_name(case, gid, flat):
    dims = case.dims
    ch = 0
    if gid != R.SDF_GID:
        flat, ch = divmod(flat, 6)
    z = flat % dims[2]
    y = (flat // dims[2]) % dims[1]
    x = flat // (dims[1] * dims[2])
    return f"grid {gid} cell (x {x}, y {y}, z {z}, channel {ch})"


def _has_lanes(case, census_tiles, phase):
    """per sample slot: its lane's window fits in `phase` (False outside the launch range)"""
    tb, _ = case.launch_range()
    has = torch.zeros(case.tiles_all * 32, dtype=torch.bool)
    for n, info in enumerate(census_tiles):
        if info and phase in info["has"]:
            has[(tb + n) * 32:(tb + n) * 32 + 32] = torch.tensor(info["has"][phase])
    return has


def check_grids(tag, case, ref, out, census_tiles, dsdf, ck):
    """Every touched cell within its family's bound, every other cell exactly 0, dsdf_out per lane exactly."""
    tb, _ = case.launch_range()
    for gid, buf in out.items():
        buf = buf.reshape(-1)
        ck.exact("finite", torch.isfinite(buf).all(), f"{tag}: grid {gid}: {int((~torch.isfinite(buf)).sum())} non-finite cells")
        if gid not in ref.cells:                              # nothing reaches this grid
            nz = torch.nonzero(buf != 0)[:, 0]
            ck.exact("untouched", nz.numel() == 0, f"{tag}: grid {gid} should be untouched: {nz.numel()} non-zero cells, first "
                     f"{_cell_name(case, gid, int(nz[0])) if nz.numel() else ''}")
            continue
        u, v, a = ref.cells[gid]
        tf, _, _, tt, tl, tg4 = ref.terms[gid]
        got = buf[u].double()
        err = (got - v).abs()
        err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))

        def info_of(fl):
            tiles = sorted(set(tt[tf == fl].tolist()))[:6]
            return [(t, census_tiles[t - tb]["classes"] if census_tiles[t - tb] else None) for t in tiles]

        if gid == R.SDF_GID:
            pos = torch.searchsorted(u, tf)
            glob = ~_has_lanes(case, census_tiles, "sdf")[tl]
            cg4 = torch.zeros(u.numel(), dtype=torch.bool).index_put((pos[tg4],), torch.tensor(True))
            cgl = torch.zeros(u.numel(), dtype=torch.bool).index_put((pos[glob],), torch.tensor(True))
            fams = {"sdf grad4": cg4, "sdf global": cgl & ~cg4, "sdf fit": ~cgl & ~cg4}
        else:
            fams = {"colour grid": torch.ones(u.numel(), dtype=torch.bool)}
        for fam, sel in fams.items():
            if not bool(sel.any()):
                continue
            e, aa = err[sel], a[sel]
            bound = ck.K[fam] * R.U * aa + FLOOR
            ck.ratio(fam, (e / (R.U * aa + FLOOR)).max())
            bad = e > bound
            if bool(bad.any()):
                i = int(torch.nonzero(sel)[:, 0][int((e / bound).argmax())])
                fl = int(u[i])
                ck.fail(fam, f"{tag}: {_cell_name(case, gid, fl)}: |got - ref| = {float(err[i]):.3e} > bound "
                        f"{float(ck.K[fam] * R.U * a[i] + FLOOR):.3e} (got {float(got[i]):.9e}, ref {float(v[i]):.9e}, absref "
                        f"{float(a[i]):.3e}); {int(bad.sum())} of {int(sel.sum())} cells; tiles / path classes: {info_of(fl)}")
        nz_all, nz_touched = int((buf != 0).sum()), int((got != 0).sum())
        if nz_all != nz_touched:                              # a non-zero cell outside the touched set
            extra = torch.nonzero(buf != 0)[:, 0]
            f0 = int(extra[~torch.isin(extra, u)][0])
            ck.fail("untouched", f"{tag}: {_cell_name(case, gid, f0)}: non-zero ({float(buf[f0]):.3e}) but no term reaches it "
                    f"({nz_all} non-zero, {nz_touched} touched)")
    if case.dsdf_out:
        want, jj = ref.dsdf_out
        if ck.exact("dsdf_out", dsdf is not None, f"{tag}: no dsdf_out returned"):
            got = dsdf.reshape(-1)
            diff = torch.nonzero(got[jj].float() != want)[:, 0]
            ck.exact("dsdf_out", diff.numel() == 0, f"{tag}: dsdf_out differs in {diff.numel()} lanes, first slot "
                     f"{int(jj[diff[0]]) if diff.numel() else -1}")
            untouched = torch.ones(got.numel(), dtype=torch.bool)
            untouched[jj] = False
            ck.exact("dsdf_out", (got[untouched] == 12345.0).all(), f"{tag}: dsdf_out written outside the valid lanes")


def _ref_forward(case, radii):
    c = case if radii is None else R.Case(**{**case.__dict__, "grad_feat": radii})
    p, valid = R.positions(c)
    return (valid,) + R.forward_rows(c, p, valid)


def check_rows(tag, ck, X, gn, valid, val, scl, nrm, nabs, rows=range(R.XROWS)):
    """rows of X and gnorm against the restatement, per family; padding lanes exactly 0"""
    jj = torch.nonzero(valid)[:, 0]
    rows = list(rows)
    got = X.permute(0, 2, 1).reshape(-1, R.XROWS)[jj][:, rows].double()
    err = (got - val[:, rows]).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    for fam in sorted(set(ROW_FAMILY[r] for r in rows)):
        cols = [n for n, r in enumerate(rows) if ROW_FAMILY[r] == fam]
        K = ck.K.get(fam, 0)
        e, s = err[:, cols], scl[:, rows][:, cols]
        bound = K * R.U * s + FLOOR
        if fam in ck.K:
            ck.ratio(fam, (e / (R.U * s + FLOOR)).max() if e.numel() else 0.0)
        bad = e > bound
        if bool(bad.any()):
            i = int((e / bound).flatten().argmax())
            m, c = divmod(i, len(cols))
            r = rows[cols[c]]
            ck.fail(fam, f"{tag}: forward row {r} of sample {int(jj[m])} (tile {int(jj[m]) // 32}, lane {int(jj[m]) % 32}): got "
                    f"{float(got[m, cols[c]]):.9e}, ref {float(val[m, r]):.9e}, scale {float(scl[m, r]):.3e}; {int(bad.sum())} of "
                    f"{bad.numel()} values")
    gg = gn.permute(0, 2, 1).reshape(-1, 4)[jj].double()
    e = (gg - nrm).abs()
    e = torch.where(torch.isfinite(e), e, torch.full_like(e, float("inf")))
    ck.ratio("gnorm", (e / (R.U * nabs + FLOOR)).max() if e.numel() else 0.0)
    bad = e > ck.K["gnorm"] * R.U * nabs + FLOOR
    if bool(bad.any()):
        i = int((e / (ck.K["gnorm"] * R.U * nabs + FLOOR)).flatten().argmax())
        m, k = divmod(i, 4)
        ck.fail("gnorm", f"{tag}: gnorm {k} of sample {int(jj[m])} (tile {int(jj[m]) // 32}): got {float(gg[m, k]):.9e}, ref "
                f"{float(nrm[m, k]):.9e}, absref {float(nabs[m, k]):.3e}; {int(bad.sum())} of {bad.numel()} values")
    pad = torch.nonzero(~valid)[:, 0]
    if pad.numel():
        px = X.permute(0, 2, 1).reshape(-1, R.XROWS)[pad][:, rows]
        pg = gn.permute(0, 2, 1).reshape(-1, 4)[pad]
        nzp = torch.nonzero((px != 0).any(1) | (pg != 0).any(1))[:, 0]
        if nzp.numel():
            j = int(pad[nzp[0]])
            rr = [rows[c] for c in torch.nonzero(px[nzp[0]] != 0)[:, 0].tolist()]
            ck.fail("padding", f"{tag}: padding lane {j % 32} of tile {j // 32} (slot {j}) is not zero: rows {rr[:8]}, gnorm "
                    f"{pg[nzp[0]].tolist()}; {nzp.numel()} such lanes")


def check_forward(tag, case, backend, radii, ck):
    X, gn = backend.fwd(radii)
    check_rows(tag, ck, X, gn, *_ref_forward(case, radii))
    return X, gn


def check_x16(tag, case, backend, ck):
    """esr_fine_feat_fwd_x16 against the restatement rounded to bf16: a value must lie between the bf16 roundings of
    ref - bound and ref + bound (the bf16 neighbour is allowed where the binary32 value may sit on either side of a tie),
    bound the binary32 row's own; the alternate quads carry group 1 in front of rows 6 and 7; X: rows 31..42 only."""
    q, X, gn = backend.fwd16()
    valid, val, scl, nrm, nabs = _ref_forward(case, None)
    check_rows(tag + " x16", ck, X, gn, valid, val, scl, nrm, nabs, rows=range(R.ROW_NRM, R.ROW_NRM + 12))
    main, alt = R.x16_decode(q)
    T = case.tiles_all
    Krow = torch.tensor([ck.K.get(f, 0) for f in ROW_FAMILY], dtype=torch.float64)
    full_v, full_b = torch.zeros(T * 32, R.XROWS, dtype=torch.float64), torch.zeros(T * 32, R.XROWS, dtype=torch.float64)
    full_v[valid], full_b[valid] = val, Krow * R.U * scl + FLOOR            # padding lanes: exactly 0
    arows = list(range(88, 94)) + [6, 7]
    for name, got, rows in (("rows", main.permute(0, 2, 1).reshape(T * 32, 96), list(range(96))),
                            ("alternate quads", alt.permute(0, 2, 1).reshape(T * 32, 8), arows)):
        v, b = full_v[:, rows], full_b[:, rows]
        bad = ~((got >= R.round_bf16(v - b)) & (got <= R.round_bf16(v + b)))
        if bool(bad.any()):
            j, c = torch.nonzero(bad)[0].tolist()
            ck.fail("x16", f"{tag}: x16 {name}: row {rows[c]} ({ROW_FAMILY[rows[c]]}) of slot {j} (tile {j // 32}, lane {j % 32}, "
                    f"{'valid' if bool(valid[j]) else 'padding'}): got {float(got[j, c]):.6e}, ref {float(v[j, c]):.9e} -> bf16 "
                    f"{float(R.round_bf16(v[j, c])):.6e}; {int(bad.sum())} of {bad.numel()} values")


def census(tag, case, need, ck, gnorm=None):
    tiles, counts = R.census(case, gnorm=gnorm)
    ck.census[tag] = counts
    for cls, n in need.items():
        ck.exact("census", counts[cls] >= n, f"{tag}: path class {cls}: {counts[cls]} tiles, this case needs >= {n} ({counts})")
    return tiles


def run(tag, case, backend, need, ck, X=None, gn=None):
    if X is None:
        X, gn = backend.fwd()
    tiles = census(tag, case, need, ck, gnorm=gn)
    out, dsdf = backend.bwd(X, gn)
    ref = R.scatter(case, X, gn)
    check_grids(tag, case, ref, out, tiles, dsdf, ck)
    return X, gn


def bar_reach(case, ind=None):
    """feat_fwd_kernel<BAR>'s o = t.i0[axis] - b0 of all eight taps of each axis, for every valid sample (or the indices
    given): [M, 3, 8] int64.  bar_fetch1 reads bar + o * 4 .. + 8 of a 7-cell bar: 0 <= o <= 5 is what it needs."""
    if ind is None:
        p, valid = R.positions(case)
        ind = R.world_to_index(case, p[valid])
    out = torch.zeros(ind.shape[0], 3, 8, dtype=torch.long)
    for axis in range(3):
        taps = [R.tap_index(case, ind, axis, s * case.grad_feat[k])[0][:, axis] for k in range(4) for s in (-1.0, 1.0)]
        low = torch.stack(taps[0::2], 1).min(1).values                 # the kernel's: min over the four minus taps
        b0 = torch.floor(low).long()
        out[:, axis] = torch.floor(torch.stack(taps, 1)).long() - b0[:, None]
    return out


# ---- cases: the flows of tests/test_gpu_feat_scatter.py ---------------------------------------------------------------
NEED_RAYS = dict(fit=8, cut8_fit=4, cut8_global=2, mixed=2, clip_lo=4, clip_hi=4)
NEED_RAYS_COLOUR = dict(colour_only=20, fit=8, cut8_fit=4, clip_hi=2)
NEED_POINTS = dict(fit=4, cut8_global=4, mixed=4, clip_lo=2, clip_hi=2)
NEED_G256 = dict(fit=30, clip_hi=1, cut8_global=2)
NEED_FLAT = dict(small_norm=3, fit=2)


def record_mode_case(grid):
    dims = GRIDS[grid]
    g = torch.Generator().manual_seed(100 + len(grid))
    case = _base_case(dims, 1, seed=1)
    n_axis = 24 if grid != "c2" else 8
    ro, rd, rr, rs, tiles = ray_records(case, [("axis", n_axis), ("diag", 12), ("graze", 8), ("pieces", 160),
                                               ("corner", 40)], g)
    case.rays_o, case.rays_d, case.rec_ray, case.rec_step, case.tiles_all = ro, rd, rr, rs, tiles
    case.rec_sdf = torch.randn(tiles * 32, generator=g)
    case.tiles_on = tiles // 3
    case.srcs = [R.Src(_dX(tiles, g), 0, tiles, on=True, off=True)]
    return case


def flow_record_mode(grid, make, ck, sampler=None):
    """Axis-parallel, (1,1,1)-diagonal, face-grazing, short-piece (padding lanes mid-tile) and corner tiles, partial last
    tile; on/off colour grids split by tiles_on; then the same tiles as a colour-only launch (grad_sdf NULL)."""
    case = record_mode_case(grid)
    be = make(case)
    if sampler:
        sampler(case, be)
    check_forward(f"{grid}/rays bar", case, be, None, ck)
    check_forward(f"{grid}/rays direct", case, be, DIRECT_RADII, ck)
    check_x16(f"{grid}/rays", case, be, ck)
    run(f"{grid}/rays", case, be, NEED_RAYS, ck)
    case.grad_sdf = False
    # (colour windows have no margin below the base cells: they clip at dims - 1 only)
    run(f"{grid}/rays colour-only", case, be, NEED_RAYS_COLOUR, ck)


def explicit_points_case(grid):
    dims = GRIDS[grid]
    g = torch.Generator().manual_seed(200 + len(grid))
    case = _base_case(dims, 1, seed=2)
    pts = _to_world(case, point_runs(case, [("jumps", 8), ("scatter", 6), ("outside", 4)], g))
    tiles = _set_points(case, pts, g)
    case.tiles_on = tiles // 2
    dX = _dX(tiles, g)
    _zero_far_stencil_rows(case, [dX])
    case.srcs = [R.Src(dX, 0, tiles, on=True, off=True)]
    case.dsdf_out = True
    return case


def flow_explicit_points(grid, make, ck):
    """Ray-ordered runs with jumps of 3 cells (one window) and 4 cells (cut), scattered singletons (32 windows, most on
    global atomics), points up to 1 voxel outside the box; dsdf_out, the SDF value as an input."""
    case = explicit_points_case(grid)
    be = make(case)
    check_forward(f"{grid}/points bar", case, be, None, ck)
    check_forward(f"{grid}/points direct", case, be, DIRECT_RADII, ck)
    check_x16(f"{grid}/points", case, be, ck)
    run(f"{grid}/points", case, be, NEED_POINTS, ck)


def production_case(dims=GRIDS["g256"], n_runs=60):
    g = torch.Generator().manual_seed(300)
    case = _base_case(dims, 1, seed=3)
    idx = point_runs(case, [("runs", n_runs), ("scatter", 4)], g)
    tiles = _set_points(case, _to_world(case, idx), g)
    case.srcs = [R.Src(_dX(tiles, g), 0, tiles, on=False, off=True)]
    case.dsdf_out = True
    return case


def flow_production(make, ck, dims=GRIDS["g256"], need=NEED_G256, tag="g256"):
    """8-sample runs over the whole box up to its last cell, so window origins and flush indices reach the largest values;
    touched cells compared, the rest must stay 0."""
    case = production_case(dims)
    be = make(case)
    check_forward(f"{tag}/points bar", case, be, None, ck)
    run(f"{tag}/points", case, be, need, ck)
    return case


def _abi_case(seed):
    dims = GRIDS["odd"]
    g = torch.Generator().manual_seed(seed)
    case = _base_case(dims, 1, seed=seed)
    idx = point_runs(case, [("jumps", 10), ("scatter", 4), ("runs", 10)], g)
    tiles = _set_points(case, _to_world(case, idx), g)
    return case, g, tiles


def flow_multi_source(make, ck):
    """n_src 2 and 3: dX rows 6-42 summed over the sources covering a tile, colour rows to each source's own grid;
    tiles_on routes a tile's colour to grad_color_on / _off, NULL for one of them; sources over part of the tiles."""
    case, g, T = _abi_case(400)
    case.tiles_on = T // 3
    case.srcs = [R.Src(_dX(T, g), 0, T, on=True, off=True), R.Src(_dX(T, g), 0, T // 2, on=False, off=True),
                 R.Src(_dX(T, g), T // 4, 3 * T // 4, on=True, off=False)]
    be = make(case)
    X, gn = run("abi/3 sources", case, be, dict(fit=4, cut8_global=1), ck)
    case.srcs = case.srcs[:2]
    case.srcs[1] = R.Src(case.srcs[1].dX, T // 5, T, on=True, off=False)
    run("abi/2 sources", case, be, dict(fit=4), ck, X, gn)
    # a source over part of the tiles: the launch covers its range only
    case.srcs = [R.Src(_dX(T, g), T // 4, T // 2, on=True, off=True)]
    ck.exact("census", case.launch_range() == (T // 4, T // 2), "abi/partial source: launch range")
    run("abi/partial source", case, be, dict(fit=2), ck, X, gn)


PARTIAL_EXTRAS = ["gap+dsdf_extra", "dsdf_out", "grad4-0", "grad4-1", "grad4-2", "grad4-3"]


def partial_sources_case(extra):
    case, g, T = _abi_case(500)
    # points up to a voxel outside the box, for the border-replicated / dropped corners of grad4 (stencil rows zeroed)
    out_idx = point_runs(case, [("outside", 2)], g)
    T = _set_points(case, torch.cat([case.pts, _to_world(case, out_idx)]), g)
    dX0, dX1 = _dX(T, g), _dX(T, g)
    _zero_far_stencil_rows(case, [dX0, dX1])
    case.srcs = [R.Src(dX0, 0, T // 3, on=True, off=True), R.Src(dX1, 2 * T // 3, T - 1, on=True, off=True)]
    case.tiles_on = T // 2
    if extra == "gap+dsdf_extra":
        case.dsdf_extra = torch.randn(T * 32, generator=g)
    elif extra == "dsdf_out":
        case.dsdf_out = True
        case.dsdf_extra = torch.randn(T * 32, generator=g)
    else:
        mode = int(extra[-1])
        case.grad4 = torch.randn(T * 32, 4, generator=g)
        case.grad4_mode = mode
        case.dsdf_out = bool(mode & 2)
    return case


def flow_partial_sources(extra, make, ck):
    """Sources with a gap, together with what widens the launch to every tile: dsdf_extra, dsdf_out, grad4 modes 0-3
    (bit 0: out-of-grid corners dropped; bit 1: the sample's own SDF-value gradient as the value component).  A tile no
    source covers contributes its dsdf_extra / grad4 terms only."""
    case = partial_sources_case(extra)
    ck.exact("census", case.launch_range() == (0, case.tiles_all), f"abi/{extra}: launch range")
    run(f"abi/{extra}", case, make(case), dict(fit=2), ck)


def flow_uncovered(make, ck, whats=("dsdf_extra", "grad4", "dsdf_out")):
    """The launch spans every tile (dsdf_extra / grad4 / dsdf_out) but the source covers tiles 0..99 only.  With 2048 waves
    (512 workgroups x 4), wave w takes tile w, then w + 2048: tiles 2048..2147 are uncovered tiles that follow a covered
    tile in the same wave (tiles 100..2047: padding).  They must add their dsdf_extra / grad4 terms and nothing else --
    the stencil rows of feat_bwd_kernel were assigned only for covered tiles."""
    dims = GRIDS["tiny"]
    g = torch.Generator().manual_seed(600)
    case = _base_case(dims, 1, seed=6)
    ro, rd, rr, rs, tiles = ray_records(case, [("axis", 110)], g)
    ro2, rd2, rr2, rs2, tiles2 = ray_records(case, [("pieces", 900)], g)
    n1 = 100
    assert tiles >= n1 and tiles2 >= 100
    T = 2048 + 100
    rec_ray = torch.full((T * 32,), -1, dtype=torch.int32)
    rec_step = torch.zeros(T * 32, dtype=torch.int32)
    rec_ray[:n1 * 32], rec_step[:n1 * 32] = rr[:n1 * 32], rs[:n1 * 32]
    rr2 = torch.where(rr2 >= 0, rr2 + ro.shape[0], rr2)
    rec_ray[2048 * 32:], rec_step[2048 * 32:] = rr2[:100 * 32], rs2[:100 * 32]
    case.rays_o, case.rays_d = torch.cat([ro, ro2]), torch.cat([rd, rd2])
    case.rec_ray, case.rec_step, case.tiles_all = rec_ray, rec_step, T
    case.rec_sdf = torch.randn(T * 32, generator=g)
    case.srcs = [R.Src(_dX(T, g) * 10, 0, n1, on=True, off=True)]
    be = make(case)
    X, gn = be.fwd()
    for what in ("dsdf_extra", "grad4", "dsdf_out"):
        case.dsdf_extra = case.grad4 = None
        case.dsdf_out = False
        if what in ("dsdf_extra", "dsdf_out"):
            case.dsdf_extra = torch.randn(T * 32, generator=g)
            case.dsdf_out = what == "dsdf_out"
        else:
            case.grad4 = torch.randn(T * 32, 4, generator=g)
        if what not in whats:
            continue
        ck.exact("census", case.launch_range() == (0, T), f"uncovered/{what}: launch range")
        run(f"uncovered/{what}", case, be, dict(), ck, X, gn)


def flow_one_tile(make, ck):
    """A launch of a single tile (record mode, a partial tile)."""
    dims = GRIDS["odd"]
    g = torch.Generator().manual_seed(700)
    case = _base_case(dims, 1, seed=7)
    ro, rd, rr, rs, tiles = ray_records(case, [("diag", 1)], g)
    case.rays_o, case.rays_d, case.rec_ray, case.rec_step = ro, rd, rr[:32].clone(), rs[:32].clone()
    case.rec_ray[27:] = -1
    case.rec_sdf = torch.randn(32, generator=g)
    case.srcs = [R.Src(_dX(1, g), 0, 1, on=False, off=True)]
    be = make(case)
    check_forward("one tile", case, be, None, ck)
    check_x16("one tile", case, be, ck)
    run("one tile", case, be, dict(), ck)


# ---- the small cases: flat, groups, faces -----------------------------------------------------------------------------
def flat_case(grid):
    """A block of the SDF grid at exactly 0 (bit-equal nodes: every tap and |g| are exactly 0 inside it) beside a block of
    nodes of magnitude ~1e-16 (0 < |g| <= 1e-12) inside the random grid: 8-sample runs inside each block, across the two
    and across the blocks' outer edges; dX has non-zero normal rows everywhere.  Both kinds of lane take the backward's
    |g| <= 1e-12 branch (feat.hip: `big ? ... : d0` with inv = 1e12f)."""
    dims = GRIDS[grid]
    g = torch.Generator().manual_seed(900 + len(grid))
    case = _base_case(dims, 1, seed=9)
    z0, z1 = 2, dims[2] - 2
    case.sdf[4:16, 6:30, z0:z1] = 0.0
    case.sdf[16:28, 6:30, z0:z1] = torch.randn(12, 24, z1 - z0, generator=g) * 1e-16
    dm = torch.tensor(dims)
    pts = []
    for i in range(24):
        # x of the run's centre: inside the zero block, across zero / tiny, inside tiny, across the outer edges
        cx = (7.0, 10.0, 13.0, 16.0, 19.0, 22.0, 25.0, 28.0, 4.0, 3.0, 29.5, 16.2)[i % 12] + 0.37 * float(torch.rand(1, generator=g))
        c = torch.tensor([cx, 9.0 + 18.0 * float(torch.rand(1, generator=g)), z0 + 2.5 + (z1 - z0 - 5.0) * float(torch.rand(1, generator=g))])
        d = torch.nn.functional.normalize(torch.randn(3, generator=g), dim=0) * 0.5
        if i % 3 == 0:
            d = torch.tensor([0.5, 0.0, 0.0])
        pts += [c + d * (q - 3.5) for q in range(8)]
    idx = torch.minimum(torch.stack(pts).float().clamp_min(0.0), (dm - 1).float())
    tiles = _set_points(case, _to_world(case, idx), g)
    case.tiles_on = tiles // 2
    case.srcs = [R.Src(_dX(tiles, g), 0, tiles, on=True, off=True)]
    return case


def flow_flat(grid, make, ck):
    case = flat_case(grid)
    be = make(case)
    X, gn = check_forward(f"{grid}/flat", case, be, None, ck)
    _, valid = R.positions(case)
    gv = gn.permute(0, 2, 1).reshape(-1, 4)[valid]
    ck.exact("census", int((gv == 0).any(1).sum()) >= 8 and int(((gv > 0) & (gv <= 1e-12)).any(1).sum()) >= 8
             and int((gv > 1e-12).all(1).sum()) >= 8,
             f"{grid}/flat: lanes with |g| == 0: {int((gv == 0).any(1).sum())}, with 0 < |g| <= 1e-12: "
             f"{int(((gv > 0) & (gv <= 1e-12)).any(1).sum())}, above: {int((gv > 1e-12).all(1).sum())}; each needs >= 8")
    run(f"{grid}/flat", case, be, NEED_FLAT, ck, X, gn)


def groups_case(grid):
    """All three colour groups on on-tiles, groups 0 and 1 on the other tiles (group 2 absent), a grid of its own each."""
    dims = GRIDS[grid]
    g = torch.Generator().manual_seed(1000 + len(grid))
    case = _base_case(dims, 1, seed=10)
    mk = lambda: torch.randn(*dims, 6, generator=g) * 0.3
    case.color_on1, case.color_on2, case.color_off1 = mk(), mk(), mk()
    idx = point_runs(case, [("scatter", 2), ("outside", 1), ("runs", 1)], g)
    tiles = _set_points(case, _to_world(case, idx), g)
    case.tiles_on = tiles // 2
    dX = _dX(tiles, g)
    _zero_far_stencil_rows(case, [dX])
    case.srcs = [R.Src(dX, 0, tiles, on=True, off=True)]
    return case


def flow_groups(grid, make, ck):
    case = groups_case(grid)
    be = make(case)
    check_forward(f"{grid}/groups", case, be, None, ck)
    check_x16(f"{grid}/groups", case, be, ck)


def face_tol(case, axis, n):
    d = case.dims[axis]
    lo, hi = float(case.lo[axis]), float(case.hi[axis])
    pw = lo + n / (d - 1) * (hi - lo)
    step = max(float(np.spacing(np.float32(abs(pw)))), float(np.spacing(np.float32(1.0))) * (hi - lo) / 2) * (d - 1) / (hi - lo)
    return max(2 * float(np.spacing(np.float32(max(n, 1)))), 2 * step)


def faces_points(case):
    """World points whose replayed grid index is exactly 0, exactly dims - 1, or as near an integer from 0 to 3 and
    dims - 4 to dims - 1 along one axis as a binary32 world point gets (the other two coordinates: inside the box, off the
    integers): within FACE_TOL(n) of it, on both sides.  Near the low face a world coordinate's own spacing, times
    (dims - 1) / extent, is coarser than the index's ulp (and 2u - 1 near -1 quantises u once more), so "within 2 ulp of the
    index" is reachable only where the position's resolution allows it: the tolerance is the larger of 2 ulp of the index
    and 2 steps of the position, in index units."""
    dims = case.dims
    g = torch.Generator().manual_seed(1100 + dims[0])
    out = [case.lo[None].clone(), case.hi[None].clone()]
    for axis in range(3):
        d = dims[axis]
        for n in sorted(set([0, 1, 2, 3, d - 4, d - 3, d - 2, d - 1])):
            base = torch.tensor([1.3, 1.3, 1.3]) + torch.rand(3, generator=g) * (torch.tensor(dims) - 3.6)
            base[axis] = float(n)
            p0 = _to_world(case, base[None])[0]
            if n == 0:
                p0[axis] = case.lo[axis]
            if n == d - 1:
                p0[axis] = case.hi[axis]
            cand = []
            for k in range(-40, 41):
                p = p0.clone()
                q = p[axis].clone()
                for _ in range(abs(k)):
                    q = torch.nextafter(q, torch.tensor(float("inf") if k > 0 else -float("inf")))
                p[axis] = q
                cand.append(p)
            cand = torch.stack(cand)
            cand = cand[(cand[:, axis] >= case.lo[axis]) & (cand[:, axis] <= case.hi[axis])]
            ix = R.world_to_index(case, cand)[:, axis].double()
            near = (ix - n).abs() <= face_tol(case, axis, n)
            # one point per distinct index value
            _, first = np.unique(ix[near].numpy(), return_index=True)
            out.append(cand[near][torch.from_numpy(first)])
    return torch.cat(out)


def faces_case(grid):
    """Samples on and within 2 ulp of the grid's faces and of the first and last four integer indices per axis, default radii:
    where the bar's reach (7 cells) and the single rounding of the hat weights' t = ixA - (iA - 2) act."""
    dims = GRIDS[grid]
    g = torch.Generator().manual_seed(1200 + len(grid))
    case = _base_case(dims, 1, seed=11)
    tiles = _set_points(case, faces_points(case), g)
    case.tiles_on = tiles // 2
    case.srcs = [R.Src(_dX(tiles, g), 0, tiles, on=True, off=True)]
    return case


def check_faces_indices(tag, case, ck):
    p, valid = R.positions(case)
    ind = R.world_to_index(case, p[valid]).double()
    top = torch.tensor([d - 1 for d in case.dims], dtype=torch.float64)
    ck.exact("census", bool((ind == 0).any(0).all()) and bool((ind == top).any(0).all()),
             f"{tag}: no sample at index exactly 0 / dims - 1 on every axis")
    for axis in range(3):
        d = case.dims[axis]
        for n in (0, 1, 2, 3, d - 4, d - 3, d - 2, d - 1):
            x = ind[:, axis]
            near = (x - n).abs() <= face_tol(case, axis, n)
            ck.exact("census", bool((near & (x < n)).any() or n == 0) and bool((near & (x > n)).any() or n == d - 1),
                     f"{tag}: axis {axis}: no samples just below and just above index {n}")


def flow_faces(grid, make, ck):
    case = faces_case(grid)
    check_faces_indices(f"{grid}/faces", case, ck)
    be = make(case)
    X, gn = check_forward(f"{grid}/faces", case, be, None, ck)
    run(f"{grid}/faces", case, be, dict(clip_lo=1, clip_hi=1), ck, X, gn)
