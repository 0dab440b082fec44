"""esr_fine_feat_bwd / esr_fine_feat_fwd (csrc/feat.hip) cell by cell against the float64 restatement in feat_ref64.py, with
a census of the backward's window paths that every case asserts.

Per-cell bound: |gpu - ref| <= K * 2^-24 * absref + FLOOR for every touched cell (absref: the scatter evaluated on
magnitudes, feat_ref64's docstring), and every untouched cell exactly 0.  K covers, per term:
  - the binary32 products of a term's weights and gradient rows, and the bar's fma sums of up to 9 taps onto a cell;
  - the window's double sum rounded to binary32 once, then one fp32 atomic per flush, or per term on the fallback path;
  - v_rcp_f32 (1 ulp) for 1/|g|, 1/(cp - cm + 1e-12) and 1/voxel, and the grad4 scale (float)(dims - 1) / extent;
  - the documented <= 2 ulp `ixm = cm` shortcut and the bar's hat weights, formed from t = ixA - (iA - 2) in binary32
    (rounded once near the low faces): positions, which feat_ref64 replays bit for bit, so they cost nothing here.
The normals and |g| are read from the forward's binary32 tile, as the kernel reads them (they are ABI inputs).
Measured worst ratios |gpu - ref| / (2^-24 absref) are printed per grid (-s)."""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

import feat_ref64 as R

pytestmark = pytest.mark.gpu

K_BWD = 8                       # backward cells (measured worst on the MI355X: 3.3)
K_FWD = 8                       # forward rows (normals: through the first-order scale, feat_ref64.forward_rows; measured: 4.7)
FLOOR = 1e-30
DEV = "cuda"
DEFAULT_RADII = (0.5, 1.0, 1.5, 2.0)
DIRECT_RADII = (0.5, 1.0, 1.5, 2.5)        # a radius beyond the bars' reach: esr_fine_feat_fwd runs the direct form
GRIDS = {"tiny": (64, 64, 16), "odd": (37, 61, 23), "c2": (256, 256, 64), "g256": (256, 256, 256)}
VOX = 1.0 / 64


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


# ---- running the kernels ----------------------------------------------------------------------------------------------
def _scene(case):
    from esr_nerf_amd.fine_engine import make_scene
    return make_scene(case.lo.tolist(), case.hi.tolist(), case.lo.tolist(), case.hi.tolist(), list(case.dims), [32, 32, 32],
                      case.near, case.stepdist, case.vox, 0.0, 1e-3, 1e-4, 40.0, list(case.grad_feat))


class Gpu:
    """Device copies of a case's inputs (kept alive across the async launches)."""

    def __init__(self, case):
        from esr_nerf_amd import _lib
        self.case, self.L = case, _lib.lib()
        d = lambda t: None if t is None else t.contiguous().to(DEV)
        fa = _lib.EsrFeatArgs()
        self.keep = []
        k = lambda t: (self.keep.append(d(t)), self.keep[-1])[1]
        n = case.tiles_all * 32
        if case.pts is not None:
            fa.pts, fa.pt_viewdirs, fa.pt_sdf = k(case.pts).data_ptr(), k(torch.zeros_like(case.pts)).data_ptr(), \
                k(case.pt_sdf).data_ptr()
            fa.n_pts = case.n_pts
        else:
            fa.rays_o, fa.rays_d = k(case.rays_o).data_ptr(), k(case.rays_d).data_ptr()
            fa.viewdirs = k(torch.nn.functional.normalize(case.rays_d, dim=-1)).data_ptr()
            fa.rec_ray, fa.rec_step, fa.rec_sdf = k(case.rec_ray).data_ptr(), k(case.rec_step).data_ptr(), \
                k(case.rec_sdf).data_ptr()
        fa.sdf = k(case.sdf).data_ptr()
        fa.color_on[0] = k(case.color_on).data_ptr()
        fa.color_off[0] = k(case.color_off).data_ptr()
        fa.tiles_on, fa.tiles_all = case.tiles_on, case.tiles_all
        self.fa, self.n = fa, n
        self.s = _lib.stream_ptr("cuda:0")

    def fwd(self, radii=None):
        from esr_nerf_amd import _lib
        case = self.case
        sc = _scene(case) if radii is None else _scene(SimpleNamespace(**{**case.__dict__, "grad_feat": radii}))
        X = torch.zeros(case.tiles_all * 104 * 32, device=DEV)
        gn = torch.zeros(case.tiles_all * 4 * 32, device=DEV)
        _lib.check(self.L.esr_fine_feat_fwd(C.byref(sc), C.byref(self.fa), _lib.ptr(X), _lib.ptr(gn), self.s), "feat_fwd")
        return X.view(case.tiles_all, 104, 32), gn.view(case.tiles_all, 4, 32)

    def bwd(self, X, gn):
        from esr_nerf_amd import _lib
        case = self.case
        dims = case.dims
        ncell = dims[0] * dims[1] * dims[2]
        out = {}
        src = (_lib.EsrFeatBwdSrc * len(case.srcs))()
        for i, s in enumerate(case.srcs):
            dX = s.dX.contiguous().to(DEV)
            self.keep.append(dX)
            src[i].dX, src[i].t0, src[i].t1 = dX.data_ptr(), s.t0, s.t1
            if s.on:
                out[R.colour_gid(i, True)] = torch.zeros(ncell * 6, device=DEV)
                src[i].grad_color_on = out[R.colour_gid(i, True)].data_ptr()
            if s.off:
                out[R.colour_gid(i, False)] = torch.zeros(ncell * 6, device=DEV)
                src[i].grad_color_off = out[R.colour_gid(i, False)].data_ptr()
        if case.grad_sdf:
            out[R.SDF_GID] = torch.zeros(ncell, device=DEV)
        extra = None if case.dsdf_extra is None else case.dsdf_extra.contiguous().to(DEV)
        g4 = None if case.grad4 is None else case.grad4.contiguous().to(DEV)
        dsdf = torch.full((self.n,), 12345.0, device=DEV) if case.dsdf_out else None
        self.keep += [extra, g4]
        _lib.check(self.L.esr_fine_feat_bwd(C.byref(_scene(case)), C.byref(self.fa), _lib.ptr(X.view(-1)),
                                            _lib.ptr(gn.view(-1)), src, len(case.srcs), _lib.ptr(extra),
                                            _lib.ptr(out.get(R.SDF_GID)), _lib.ptr(dsdf), _lib.ptr(g4), case.grad4_mode,
                                            self.s), "feat_bwd")
        torch.cuda.synchronize()
        return out, dsdf


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


def check_grids(tag, case, ref, out, census_tiles, dsdf=None):
    """Every touched cell within the bound, every other cell exactly 0, dsdf_out per lane exactly."""
    tb, _ = case.launch_range()
    worst = {}
    for gid, buf in out.items():
        if gid not in ref.cells:                              # nothing reaches this grid
            assert int((buf != 0).sum()) == 0, f"{tag}: grid {gid} should be untouched"
            continue
        u, v, a = ref.cells[gid]
        got = buf[u.to(DEV)].double().cpu()
        err = (got - v).abs()
        bound = K_BWD * 2.0 ** -24 * a + FLOOR
        ratio = err / (2.0 ** -24 * a + FLOOR)
        worst[gid] = float(ratio.max()) if ratio.numel() else 0.0
        nz_all, nz_touched = int((buf != 0).sum()), int((got != 0).sum())
        bad = err > bound
        if bool(bad.any()) or nz_all != nz_touched:
            if bool(bad.any()):
                i = int((err / bound).argmax())
            else:                                            # a non-zero cell outside the touched set
                extra = torch.nonzero(buf.cpu() != 0)[:, 0]
                mask = ~torch.isin(extra, u)
                i = None
                f0 = int(extra[mask][0])
            fl = int(u[i]) if i is not None else f0
            tf, tv, ta, tt = ref.terms[gid]
            tiles = sorted(set(tt[tf == fl].tolist()))[:6]
            info = [(t, census_tiles[t - tb]["classes"] if census_tiles[t - tb] else None) for t in tiles]
            what = (f"|gpu - ref| = {float(err[i]):.3e} > bound {float(bound[i]):.3e} (gpu {float(got[i]):.9e}, ref "
                    f"{float(v[i]):.9e}, absref {float(a[i]):.3e})") if i is not None else \
                f"non-zero ({float(buf[fl]):.3e}) but no term reaches it ({nz_all} non-zero, {nz_touched} touched)"
            pytest.fail(f"{tag}: {_cell_name(case, gid, fl)}: {what}; tiles / path classes: {info}")
    if case.dsdf_out:
        want, jj = ref.dsdf_out
        got = dsdf.cpu()
        assert torch.equal(got[jj], want), f"{tag}: dsdf_out differs in {int((got[jj] != want).sum())} lanes"
        untouched = torch.ones(got.numel(), dtype=torch.bool)
        untouched[jj] = False
        assert bool((got[untouched] == 12345.0).all()), f"{tag}: dsdf_out written outside the valid lanes"
    print(f"{tag}: worst |gpu - ref| / (2^-24 absref) per grid: " + ", ".join(f"{k}: {v:.2f}" for k, v in worst.items()))
    return worst


def check_forward(tag, case, gpu, radii):
    X, gn = gpu.fwd(radii)
    c = case if radii is None else R.Case(**{**case.__dict__, "grad_feat": radii})
    p, valid = R.positions(c)
    val, scl, nrm, nabs = R.forward_rows(c, p, valid)
    jj = torch.nonzero(valid)[:, 0]
    Xc = X.cpu()
    got = Xc[jj // 32, :43, jj % 32].double()
    err = (got - val).abs()
    bound = K_FWD * 2.0 ** -24 * scl + FLOOR
    bad = err > bound
    if bool(bad.any()):
        i = int((err / bound).flatten().argmax())
        m, r = divmod(i, 43)
        pytest.fail(f"{tag}: forward row {r} of sample {int(jj[m])} (tile {int(jj[m]) // 32}): gpu {float(got[m, r]):.9e}, "
                    f"ref {float(val[m, r]):.9e}, scale {float(scl[m, r]):.3e}")
    gg = gn.cpu()[jj // 32, :, jj % 32].double()
    assert bool(((gg - nrm).abs() <= K_FWD * 2.0 ** -24 * nabs + FLOOR).all()), f"{tag}: gnorm"
    ratio = float((err / (2.0 ** -24 * scl + FLOOR)).max())
    print(f"{tag}: forward worst |gpu - ref| / (2^-24 scale): {ratio:.2f}")
    return X, gn


def _dX(tiles, g):
    dX = torch.randn(tiles, 64, 32, generator=g)
    dX[:, 43:] = 0.0
    return dX


def _census(tag, case, need):
    tiles, counts = R.census(case)
    print(f"{tag}: census {counts}")
    for cls, n in need.items():
        assert counts[cls] >= n, f"{tag}: path class {cls}: {counts[cls]} tiles, this case needs >= {n} ({counts})"
    return tiles


def _run(tag, case, need, out_gpu=None):
    gpu = out_gpu or Gpu(case)
    X, gn = gpu.fwd()
    tiles = _census(tag, case, need)
    out, dsdf = gpu.bwd(X, gn)
    ref = R.scatter(case, X.cpu(), gn.cpu())
    check_grids(tag, case, ref, out, tiles, dsdf)
    return gpu, X, gn


def _check_sampler(case, gpu):
    """the replayed positions are esr_sample_points', bit for bit"""
    from esr_nerf_amd import _lib
    p, valid = R.positions(case)
    n = case.tiles_all * 32
    pd = torch.zeros(n, 3, device=DEV)
    ro, rd, rr, rs = (t.contiguous().to(DEV) for t in (case.rays_o, case.rays_d, case.rec_ray, case.rec_step))
    _lib.check(gpu.L.esr_sample_points(C.byref(_scene(case)), _lib.ptr(ro), _lib.ptr(rd), _lib.ptr(rr), _lib.ptr(rs), n,
                                       _lib.ptr(pd), gpu.s), "sample_points")
    assert torch.equal(pd.cpu()[valid], p[valid])


# ---- cases ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", ["tiny", "odd", "c2"])
def test_record_mode_scatter(grid):
    """Axis-parallel, (1,1,1)-diagonal, face-grazing, short-piece (padding lanes mid-tile) and corner tiles, partial last
    tile; on/off colour grids split by tiles_on; then the same tiles as a colour-only launch (grad_sdf NULL)."""
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
    gpu = Gpu(case)
    _check_sampler(case, gpu)
    check_forward(f"{grid}/rays bar", case, gpu, None)
    check_forward(f"{grid}/rays direct", case, gpu, DIRECT_RADII)
    _run(f"{grid}/rays", case, dict(fit=8, cut8_fit=4, cut8_global=2, mixed=2, clip_lo=4, clip_hi=4), gpu)
    case.grad_sdf = False
    # (colour windows have no margin below the base cells: they clip at dims - 1 only)
    _run(f"{grid}/rays colour-only", case, dict(colour_only=20, fit=8, cut8_fit=4, clip_hi=2), gpu)


@pytest.mark.parametrize("grid", ["tiny", "odd", "c2"])
def test_explicit_points_scatter(grid):
    """Ray-ordered runs with jumps of 3 cells (one window) and 4 cells (cut), scattered singletons (32 windows, most on
    global atomics), points up to 1 voxel outside the box; dsdf_out, the SDF value as an input."""
    dims = GRIDS[grid]
    g = torch.Generator().manual_seed(200 + len(grid))
    case = _base_case(dims, 1, seed=2)
    pts = _to_world(case, point_runs(case, [("jumps", 8), ("scatter", 6), ("outside", 4)], g))
    n = pts.shape[0]
    tiles = (n + 31) // 32
    case.pts, case.pt_sdf, case.tiles_all = pts, torch.randn(n, generator=g), tiles
    case.tiles_on = tiles // 2
    dX = _dX(tiles, g)
    # stencil rows of points more than half a voxel outside: their +-0.5 taps clamp onto each other, where the
    # difference quotient is 0 / 1e-12 (the reference's own gradient is noise there); colour and value rows stay
    far = ~_inside(case, pts, 0.5 * case.vox * 0.999)
    jf = torch.nonzero(far)[:, 0]
    dX[jf // 32, 7:43, jf % 32] = 0.0
    case.srcs = [R.Src(dX, 0, tiles, on=True, off=True)]
    case.dsdf_out = True
    gpu = Gpu(case)
    check_forward(f"{grid}/points bar", case, gpu, None)
    check_forward(f"{grid}/points direct", case, gpu, DIRECT_RADII)
    _run(f"{grid}/points", case, dict(fit=4, cut8_global=4, mixed=4, clip_lo=2, clip_hi=2), gpu)


def test_production_grid_scatter():
    """The 256^3 grid (~10^8 colour floats): 8-sample runs over the whole box up to its last cell, so window origins and
    flush indices reach the largest values the product uses; touched cells compared, the rest must stay 0."""
    dims = GRIDS["g256"]
    g = torch.Generator().manual_seed(300)
    case = _base_case(dims, 1, seed=3)
    idx = point_runs(case, [("runs", 60), ("scatter", 4)], g)
    pts = _to_world(case, idx)
    n = pts.shape[0]
    tiles = (n + 31) // 32
    case.pts, case.pt_sdf, case.tiles_all = pts, torch.randn(n, generator=g), tiles
    case.srcs = [R.Src(_dX(tiles, g), 0, tiles, on=False, off=True)]
    case.dsdf_out = True
    gpu = Gpu(case)
    check_forward("g256/points bar", case, gpu, None)
    _run("g256/points", case, dict(fit=30, clip_hi=1, cut8_global=2))


def _abi_case(seed):
    dims = GRIDS["odd"]
    g = torch.Generator().manual_seed(seed)
    case = _base_case(dims, 1, seed=seed)
    idx = point_runs(case, [("jumps", 10), ("scatter", 4), ("runs", 10)], g)
    pts = _to_world(case, idx)
    n = pts.shape[0]
    tiles = (n + 31) // 32
    case.pts, case.pt_sdf, case.tiles_all = pts, torch.randn(n, generator=g), tiles
    return case, g, tiles


def test_multi_source_and_on_off_grids():
    """n_src 2 and 3: dX rows 6-42 summed over the sources covering a tile, colour rows to each source's own grid;
    tiles_on routes a tile's colour to grad_color_on / _off, NULL for one of them; sources over part of the tiles."""
    case, g, T = _abi_case(400)
    case.tiles_on = T // 3
    case.srcs = [R.Src(_dX(T, g), 0, T, on=True, off=True), R.Src(_dX(T, g), 0, T // 2, on=False, off=True),
                 R.Src(_dX(T, g), T // 4, 3 * T // 4, on=True, off=False)]
    gpu = Gpu(case)
    _run("abi/3 sources", case, dict(fit=4, cut8_global=1), gpu)
    case.srcs = case.srcs[:2]
    case.srcs[1] = R.Src(case.srcs[1].dX, T // 5, T, on=True, off=False)
    _run("abi/2 sources", case, dict(fit=4), gpu)
    # a source over part of the tiles: the launch covers its range only
    case.srcs = [R.Src(_dX(T, g), T // 4, T // 2, on=True, off=True)]
    assert case.launch_range() == (T // 4, T // 2)
    _run("abi/partial source", case, dict(fit=2), gpu)


@pytest.mark.parametrize("extra", ["gap+dsdf_extra", "dsdf_out", "grad4-0", "grad4-1", "grad4-2", "grad4-3"])
def test_partial_sources_with_whole_launch_terms(extra):
    """Sources with a gap, together with what widens the launch to every tile: dsdf_extra, dsdf_out, grad4 modes 0-3
    (bit 0: out-of-grid corners dropped; bit 1: the sample's own SDF-value gradient as the value component).  A tile no
    source covers contributes its dsdf_extra / grad4 terms only."""
    case, g, T = _abi_case(500)
    # points up to a voxel outside the box, for the border-replicated / dropped corners of grad4 (stencil rows zeroed)
    out_idx = point_runs(case, [("outside", 2)], g)
    case.pts = torch.cat([case.pts, _to_world(case, out_idx)])
    case.pt_sdf = torch.randn(case.pts.shape[0], generator=g)
    T = case.tiles_all = (case.pts.shape[0] + 31) // 32
    dX0, dX1 = _dX(T, g), _dX(T, g)
    far = ~_inside(case, case.pts, 0.5 * case.vox * 0.999)
    jf = torch.nonzero(far)[:, 0]
    for d in (dX0, dX1):
        d[jf // 32, 7:43, jf % 32] = 0.0
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
    assert case.launch_range() == (0, T)
    _run(f"abi/{extra}", case, dict(fit=2))


def test_uncovered_tiles_after_covered_tiles_in_one_wave():
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
    gpu = Gpu(case)
    X, gn = gpu.fwd()
    for what in ("dsdf_extra", "grad4", "dsdf_out"):
        case.dsdf_extra = case.grad4 = None
        case.dsdf_out = False
        if what in ("dsdf_extra", "dsdf_out"):
            case.dsdf_extra = torch.randn(T * 32, generator=g)
            case.dsdf_out = what == "dsdf_out"
        else:
            case.grad4 = torch.randn(T * 32, 4, generator=g)
        assert case.launch_range() == (0, T)
        out, dsdf = gpu.bwd(X, gn)
        ref = R.scatter(case, X.cpu(), gn.cpu())
        tiles_info, _ = R.census(case)
        check_grids(f"uncovered/{what}", case, ref, out, tiles_info, dsdf)


def test_tiles_all_one():
    """A launch of a single tile (record mode, a partial tile)."""
    dims = GRIDS["odd"]
    g = torch.Generator().manual_seed(700)
    case = _base_case(dims, 1, seed=7)
    ro, rd, rr, rs, tiles = ray_records(case, [("diag", 1)], g)
    case.rays_o, case.rays_d, case.rec_ray, case.rec_step = ro, rd, rr[:32].clone(), rs[:32].clone()
    case.rec_ray[27:] = -1
    case.rec_sdf = torch.randn(32, generator=g)
    case.srcs = [R.Src(_dX(1, g), 0, 1, on=False, off=True)]
    gpu = Gpu(case)
    check_forward("one tile", case, gpu, None)
    _run("one tile", case, dict())


def test_restatement_matches_autograd_in_float64():
    """feat_ref64's scatter against torch autograd through oracle/fine_path.py's stencil and grid_sample in float64 (and the
    exact interpolant's value and gradient for grad4), on a small grid with interior points: <= 1e-12 relative."""
    from oracle import fine_path as fp
    torch.manual_seed(0)
    dims = (9, 12, 7)
    g = torch.Generator().manual_seed(800)
    case = _base_case(dims, 2, seed=8)
    lo, hi = case.lo.double(), case.hi.double()
    n = 50
    idx = 2.1 + torch.rand(n, 3, generator=g, dtype=torch.float64) * (torch.tensor(dims) - 5.2)
    pts = _to_world(case, idx)
    sdf = case.sdf.double()[None, None].clone().requires_grad_(True)
    col = case.color_off.double().permute(3, 0, 1, 2)[None].clone().requires_grad_(True)
    c = SimpleNamespace(xyz_min=lo, xyz_max=hi, voxel_size=case.vox)
    radii = torch.tensor(case.grad_feat, dtype=torch.float64)
    p64 = pts.double().requires_grad_(True)
    feat, grad, nrm = fp.sdf_stencil(c, sdf, p64, radii, diff_eps=1e-12)
    norm = fp.to_norm(p64, lo, hi)
    colv = fp.sample_grid(col, norm)
    val = fp.trilinear_explicit(sdf, norm)[:, 0]            # (grid_sample has no double backward)
    (dval,) = torch.autograd.grad(val.sum(), p64, create_graph=True)
    dX = torch.randn(n, 43, generator=g, dtype=torch.float64)
    g4 = torch.randn(n, 4, generator=g, dtype=torch.float64)
    L = (colv * dX[:, :6]).sum() + (val * dX[:, 6]).sum() + (feat * dX[:, 7:31]).sum() + (nrm * dX[:, 31:43]).sum() \
        + (val * g4[:, 0]).sum() + (dval * g4[:, 1:]).sum()
    gs, gc = torch.autograd.grad(L, [sdf, col])
    # the same inputs for the restatement, in float64 throughout (the index too)
    T = case.tiles_all
    case.pts, case.pt_sdf = pts, torch.zeros(n)
    dXt = torch.zeros(T * 32, 64, dtype=torch.float64)
    dXt[:n, :43] = dX
    case.srcs = [R.Src(dXt.view(T, 32, 64).permute(0, 2, 1), 0, T, on=False, off=True)]
    case.grad4 = torch.zeros(T * 32, 4, dtype=torch.float64)
    case.grad4[:n] = g4
    X = torch.zeros(T * 32, 104, dtype=torch.float64)
    gn = torch.zeros(T * 32, 4, dtype=torch.float64)
    X[:n, 31:43] = nrm.detach()
    gn[:n] = grad.detach().view(n, 3, 4).norm(dim=1)
    p, valid = R.positions(case)
    ind64 = torch.zeros(T * 32, 3, dtype=torch.float64)
    ind64[:n] = ((fp.to_norm(pts.double(), lo, hi).flip(-1) + 1) / 2) * torch.tensor([d - 1 for d in dims], dtype=torch.float64)
    ref = R.scatter(case, X.view(T, 32, 104).permute(0, 2, 1), gn.view(T, 32, 4).permute(0, 2, 1), p, valid, ind64)
    ncell = dims[0] * dims[1] * dims[2]
    mine = torch.zeros(ncell, dtype=torch.float64)
    u, v, _ = ref.cells[R.SDF_GID]
    mine[u] = v
    want = gs[0, 0].reshape(-1)
    assert float((mine - want).abs().max() / want.abs().max()) <= 1e-12
    mc = torch.zeros(ncell * 6, dtype=torch.float64)
    u, v, _ = ref.cells[R.colour_gid(0, False)]
    mc[u] = v
    wc = gc[0].permute(1, 2, 3, 0).reshape(-1)
    assert float((mc - wc).abs().max() / wc.abs().max()) <= 1e-12
