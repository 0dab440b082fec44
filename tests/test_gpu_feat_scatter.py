"""esr_fine_feat_fwd / esr_fine_feat_fwd_x16 / esr_fine_feat_bwd (csrc/feat.hip) value by value and cell by cell against the
float64 restatement in feat_ref64.py, with a census of the backward's window paths that every case asserts.  This file holds
the `Gpu` backend (the ctypes launches) and the assertions; the cases, the census requirements and the comparison are
feat_check.py's, which tests/test_feat_ref64_host.py runs without a device on the binary32 emulation feat_emu.py and its mutants.

Per-cell bound: |gpu - ref| <= K * 2^-24 * absref + FLOOR for every touched cell (absref: the scatter evaluated on
magnitudes, feat_ref64's docstring), and every untouched cell exactly 0; K = feat_ref64.K_FAMILY[family].  K covers, per term:
  - the binary32 products of a term's weights and gradient rows, and the bar's fma sums of up to 9 taps onto a cell;
  - the window's double sum rounded to binary32 once, then one fp32 atomic per flush (`sdf fit`), or one fp32 atomic per term on
    the fallback path (`sdf global`) -- the two rounding models, and grad4's four-term sum a third family (`sdf grad4`);
  - v_rcp_f32 (1 ulp) for 1/|g|, 1/(cp - cm + 1e-12) and 1/voxel, and the grad4 scale (float)(dims - 1) / extent;
  - the documented <= 2 ulp `ixm = cm` shortcut and the bar's hat weights, formed from t = ixA - (iA - 2) in binary32
    (rounded once near the low faces): positions, which feat_ref64 replays bit for bit, so they cost nothing here.
The normals and |g| are read from the forward's binary32 tile, as the kernel reads them (they are ABI inputs).
Forward: all 104 rows, padding lanes and the bf16 row-quad tile (feat_check's families).  Measured worst ratios
|gpu - ref| / (2^-24 absref) are printed per family (-s)."""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

import feat_check as F
import feat_ref64 as R
from feat_check import _base_case, _to_world

pytestmark = pytest.mark.gpu

DEV = "cuda"


# ---- running the kernels ----------------------------------------------------------------------------------------------
def _scene(case):
    from esr_nerf_amd.fine_engine import make_scene
    return make_scene(case.lo.tolist(), case.hi.tolist(), case.lo.tolist(), case.hi.tolist(), list(case.dims), [32, 32, 32],
                      case.near, case.stepdist, case.vox, 0.0, 1e-3, 1e-4, 40.0, list(case.grad_feat))


class Gpu:
    """Device copies of a case's inputs (kept alive across the async launches); feat_check's backend on the kernels."""

    def __init__(self, case):
        from esr_nerf_amd import _lib
        self.case, self.L = case, _lib.lib()
        d = lambda t: None if t is None else t.contiguous().to(DEV)
        fa = _lib.EsrFeatArgs()
        self.keep = []
        k = lambda t: (self.keep.append(d(t)), self.keep[-1])[1]
        n = case.tiles_all * 32
        if case.pts is not None:
            fa.pts, fa.pt_viewdirs, fa.pt_sdf = k(case.pts).data_ptr(), k(case.view_inputs()[:case.n_pts]).data_ptr(), \
                k(case.pt_sdf).data_ptr()
            fa.n_pts = case.n_pts
        else:
            fa.rays_o, fa.rays_d = k(case.rays_o).data_ptr(), k(case.rays_d).data_ptr()
            vd = case.viewdirs if case.viewdirs is not None else torch.nn.functional.normalize(case.rays_d, dim=-1)
            fa.viewdirs = k(vd).data_ptr()
            fa.rec_ray, fa.rec_step, fa.rec_sdf = k(case.rec_ray).data_ptr(), k(case.rec_step).data_ptr(), \
                k(case.rec_sdf).data_ptr()
        fa.sdf = k(case.sdf).data_ptr()
        for gi, (on, off) in enumerate(zip(case.colour_grids(True), case.colour_grids(False))):
            if on is not None:
                fa.color_on[gi] = k(on).data_ptr()
            if off is not None:
                fa.color_off[gi] = k(off).data_ptr()
        fa.tiles_on, fa.tiles_all = case.tiles_on, case.tiles_all
        self.fa, self.n = fa, n
        self.s = _lib.stream_ptr("cuda:0")

    def _scene(self, radii):
        case = self.case
        return _scene(case) if radii is None else _scene(SimpleNamespace(**{**case.__dict__, "grad_feat": radii}))

    def fwd(self, radii=None):
        from esr_nerf_amd import _lib
        case = self.case
        X = torch.full((case.tiles_all * 104 * 32,), 7.0, device=DEV)       # (not zeros: padding lanes must be written)
        gn = torch.full((case.tiles_all * 4 * 32,), 7.0, device=DEV)
        _lib.check(self.L.esr_fine_feat_fwd(C.byref(self._scene(radii)), C.byref(self.fa), _lib.ptr(X), _lib.ptr(gn), self.s),
                   "feat_fwd")
        return X.view(case.tiles_all, 104, 32).cpu(), gn.view(case.tiles_all, 4, 32).cpu()

    def fwd16(self):
        from esr_nerf_amd import _lib
        T = self.case.tiles_all
        assert int(self.L.esr_fine_feat_x16_bytes(T)) == T * 26 * 256
        X16 = torch.full((T * 26 * 256,), 0x7f, dtype=torch.uint8, device=DEV)
        X = torch.full((T * 104 * 32,), float("nan"), device=DEV)
        gn = torch.full((T * 4 * 32,), 7.0, device=DEV)
        _lib.check(self.L.esr_fine_feat_fwd_x16(C.byref(self._scene(None)), C.byref(self.fa), _lib.ptr(X), _lib.ptr(gn),
                                                _lib.ptr(X16), self.s), "feat_fwd_x16")
        return X16.cpu().view(torch.bfloat16).view(T, 26, 32, 4), X.view(T, 104, 32).cpu(), gn.view(T, 4, 32).cpu()

    def bwd(self, X, gn):
        from esr_nerf_amd import _lib
        case = self.case
        dims = case.dims
        ncell = dims[0] * dims[1] * dims[2]
        X, gn = X.contiguous().to(DEV), gn.contiguous().to(DEV)
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
        return {g: v.cpu() for g, v in out.items()}, (None if dsdf is None else dsdf.cpu())


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


def _done(ck):
    for tag, counts in ck.census.items():
        print(f"{tag}: census {counts}")
    print("worst |gpu - ref| / (2^-24 absref) per family: " + ", ".join(f"{k}: {v:.3f}" for k, v in sorted(ck.worst.items())))
    assert not ck.fails, ck.report()


# ---- cases (feat_check's flows) ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", ["tiny", "odd", "c2"])
def test_record_mode_scatter(grid):
    """Axis-parallel, (1,1,1)-diagonal, face-grazing, short-piece (padding lanes mid-tile) and corner tiles, partial last
    tile; on/off colour grids split by tiles_on; then the same tiles as a colour-only launch (grad_sdf NULL).  Forward: bar
    and direct form, all 104 rows, and the bf16 row-quad tile."""
    ck = F.Check()
    F.flow_record_mode(grid, Gpu, ck, sampler=_check_sampler)
    _done(ck)


@pytest.mark.parametrize("grid", ["tiny", "odd", "c2"])
def test_explicit_points_scatter(grid):
    """Ray-ordered runs with jumps of 3 cells (one window) and 4 cells (cut), scattered singletons (32 windows, most on
    global atomics), points up to 1 voxel outside the box; dsdf_out, the SDF value as an input."""
    ck = F.Check()
    F.flow_explicit_points(grid, Gpu, ck)
    _done(ck)


def test_production_grid_scatter():
    """The 256^3 grid (~10^8 colour floats): 8-sample runs over the whole box up to its last cell, so window origins and
    flush indices reach the largest values the product uses; touched cells compared, the rest must stay 0."""
    ck = F.Check()
    F.flow_production(Gpu, ck)
    _done(ck)


def test_multi_source_and_on_off_grids():
    """n_src 2 and 3: dX rows 6-42 summed over the sources covering a tile, colour rows to each source's own grid;
    tiles_on routes a tile's colour to grad_color_on / _off, NULL for one of them; sources over part of the tiles."""
    ck = F.Check()
    F.flow_multi_source(Gpu, ck)
    _done(ck)


@pytest.mark.parametrize("extra", F.PARTIAL_EXTRAS)
def test_partial_sources_with_whole_launch_terms(extra):
    """Sources with a gap, together with what widens the launch to every tile: dsdf_extra, dsdf_out, grad4 modes 0-3
    (bit 0: out-of-grid corners dropped; bit 1: the sample's own SDF-value gradient as the value component).  A tile no
    source covers contributes its dsdf_extra / grad4 terms only."""
    ck = F.Check()
    F.flow_partial_sources(extra, Gpu, ck)
    _done(ck)


def test_uncovered_tiles_after_covered_tiles_in_one_wave():
    """The launch spans every tile (dsdf_extra / grad4 / dsdf_out) but the source covers tiles 0..99 only.  With 2048 waves
    (512 workgroups x 4), wave w takes tile w, then w + 2048: tiles 2048..2147 are uncovered tiles that follow a covered
    tile in the same wave (tiles 100..2047: padding).  They must add their dsdf_extra / grad4 terms and nothing else --
    the stencil rows of feat_bwd_kernel were assigned only for covered tiles."""
    ck = F.Check()
    F.flow_uncovered(Gpu, ck)
    _done(ck)


def test_tiles_all_one():
    """A launch of a single tile (record mode, a partial tile)."""
    ck = F.Check()
    F.flow_one_tile(Gpu, ck)
    _done(ck)


@pytest.mark.parametrize("grid", ["tiny", "odd"])
def test_flat_block_takes_the_small_norm_branch(grid):
    """A block of bit-equal SDF nodes beside a block of ~1e-16 nodes: lanes with |g| == 0 and with 0 < |g| <= 1e-12 take
    the backward's `big ? ... : d0` branch with inv = 1e12f; the census class small_norm is required."""
    ck = F.Check()
    F.flow_flat(grid, Gpu, ck)
    _done(ck)


@pytest.mark.parametrize("grid", ["tiny", "odd"])
def test_three_colour_groups(grid):
    """All three colour groups on on-tiles, two on the other tiles (group 2 absent), distinct grids: rows 0-5, 88-93,
    96-101 of the fp32 tile, and the x16 tile's alternate quads."""
    ck = F.Check()
    F.flow_groups(grid, Gpu, ck)
    _done(ck)


@pytest.mark.parametrize("grid", ["tiny", "odd"])
def test_samples_on_the_faces_and_integer_indices(grid):
    """Samples on the faces and next to the first and last four integer indices of every axis: the bar's reach and the hat
    weights' single rounding."""
    ck = F.Check()
    F.flow_faces(grid, Gpu, ck)
    o = F.bar_reach(F.faces_case(grid))
    assert int(o.min()) >= 0 and int(o.max()) <= 5, (int(o.min()), int(o.max()))
    _done(ck)


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
