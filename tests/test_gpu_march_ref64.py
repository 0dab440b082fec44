"""Every entry point of the ray march (csrc/march.hip) against the float64 restatement in march_ref64.py -- not against one
another -- with a census of the classes each case claims to reach.

Per-cell / per-value bound: |gpu - ref| <= K * 2^-24 * absref + FLOOR, absref from march_ref64 (magnitudes plus the
first-order error terms of the kernel's binary32 intermediates, its docstring); FLOOR covers binary32 underflow of
intermediates only.  Untouched cells stay exactly 0, every value is finite.  Counts, steps, info words, ray ids and the plan
are exact; transmittance from the cached COUNT pass is bit-exact given the kernel's own alphas.  Decisions that differ from
the restatement's must lie in their band (march_ref64.DEC_K); the flips are counted and printed (-s), as are the worst
ratios |gpu - ref| / (2^-24 absref) per entry-point family."""
import ctypes as C

import numpy as np
import pytest
import torch

import march_ref64 as R

pytestmark = pytest.mark.gpu

K = 32
FLOOR = 1e-30                   # absolute: binary32 intermediates of tiny upstream gradients (1e-7 times a sigmoid tail) underflow
DEV = "cuda"
WORST = {}
FLIPS = {}


def _L():
    from esr_nerf_amd import _lib
    return _lib, _lib.lib()


# ---- scenes -----------------------------------------------------------------------------------------------------------
def _inputs(sc, N, seed):
    g = torch.Generator().manual_seed(seed)
    lo, hi = sc.lo, sc.hi
    ext = hi - lo
    kinds = torch.randint(0, 6, (N,), generator=g)
    o = lo + ext * torch.rand(N, 3, generator=g)
    d = torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=1)
    out = kinds == 0                                            # from outside, through the box
    o[out] = (o[out] - d[out] * float(ext.norm()))
    ax = kinds == 1                                             # axis-aligned: zero direction components
    a = torch.randint(0, 3, (N,), generator=g)
    dd = torch.zeros(N, 3)
    dd[torch.arange(N), a] = torch.where(torch.rand(N, generator=g) < 0.5, -1.0, 1.0)
    d[ax] = dd[ax]
    gr = kinds == 2                                             # grazing the high y face (samples on index dims - 1)
    o[gr, 1] = hi[1]
    d[gr, 1] = 0.0
    ms = kinds == 3                                             # missing the box
    o[ms] = hi + 0.3 + torch.rand(int(ms.sum()), 3, generator=g)
    d[ms] = torch.nn.functional.normalize(torch.rand(int(ms.sum()), 3, generator=g) + 0.1, dim=1)
    # kinds 4, 5: start inside the box
    xs = [torch.linspace(float(lo[i]), float(hi[i]), sc.dims[i]) for i in range(3)]
    X, Y, Z = torch.meshgrid(*xs, indexing="ij")
    z0 = 0.25 * torch.sin(3.0 * X) * torch.cos(2.0 * Y)
    sdf = torch.minimum(Z - z0, 0.9 - (X ** 2 + Y ** 2).sqrt()) + 0.01 * torch.randn(*sc.dims, generator=g)
    mask = torch.full(sc.mdims, 6.0)
    blk = torch.rand(*[(m + 3) // 4 for m in sc.mdims], generator=g) < 0.2   # pruned 4^3 blocks: gaps in the survivors
    blk = blk.repeat_interleave(4, 0).repeat_interleave(4, 1).repeat_interleave(4, 2)[:sc.mdims[0], :sc.mdims[1], :sc.mdims[2]]
    mask[blk] = -9.0
    gg = (0.8 * torch.randn(*sc.dims, 3, generator=g)).float()
    return R.Inputs(rays_o=o.float(), rays_d=d.float(), viewdirs=torch.nn.functional.normalize(d, dim=1).float(),
                    mask=mask.float(), sdf=sdf.float(), gg=gg)


def _subset(inp, idx):
    return R.Inputs(rays_o=inp.rays_o[idx].contiguous(), rays_d=inp.rays_d[idx].contiguous(),
                    viewdirs=inp.viewdirs[idx].contiguous(), mask=inp.mask, sdf=inp.sdf, gg=inp.gg)


N1_TARGETS = (0, 1, 2, 63, 64, 65, 127, 128, 129)


def _stop_pos(fw):
    """position of the early stop per ray (-1: none)"""
    L = fw.proc.shape[1]
    P = torch.arange(L)[None]
    lastp = torch.where(fw.proc.any(1), (fw.proc * (P + 1)).max(1).values - 1, torch.full((fw.N,), -1))
    stopped = fw.last < R.T_STOP
    return torch.where(stopped, lastp, torch.full_like(lastp, -1))


def _select(sc, inp, per_class=3, extra=150):
    """Rays of a candidate pool chosen by the classes of the restatement (interp): the n1 targets, rays over 256
    survivors, stops in lane 0 / lane 63 / on the last survivor, and a random rest."""
    fw = R.forward(sc, inp, coarse=False, ga=False)
    sp = _stop_pos(fw)
    n1 = fw.n1
    pick = []
    for t in N1_TARGETS:
        pick += torch.nonzero(n1 == t)[:per_class, 0].tolist()
    pick += torch.nonzero(n1 > 256)[:per_class, 0].tolist()
    pick += torch.nonzero((sp >= 0) & (sp % 64 == 0) & (sp >= 64))[:per_class, 0].tolist()
    pick += torch.nonzero((sp >= 0) & (sp % 64 == 0))[:per_class, 0].tolist()
    pick += torch.nonzero((sp >= 0) & (sp % 64 == 63))[:per_class, 0].tolist()
    pick += torch.nonzero((sp >= 0) & (sp == n1 - 1))[:per_class, 0].tolist()
    pick += torch.nonzero(fw.overflow)[:per_class, 0].tolist()
    g = torch.Generator().manual_seed(5)
    pick += torch.randperm(fw.N, generator=g)[:extra].tolist()
    idx = torch.tensor(sorted(set(pick)))
    return idx


SCENES = {
    # odd dims with a long axis (rays over 256 survivors), s_val where the surfaces stop rays at every lane
    "odd": dict(dims=(37, 61, 151), s_val=40.0, pool=6000, seed=1),
    # one 2-wide axis, alpha saturating to 1.0f
    "sat2": dict(dims=(2, 45, 33), s_val=4000.0, pool=400, seed=2),
    # production-size grid, a subset of rays
    "prod": dict(dims=(160, 160, 160), s_val=80.0, pool=300, seed=3),
}
_CACHE = {}


def scene(name):
    if name not in _CACHE:
        cfg = SCENES[name]
        sc = R.box_scene(cfg["dims"], s_val=cfg["s_val"])
        inp = _inputs(sc, cfg["pool"], cfg["seed"])
        if name == "odd":
            inp = _subset(inp, _select(sc, inp))
        _CACHE[name] = (sc, inp)
    return _CACHE[name]


# ---- GPU runs ---------------------------------------------------------------------------------------------------------
def _dev(t):
    return t.to(DEV).contiguous()


class Run:
    """Device inputs of one (scene, variant); every entry point as a method returning its outputs."""

    def __init__(self, sc, inp, coarse, ga):
        self.lib, self.L = _L()
        self.sc, self.inp, self.coarse, self.ga = sc, inp, coarse, ga
        self.s = self.lib.stream_ptr(DEV)
        self.o, self.d, self.vd = _dev(inp.rays_o), _dev(inp.rays_d), _dev(inp.viewdirs)
        self.mask, self.sdf, self.gg = _dev(inp.mask), _dev(inp.sdf), _dev(inp.gg)
        self.n = inp.rays_o.shape[0]

    def p(self, t):
        return self.lib.ptr(t)

    def args(self, **own):
        """The argument struct of the three passes for this (coarse, ga) with the pass's ``own`` fields (tensors, or ints)."""
        lib, p = self.lib, self.p
        a = lib.EsrMarch(scene=C.pointer(self.sc.struct()), rays_o=p(self.o), rays_d=p(self.d), mask_density=p(self.mask),
                         sdf=p(self.sdf), n_rays=self.n,
                         flags=(lib.MARCH_COARSE if self.coarse else 0) | (lib.MARCH_GRAD_ALPHA if self.ga else 0))
        if self.ga:
            a.viewdirs = p(self.vd)
        if self.coarse and self.ga:
            a.gg = p(self.gg)
        for k, v in own.items():
            setattr(a, k, v if isinstance(v, int) else p(v))
        return a

    def count(self, cached=False, expect=0):
        n, L, sp = self.n, self.L, C.byref(self.sc.struct())
        i32 = lambda k: torch.full((k,), -7, dtype=torch.int32, device=DEV)
        out = dict(cnt3=i32(n), stats=i32(3 * n), last=torch.full((n,), -7.0, device=DEV),
                   cumw=torch.full((n,), -7.0, device=DEV), plan=torch.zeros(8, dtype=torch.int32, device=DEV))
        own = dict(cnt3=out["cnt3"], alphainv_last=out["last"], ray_stats=out["stats"], plan=out["plan"])
        if self.coarse:
            own["cum_weights"] = out["cumw"]
        if cached:
            out["cache"] = own["cache"] = torch.full((int(L.esr_fine_march_cache_floats(sp, n)),), -7.0, device=DEV)
        rc = L.esr_march_count(self.args(**own), self.s)
        assert rc == expect, rc
        torch.cuda.synchronize()
        return {k: v.cpu() for k, v in out.items()}

    def plan(self, cnt3, stats, em):
        n = self.n
        off3 = torch.full((n,), -7, dtype=torch.int32, device=DEV)
        plan = torch.zeros(8, dtype=torch.int32, device=DEV)
        dc, de, ds = _dev(cnt3), _dev(em), _dev(stats)          # (held: a freed temporary's block is reused at once)
        self.lib.check(self.L.esr_fine_plan(self.p(dc), self.p(de), self.p(ds), n, self.p(off3), self.p(plan), self.s), "plan")
        torch.cuda.synchronize()
        return off3.cpu(), plan.cpu().tolist()

    def fill(self, off3, tiles, cached=None, expect=0):
        m = max(tiles, 1) * 32
        out = dict(ray=torch.full((m,), -1, dtype=torch.int32, device=DEV), step=torch.full((m,), -7, dtype=torch.int32, device=DEV),
                   w=torch.full((m,), -7.0, device=DEV), sdf=torch.full((m,), -7.0, device=DEV))
        own = dict(off3=_dev(off3), rec_ray=out["ray"], rec_step=out["step"], rec_w=out["w"], rec_sdf=out["sdf"])
        if cached is not None:
            own.update(ray_stats=_dev(cached["stats"]), cache=_dev(cached["cache"]))
        rc = self.L.esr_march_fill(self.args(**own), self.s)
        assert rc == expect, rc
        torch.cuda.synchronize()
        return {k: v.cpu() for k, v in out.items()}

    def bwd(self, off3, dweight, dlast, rec=None, acc=0, cached=None, prefill=None, expect=0):
        """rec: None (plain) or a prefilled dsdf_rec array; cached: the cached COUNT's outputs."""
        grad = torch.zeros(self.sdf.shape, device=DEV)
        ggrad = torch.zeros(self.gg.shape, device=DEV)
        dsdf = _dev(rec) if rec is not None else None
        own = dict(off3=_dev(off3), dweight=_dev(dweight), dlast=_dev(dlast), grad_sdf=grad, dsdf_rec=dsdf, accumulate=acc)
        if self.coarse and self.ga:
            own["grad_gg"] = ggrad
        if cached is not None:
            own.update(ray_stats=_dev(cached["stats"]), alphainv_last=_dev(cached["last"]), cache=_dev(cached["cache"]))
        rc = self.L.esr_march_bwd(self.args(**own), self.s)
        assert rc == expect, rc
        torch.cuda.synchronize()
        return grad.cpu(), ggrad.cpu(), None if dsdf is None else dsdf.cpu()


# ---- comparisons ------------------------------------------------------------------------------------------------------
def _bound(family, gpu, ref, absref, what=""):
    gpu, ref, absref = gpu.double(), ref.double(), absref.double()
    assert bool(torch.isfinite(gpu).all()), f"{family} {what}: non-finite values"
    err = (gpu - ref).abs()
    ratio = err / (R.U * absref).clamp_min(1e-300)
    bad = err > K * R.U * absref + FLOOR
    if gpu.numel():
        above = (err > 0) & (K * R.U * absref > FLOOR)          # (the ratio of a floor-bound value is not a measurement)
        WORST[family] = max(WORST.get(family, 0.0), float(torch.where(above, ratio, torch.zeros_like(ratio)).max()))
    assert not bool(bad.any()), (f"{family} {what}: {int(bad.sum())} of {gpu.numel()} beyond K 2^-24 absref; worst at "
                                 f"{int(ratio.argmax())}: gpu {float(gpu.reshape(-1)[ratio.argmax()])} ref "
                                 f"{float(ref.reshape(-1)[ratio.argmax()])}")


def _check_cells(family, dense, cells, zero_also=None):
    u, v, a = cells
    flat = dense.reshape(-1).double()
    assert bool(torch.isfinite(flat).all()), family
    _bound(family, flat[u], v, a, "touched cells")
    untouched = torch.ones(flat.numel(), dtype=torch.bool)
    untouched[u] = False
    nz = untouched & (flat != 0)
    assert not bool(nz.any()), f"{family}: {int(nz.sum())} untouched cells are not 0 (first {torch.nonzero(nz)[:5, 0].tolist()})"


def _info_of(fw):
    return (fw.v2.long() | (fw.proc.long() << 1) | torch.where(fw.v3, (fw.rank + 1) << 8, torch.zeros_like(fw.rank)))


def _mask_keys(cache, stats, sc, n):
    cap = sc.cap
    c = cache.view(n, 5, cap)
    n1 = stats.view(n, 3)[:, 1].long()
    live = torch.arange(cap)[None] < n1[:, None]
    steps = c[:, 1].contiguous().view(torch.int32).long()
    r = torch.nonzero(live)[:, 0]
    return (r * R.KEY + steps[live]), c, live


def _census_fwd(fw, sc, inp, cached_alpha=None):
    """classes reached by one forward (interp: lanes / chunk seams; all: geometry)"""
    sp = _stop_pos(fw)
    n1 = fw.n1
    c = {f"n1={t}": int((n1 == t).sum()) for t in N1_TARGETS}
    c["n1>256"] = int((n1 > 256).sum())
    c["stop_lane0"] = int(((sp >= 0) & (sp % 64 == 0)).sum())
    c["stop_lane0_seam"] = int(((sp >= 64) & (sp % 64 == 0)).sum())
    c["stop_lane63"] = int(((sp >= 0) & (sp % 64 == 63)).sum())
    c["stop_last"] = int(((sp >= 0) & (sp == n1 - 1)).sum())
    c["no_stop"] = int(((sp < 0) & (n1 > 0)).sum())
    L = fw.live.shape[1]
    P = torch.arange(L)[None]
    # neighbour pairs that straddle a gap (non-consecutive steps) across a chunk seam (positions 63 | 64)
    gap = fw.live & (P > 0) & (fw.step - torch.cat([fw.step[:, :1], fw.step[:, :-1]], 1) > 1)
    c["gap"] = int(gap.sum())
    c["gap_at_seam"] = int((gap & (P % 64 == 0)).sum())
    c["pc<=nc"] = int((fw.proc & (fw.pc <= fw.nc)).sum())
    c["overflow"] = int(fw.overflow.sum())
    c["miss"] = int(((fw.n0 == 0) & ~fw.overflow).sum())
    lo, hi = inp.rays_o > sc.lo, inp.rays_o < sc.hi
    c["start_inside"] = int((lo & hi).all(1).sum())
    c["zero_dir"] = int((inp.rays_d == 0).any(1).sum())
    top = torch.tensor([d - 1 for d in sc.dims], dtype=torch.float32)
    c["idx_on_top"] = int(((fw.ind == top) & fw.live[..., None]).any(-1).sum())
    c["tap_clamped"] = int((((fw.ind + 1 > top) | (fw.ind - 1 < 0)) & fw.live[..., None]).any(-1).sum())
    if cached_alpha is not None:
        c["alpha==1"] = int((cached_alpha == 1.0).sum())
    return c


def _gw(fw, seed, mode):
    """dweight per record [N, L] (scales 1e-7..30, zeros on some) and dlast [N]: mode mixed / dlast / dweight"""
    g = torch.Generator().manual_seed(seed)
    N, L = fw.s.shape
    scale = 10.0 ** (torch.rand(N, 1, generator=g) * 8.5 - 7)
    gw = torch.randn(N, L, generator=g) * scale
    gw[torch.rand(N, L, generator=g) < 0.2] = 0.0
    dlast = torch.randn(N, generator=g) * scale[:, 0]
    dlast[torch.rand(N, generator=g) < 0.2] = 0.0
    if mode == "dlast":
        gw.zero_()
    if mode == "dweight":
        dlast.zero_()
    return gw.float(), dlast.float()


def _slots(fw, off3):
    rec = fw.records()
    return off3.long()[rec["ray"]] + rec["rank"], rec


def check_variant(sc, inp, coarse, ga, census=None, em_seed=0):
    """COUNT, plan, FILL, BWD of one (COARSE, GA) variant against the restatement; returns its forward census."""
    run = Run(sc, inp, coarse, ga)
    n = run.n
    # the kernel's mask-cache decisions (the walk is common to every variant) and, for interp, everything it caches
    cc = Run(sc, inp, False, False).count(cached=True)
    mkeys, cache, clive = _mask_keys(cc["cache"], cc["stats"], sc, n)
    force = R.Force(mask_keys=mkeys)
    alpha_in = s_in = None
    if not coarse and not ga:
        force.info = cache[:, 4].contiguous().view(torch.int32)[clive]
        alpha_in, s_in = cache[:, 2][clive], cache[:, 0][clive]
    cnt = run.count()
    g = torch.Generator().manual_seed(em_seed)
    em = torch.randint(-1, 3, (n,), generator=g, dtype=torch.int64)      # values outside {0, 1} included
    off3, hdr = run.plan(cnt["cnt3"], cnt["stats"], em)
    ref_off, ref_hdr = R.plan(cnt["cnt3"].numpy(), em.numpy(), cnt["stats"].numpy())
    assert np.array_equal(off3.numpy(), ref_off) and hdr[:7] == ref_hdr, (hdr, ref_hdr)
    tiles = hdr[3]
    fill = run.fill(off3, tiles)
    live = fill["ray"] >= 0
    force.rec_keys = fill["ray"][live].long() * R.KEY + fill["step"][live].long()
    fam = ("coarse" if coarse else "fine") + ("_ga" if ga else "")
    fw64 = R.forward(sc, inp, coarse, ga, force)                       # float64 alphas and T (bounds of the uncached kernels)
    fwc = R.forward(sc, inp, coarse, ga, force, alpha_in=alpha_in, s_in=s_in) if alpha_in is not None else fw64
    for k, v in fw64.flips.items():
        FLIPS[(fam, k)] = FLIPS.get((fam, k), 0) + v
    # COUNT: counts exact, plan overflow bit, alphainv_last / cumw per ray
    assert torch.equal(cnt["cnt3"].long(), torch.where(fw64.overflow, 0, fw64.n3)), fam
    st = cnt["stats"].view(n, 3).long()
    for c_, ref in enumerate((fw64.n0, fw64.n1, fw64.n2)):
        assert torch.equal(st[:, c_], torch.where(fw64.overflow, 0, ref)), (fam, c_)
    assert (cnt["plan"][7].item() & 1) == int(bool(fw64.overflow.any())), fam
    assert bool((cnt["last"][fw64.overflow] == 1.0).all())
    ok = ~fw64.overflow
    _bound(f"{fam} count last", cnt["last"][ok], fw64.last[ok], fw64.last_E[ok] + fw64.last[ok] * 4)
    if coarse:
        _bound(f"{fam} count cumw", cnt["cumw"][ok], fw64.cumw[ok], fw64.cumw_M[ok] + 1e-30)
    if alpha_in is not None:
        # the cache rows per survivor: step and info exact, T bit-exact given the kernel's alpha, sdf / alpha in the bound
        cs = cache[:, 1].contiguous().view(torch.int32)[clive].long()
        assert torch.equal(cs, fw64.step[fw64.live])
        assert torch.equal(force.info.long(), _info_of(fwc)[fwc.live])
        assert torch.equal(cache[:, 3][clive], fwc.T[fwc.live].float())
        assert torch.equal(cc["last"][ok], fwc.last[ok].float())
        _bound("fine cache sdf", cache[:, 0][clive], fw64.s[fw64.live], fw64.s_E[fw64.live] + fw64.s[fw64.live].abs())
        _bound("fine cache alpha", alpha_in, fw64.alpha[fw64.live], fw64.alpha_E[fw64.live])
        assert torch.equal(cc["cnt3"], cnt["cnt3"]) and torch.equal(cc["stats"], cnt["stats"])
    # FILL: ray and step exact, w and sdf per record
    slots, rec = _slots(fw64, off3)
    assert int(live.sum()) == slots.numel() == hdr[0] + hdr[1]
    assert torch.equal(fill["ray"][slots].long(), rec["ray"]) and torch.equal(fill["step"][slots].long(), rec["step"])
    _bound(f"{fam} fill w", fill["w"][slots], rec["w"], rec["w_E"])
    _bound(f"{fam} fill sdf", fill["sdf"][slots], rec["sdf"], rec["sdf_E"] + rec["sdf"].abs())
    if alpha_in is not None:
        f2 = run.fill(off3, tiles, cached=cc)
        for k in ("ray", "step"):
            assert torch.equal(f2[k], fill[k])
        rc = fwc.records()
        assert torch.equal(f2["w"][slots], (fwc.T[fwc.v3].float() * fwc.alpha[fwc.v3].float()))
        assert torch.equal(f2["sdf"][slots], rc["sdf"].float())
    # BWD
    m = max(tiles, 1) * 32
    modes = ("mixed", "dlast", "dweight") if not (coarse or ga) else ("mixed",)
    for mi, mode in enumerate(modes):
        gw, dlast = _gw(fw64, 11 + mi, mode)
        dweight = torch.zeros(m)
        dweight[slots] = gw[rec["ray"], rec["j"]]
        gwp = torch.zeros(fw64.s.shape, dtype=torch.float64).index_put((rec["ray"], rec["j"]), dweight[slots].double())
        ref = R.backward(sc, inp, fw64, gwp, dlast)
        grad, ggrad, _ = run.bwd(off3, dweight, dlast)
        _check_cells(f"{fam} bwd", grad, ref.grad_sdf)
        if coarse and ga:
            _check_cells(f"{fam} bwd grad_gg", ggrad, ref.grad_gg)
        if coarse or ga:
            continue
        for acc in (0, 1):
            pre = torch.full((m,), float("nan")) if acc == 0 else torch.randn(m, generator=torch.Generator().manual_seed(acc))
            for which, fw_ in (("bwd_rec", fw64), ("bwd_cached", fwc)):
                rr = R.backward(sc, inp, fw_, gwp, dlast, rec_mode=True)
                grad, _, dsdf = run.bwd(off3, dweight, dlast, rec=pre.clone(), acc=acc,
                                        cached=cc if which == "bwd_cached" else None)
                _check_cells(f"fine {which}", grad, rr.grad_sdf)
                assert bool((grad.reshape(-1)[rr.rec_only_cells] == 0).all())
                pairs, val, mag = rr.dsdf
                sl = off3.long()[pairs[:, 0]] + pairs[:, 1]
                base = pre[sl].double() if acc else torch.zeros_like(val)
                _bound(f"fine {which} dsdf_rec", dsdf[sl], base + val, mag + (base.abs() if acc else 0))
                untouched = torch.ones(m, dtype=torch.bool)
                untouched[sl] = False
                same = (dsdf[untouched] == pre[untouched]) | (torch.isnan(dsdf[untouched]) & torch.isnan(pre[untouched]))
                assert bool(same.all()), f"{which}: dsdf_rec slots without a record were written"
    if census is not None:
        ca = _census_fwd(fwc, sc, inp, cached_alpha=alpha_in)
        ca["relu_kink_band"] = fw64.census.get("relu_kink", 0)
        for k, v in ca.items():
            census[k] = census.get(k, 0) + v
    return fw64


VARIANTS = [(False, False), (False, True), (True, False), (True, True)]


@pytest.mark.parametrize("name", ["odd", "sat2", "prod"])
def test_march_against_float64(name):
    sc, inp = scene(name)
    census = {}
    for coarse, ga in VARIANTS:
        check_variant(sc, inp, coarse, ga, census=census if (coarse, ga) == (False, False) else None)
    print(f"\n[{name}] census", census, "\nflips", FLIPS, "\nworst |gpu - ref| / (2^-24 absref) (K =", K, ")",
          {k: round(v, 3) for k, v in sorted(WORST.items())})
    need = {"odd": [f"n1={t}" for t in N1_TARGETS] + ["n1>256", "stop_lane0", "stop_lane0_seam", "stop_lane63", "stop_last",
                                                       "no_stop", "gap", "gap_at_seam", "pc<=nc", "miss", "start_inside",
                                                       "zero_dir", "idx_on_top", "tap_clamped"],
            "sat2": ["alpha==1", "stop_last", "tap_clamped", "idx_on_top"],
            "prod": ["no_stop", "stop_lane0", "miss", "zero_dir"]}[name]
    missing = [k for k in need if census.get(k, 0) == 0]
    assert not missing, (missing, census)


# ---- LDS regimes, overflow rays, refusal ------------------------------------------------------------------------------
def regime(mode, ga, cap):
    """launch_march's choice: 4 / 2 / 1 waves per block, 'optin' above 64 KB, 'ecap' (including the backward's bound)"""
    narr = (5 if mode == "bwd" else 2) + (1 if ga else 0)
    per_wave = narr * cap * 4
    wpb = 4
    while wpb > 1 and per_wave * wpb > 64 * 1024:
        wpb >>= 1
    if per_wave * wpb > 160 * 1024 or (5 + (1 if ga else 0)) * cap * 4 > 160 * 1024:
        return "ecap"
    return "optin" if per_wave * wpb > 64 * 1024 else wpb


CAPS = {False: (128, 768, 1600, 2048, 3264, 4096, 8192, 8256), True: (128, 640, 1344, 2688, 5440, 6784, 6848)}


@pytest.mark.parametrize("coarse,ga", VARIANTS)
def test_march_lds_regimes_and_refusal(coarse, ga):
    """Every cap regime of COUNT / FILL / BWD against the restatement (overflow rays mixed in at cap 128: an odd ray
    count, so blocks hold rays of both kinds and a partial last block), and the first refused cap: ESR_ECAP with no output
    touched."""
    sc0, inp0 = scene("odd")
    idx = torch.arange(0, inp0.rays_o.shape[0], 3)[:101]
    inp = _subset(inp0, idx)
    reached = {m: set() for m in ("count", "fill", "bwd")}
    for cap in CAPS[ga]:
        sc = R.box_scene(sc0.dims, s_val=sc0.s_val, max_steps=cap)
        for m in reached:
            reached[m].add(regime(m, ga, cap))
        if regime("bwd", ga, cap) == "ecap":
            run = Run(sc, inp, coarse, ga)
            out = run.count(expect=-2)
            assert bool((out["cnt3"] == -7).all()) and bool((out["last"] == -7).all()) and bool((out["stats"] == -7).all())
            assert bool((out["plan"] == 0).all())
            off3 = torch.zeros(run.n, dtype=torch.int32)
            f = run.fill(off3, 4, expect=-2)
            assert bool((f["ray"] == -1).all()) and bool((f["w"] == -7).all())
            grad, ggrad, _ = run.bwd(off3, torch.zeros(128), torch.zeros(run.n), expect=-2)
            assert not bool(grad.any()) and not bool(ggrad.any())
            continue
        fw = check_variant(sc, inp, coarse, ga)
        if cap == 128:
            assert int(fw.overflow.sum()) > 0 and int((~fw.overflow & (fw.n1 > 0)).sum()) > 0
    for m, regs in reached.items():
        want = {4, 2, 1, "optin", "ecap"} if (m == "bwd" or ga) else {4, 2, 1, "ecap"}
        assert want <= regs, (m, regs)


# ---- plan -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 1023, 1024, 1025, 2047, 2048, 2049, 64 * 2048 + 1, 70001])
def test_plan_against_numpy(n):
    """esr_fine_plan and esr_fine_plan_totals + esr_fine_plan_offsets against the numpy restatement: offsets, n_on / n_off,
    tiles, m0..m2 and the overflow word (bit 0 as the march leaves it), with em_modes outside {0, 1}."""
    lib, L = _L()
    s = lib.stream_ptr(DEV)
    g = torch.Generator().manual_seed(n)
    cnt3 = torch.randint(0, 70, (n,), generator=g, dtype=torch.int32)
    em = torch.randint(-2, 4, (n,), generator=g, dtype=torch.int64)
    stats = torch.randint(0, 300, (3 * n,), generator=g, dtype=torch.int32)
    ref_off, ref_hdr = R.plan(cnt3.numpy(), em.numpy(), stats.numpy())
    p = lambda t: lib.ptr(t)
    dc, de, ds = _dev(cnt3), _dev(em), _dev(stats)
    for pre in (0, 1):
        off_a = torch.full((max(n, 1),), -7, dtype=torch.int32, device=DEV)
        off_b = off_a.clone()
        plan_a = torch.zeros(8, dtype=torch.int32, device=DEV)
        plan_a[7] = pre
        plan_b = plan_a.clone()
        lib.check(L.esr_fine_plan(p(dc), p(de), p(ds), n, p(off_a), p(plan_a), s), "plan")
        lib.check(L.esr_fine_plan_totals(p(dc), p(de), p(ds), n, p(plan_b), s), "totals")
        torch.cuda.synchronize()
        hb = plan_b.cpu().tolist()
        lib.check(L.esr_fine_plan_offsets(p(dc), p(de), n, p(off_b), p(plan_b), s), "offsets")
        torch.cuda.synchronize()
        ha = plan_a.cpu().tolist()
        assert ha[:7] == ref_hdr and (ha[7] & 1) == pre, (ha, ref_hdr)
        assert hb[0:2] == ref_hdr[0:2] and hb[4:7] == ref_hdr[4:7] and (hb[7] & 1) == pre
        assert plan_b.cpu().tolist()[:7] == ref_hdr
        assert np.array_equal(off_a.cpu()[:n].numpy(), ref_off) and np.array_equal(off_b.cpu()[:n].numpy(), ref_off)
        if n:
            on = em.numpy() == 1
            if (~on).any():
                assert int(off_a.cpu()[:n].numpy()[~on].min()) % 32 == 0 or ref_off[~on].min() == (ref_hdr[0] + 31) // 32 * 32
