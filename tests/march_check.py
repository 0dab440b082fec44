"""The comparison of one ray-march backend with the float64 restatement march_ref64.py: inputs, scenes, census and
`check_variant`.  No device and no library here: a backend is any object with the four methods of the GPU test's `Run`
(the ctypes launches; tests/test_gpu_march_ref64.py) or of the binary32 emulation (march_emu.Emu; tests/test_march_ref64_host.py),

    count(cached=False) -> dict(cnt3, stats, last, cumw, plan[, cache])
    plan(cnt3, stats, em) -> (off3, header list)
    fill(off3, tiles, cached=None) -> dict(ray, step, w, sdf)
    bwd(off3, dweight, dlast, rec=None, acc=0, cached=None) -> (grad_sdf, grad_gg, dsdf_rec or None)

each returning CPU tensors in the ABI's layout; `make(sc, inp, coarse, ga)` builds one.

Per-cell / per-value bound: |got - ref| <= K * 2^-24 * absref + FLOOR with K = march_ref64.K_FAMILY[family], absref from
march_ref64 (magnitudes plus the first-order error terms of the kernel's binary32 intermediates, its docstring); FLOOR covers
binary32 underflow of intermediates only.  Untouched cells stay exactly 0, every value is finite.  Counts, steps, info words,
ray ids and the plan are exact; transmittance from the cached COUNT pass is bit-exact given the backend's own alphas.  Decisions
that differ from the restatement's must lie in their band (march_ref64.DEC_K).  Nothing raises: every miss is appended to
`Check.fails` as (family, message), the worst ratios |got - ref| / (2^-24 absref) per family go to `Check.worst`, the flips to
`Check.flips`."""
import numpy as np
import torch

import march_ref64 as R

FLOOR = 1e-30                   # absolute: binary32 intermediates of tiny upstream gradients (1e-7 times a sigmoid tail) underflow


class Check:
    """What one or more check_variant calls found."""

    def __init__(self, K=None):
        self.K = dict(R.K_FAMILY) if K is None else K
        self.fails, self.worst, self.flips = [], {}, {}

    def fail(self, family, msg):
        self.fails.append((family, msg))

    def exact(self, family, cond, msg):
        if not bool(cond):
            self.fail(family, msg)
        return bool(cond)

    def families(self):
        return {f for f, _ in self.fails}

    def report(self):
        return "\n".join(f"[{f}] {m}" for f, m in self.fails)


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


# what test_march_against_float64 requires of the census of each scene
NEED = {"odd": [f"n1={t}" for t in N1_TARGETS] + ["n1>256", "stop_lane0", "stop_lane0_seam", "stop_lane63", "stop_last",
                                                   "no_stop", "gap", "gap_at_seam", "pc<=nc", "miss", "start_inside",
                                                   "zero_dir", "idx_on_top", "tap_clamped"],
        "sat2": ["alpha==1", "stop_last", "tap_clamped", "idx_on_top"],
        "prod": ["no_stop", "stop_lane0", "miss", "zero_dir"]}


# ---- comparisons ------------------------------------------------------------------------------------------------------
def _bound(ck, family, gpu, ref, absref, what="", cells=None):
    """cells: the flat grid index of each value, named in the message of a miss"""
    K = ck.K[family]
    gpu, ref, absref = gpu.double(), ref.double(), absref.double()
    if not ck.exact(family, torch.isfinite(gpu).all(), f"{what}: non-finite values"):
        return
    err = (gpu - ref).abs()
    ratio = err / (R.U * absref).clamp_min(1e-300)
    bad = err > K * R.U * absref + FLOOR
    if gpu.numel():
        above = (err > 0) & (K * R.U * absref > FLOOR)          # (the ratio of a floor-bound value is not a measurement)
        ck.worst[family] = max(ck.worst.get(family, 0.0), float(torch.where(above, ratio, torch.zeros_like(ratio)).max()))
    if bool(bad.any()):
        at = int(torch.where(bad, ratio, torch.zeros_like(ratio)).argmax())
        where = at if cells is None else f"{at} (grid cell {int(cells[at])})"
        ck.fail(family, f"{what}: {int(bad.sum())} of {gpu.numel()} beyond K = {K} x 2^-24 absref; worst at {where}: got "
                        f"{float(gpu.reshape(-1)[at])} ref {float(ref.reshape(-1)[at])} ratio {float(ratio.reshape(-1)[at]):.4g}")


def _check_cells(ck, family, dense, cells, zero_also=None):
    u, v, a = cells
    flat = dense.reshape(-1).double()
    if not ck.exact(family, torch.isfinite(flat).all(), "non-finite cells"):
        return
    _bound(ck, family, flat[u], v, a, "touched cells", cells=u)
    untouched = torch.ones(flat.numel(), dtype=torch.bool)
    untouched[u] = False
    nz = untouched & (flat != 0)
    ck.exact(family, not bool(nz.any()),
             f"{int(nz.sum())} untouched cells are not 0 (first {torch.nonzero(nz)[:5, 0].tolist()})")


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


def _forward(ck, fam, *a, **k):
    """The restatement's forward under the backend's decisions; a decision off its band is a failure, not an exception."""
    try:
        return R.forward(*a, **k)
    except AssertionError as e:
        ck.fail(f"{fam} decisions", str(e))
        return None


def check_variant(make, sc, inp, coarse, ga, ck, census=None, em_seed=0):
    """COUNT, plan, FILL, BWD of one (COARSE, GA) variant of the backend `make(sc, inp, coarse, ga)` against the
    restatement; misses go to ck.fails.  Returns the restatement's forward (None when the comparison had to end early: a
    count, a decision or a record that is off leaves nothing to compare the later values with)."""
    run = make(sc, inp, coarse, ga)
    n = run.n
    fam = ("coarse" if coarse else "fine") + ("_ga" if ga else "")
    # the backend's mask-cache decisions (the walk is common to every variant) and, for interp, everything it caches
    cc = make(sc, inp, False, False).count(cached=True)
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
    if not ck.exact(f"{fam} plan", np.array_equal(off3.numpy(), ref_off) and hdr[:7] == ref_hdr, f"{hdr} != {ref_hdr}"):
        return None
    tiles = hdr[3]
    fill = run.fill(off3, tiles)
    live = fill["ray"] >= 0
    force.rec_keys = fill["ray"][live].long() * R.KEY + fill["step"][live].long()
    fw64 = _forward(ck, fam, sc, inp, coarse, ga, force)                 # float64 alphas and T (bounds of the uncached kernels)
    if fw64 is None:
        return None
    fwc = _forward(ck, fam, sc, inp, coarse, ga, force, alpha_in=alpha_in, s_in=s_in) if alpha_in is not None else fw64
    if fwc is None:
        return None
    for k, v in fw64.flips.items():
        ck.flips[(fam, k)] = ck.flips.get((fam, k), 0) + v
    # COUNT: counts exact, plan overflow bit, alphainv_last / cumw per ray
    e = f"{fam} count exact"
    good = ck.exact(e, torch.equal(cnt["cnt3"].long(), torch.where(fw64.overflow, 0, fw64.n3)), "cnt3")
    st = cnt["stats"].view(n, 3).long()
    for c_, ref in enumerate((fw64.n0, fw64.n1, fw64.n2)):
        good &= ck.exact(e, torch.equal(st[:, c_], torch.where(fw64.overflow, 0, ref)), f"ray_stats column {c_}")
    good &= ck.exact(e, (cnt["plan"][7].item() & 1) == int(bool(fw64.overflow.any())), "the plan's overflow bit")
    good &= ck.exact(e, (cnt["last"][fw64.overflow] == 1.0).all(), "alphainv_last of an overflow ray is not 1")
    if not good:
        return None
    ok = ~fw64.overflow
    _bound(ck, f"{fam} count last", cnt["last"][ok], fw64.last[ok], fw64.last_E[ok] + fw64.last[ok] * 4)
    if coarse:
        _bound(ck, f"{fam} count cumw", cnt["cumw"][ok], fw64.cumw[ok], fw64.cumw_M[ok] + 1e-30)
    if alpha_in is not None:
        # the cache rows per survivor: step and info exact, T bit-exact given the backend's alpha, sdf / alpha in the bound
        e = "fine cache exact"
        cs = cache[:, 1].contiguous().view(torch.int32)[clive].long()
        good = ck.exact(e, torch.equal(cs, fw64.step[fw64.live]), "steps")
        good &= ck.exact(e, torch.equal(force.info.long(), _info_of(fwc)[fwc.live]), "info words")
        good &= ck.exact(e, torch.equal(cache[:, 3][clive], fwc.T[fwc.live].float()), "T is not the serial product of the cached alphas")
        good &= ck.exact(e, torch.equal(cc["last"][ok], fwc.last[ok].float()), "alphainv_last is not the serial product of the cached alphas")
        _bound(ck, "fine cache sdf", cache[:, 0][clive], fw64.s[fw64.live], fw64.s_E[fw64.live] + fw64.s[fw64.live].abs())
        _bound(ck, "fine cache alpha", alpha_in, fw64.alpha[fw64.live], fw64.alpha_E[fw64.live])
        good &= ck.exact(e, torch.equal(cc["cnt3"], cnt["cnt3"]) and torch.equal(cc["stats"], cnt["stats"]),
                         "the cached COUNT's counts differ from the plain one's")
        if not good:
            return None
    # FILL: ray and step exact, w and sdf per record
    e = f"{fam} fill exact"
    slots, rec = _slots(fw64, off3)
    if not ck.exact(e, int(live.sum()) == slots.numel() == hdr[0] + hdr[1], "number of records"):
        return None
    if not ck.exact(e, torch.equal(fill["ray"][slots].long(), rec["ray"]) and torch.equal(fill["step"][slots].long(), rec["step"]),
                    "a record's ray or step is not at off3[ray] + rank"):
        return None
    _bound(ck, f"{fam} fill w", fill["w"][slots], rec["w"], rec["w_E"])
    _bound(ck, f"{fam} fill sdf", fill["sdf"][slots], rec["sdf"], rec["sdf_E"] + rec["sdf"].abs())
    if alpha_in is not None:
        e = "fine fill_cached exact"
        f2 = run.fill(off3, tiles, cached=cc)
        for k in ("ray", "step"):
            ck.exact(e, torch.equal(f2[k], fill[k]), k)
        rc = fwc.records()
        ck.exact(e, torch.equal(f2["w"][slots], (fwc.T[fwc.v3].float() * fwc.alpha[fwc.v3].float())), "w is not the cached T * alpha")
        ck.exact(e, torch.equal(f2["sdf"][slots], rc["sdf"].float()), "sdf is not the cached one")
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
        _check_cells(ck, f"{fam} bwd", grad, ref.grad_sdf)
        if coarse and ga:
            _check_cells(ck, f"{fam} bwd grad_gg", ggrad, ref.grad_gg)
        if coarse or ga:
            continue
        for acc in (0, 1):
            pre = torch.full((m,), float("nan")) if acc == 0 else torch.randn(m, generator=torch.Generator().manual_seed(acc))
            for which, fw_ in (("bwd_rec", fw64), ("bwd_cached", fwc)):
                rr = R.backward(sc, inp, fw_, gwp, dlast, rec_mode=True)
                grad, _, dsdf = run.bwd(off3, dweight, dlast, rec=pre.clone(), acc=acc,
                                        cached=cc if which == "bwd_cached" else None)
                _check_cells(ck, f"fine {which}", grad, rr.grad_sdf)
                ck.exact(f"fine {which}", (grad.reshape(-1)[rr.rec_only_cells] == 0).all(),
                         "a cell that only recorded samples' value taps reach is not 0")
                pairs, val, mag = rr.dsdf
                sl = off3.long()[pairs[:, 0]] + pairs[:, 1]
                base = pre[sl].double() if acc else torch.zeros_like(val)
                _bound(ck, f"fine {which} dsdf_rec", dsdf[sl], base + val, mag + (base.abs() if acc else 0), f"accumulate = {acc}")
                untouched = torch.ones(m, dtype=torch.bool)
                untouched[sl] = False
                same = (dsdf[untouched] == pre[untouched]) | (torch.isnan(dsdf[untouched]) & torch.isnan(pre[untouched]))
                ck.exact(f"fine {which} dsdf_rec", same.all(), "dsdf_rec slots without a record were written")
    if census is not None:
        ca = _census_fwd(fwc, sc, inp, cached_alpha=alpha_in)
        ca["relu_kink_band"] = fw64.census.get("relu_kink", 0)
        for k, v in ca.items():
            census[k] = census.get(k, 0) + v
    return fw64


VARIANTS = [(False, False), (False, True), (True, False), (True, True)]
