"""Every entry point of the ray march (csrc/march.hip) against the float64 restatement in march_ref64.py -- not against one
another -- with a census of the classes each case claims to reach.

The comparison itself is march_check.check_variant (CPU-importable; tests/test_march_ref64_host.py runs it on a binary32
emulation and its mutants); this file holds the launches (`Run`) and asserts that the list of misses is empty.

Per-cell / per-value bound: |gpu - ref| <= K * 2^-24 * absref + FLOOR, K = march_ref64.K_FAMILY[family], absref from
march_ref64 (magnitudes plus the first-order error terms of the kernel's binary32 intermediates, its docstring); FLOOR covers
binary32 underflow of intermediates only.  Untouched cells stay exactly 0, every value is finite.  Counts, steps, info words,
ray ids and the plan are exact; transmittance from the cached COUNT pass is bit-exact given the kernel's own alphas.  Decisions that differ from
the restatement's must lie in their band (march_ref64.DEC_K); the flips are counted and printed (-s), as are the worst
ratios |gpu - ref| / (2^-24 absref) per entry-point family."""
import ctypes as C

import numpy as np
import pytest
import torch

import march_check as M
import march_ref64 as R
from march_check import VARIANTS, _subset, scene

pytestmark = pytest.mark.gpu

DEV = "cuda"
WORST = {}
FLIPS = {}


def _L():
    from esr_nerf_amd import _lib
    return _lib, _lib.lib()


# ---- GPU runs ---------------------------------------------------------------------------------------------------------
def _struct(scn):
    """the ABI's scene struct of a march_ref64.Scene"""
    from esr_nerf_amd import _lib
    sc = _lib.EsrScene()
    for i in range(3):
        sc.xyz_min[i], sc.xyz_max[i] = float(scn.lo[i]), float(scn.hi[i])
        sc.mask_min[i], sc.mask_max[i] = float(scn.mlo[i]), float(scn.mhi[i])
    sc.gx, sc.gy, sc.gz = scn.dims
    sc.mx, sc.my, sc.mz = scn.mdims
    sc.near_, sc.stepdist, sc.voxel_size = scn.near, scn.stepdist, scn.vox
    sc.act_shift, sc.mask_thres, sc.fast_thres, sc.s_val = scn.act_shift, scn.mask_thres, scn.fast_thres, scn.s_val
    sc.max_steps = scn.max_steps
    for i, v in enumerate((0.5, 1.0, 1.5, 2.0)):
        sc.grad_feat[i] = v
    return sc


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
        a = lib.EsrMarch(scene=C.pointer(_struct(self.sc)), rays_o=p(self.o), rays_d=p(self.d), mask_density=p(self.mask),
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
        n, L, sp = self.n, self.L, C.byref(_struct(self.sc))
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
def check_variant(sc, inp, coarse, ga, census=None, em_seed=0):
    """march_check.check_variant on the kernels; every miss it lists fails the test."""
    ck = M.Check()
    fw64 = M.check_variant(Run, sc, inp, coarse, ga, ck, census=census, em_seed=em_seed)
    for k, v in ck.worst.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
    for k, v in ck.flips.items():
        FLIPS[k] = FLIPS.get(k, 0) + v
    assert not ck.fails, ck.report()
    return fw64


@pytest.mark.parametrize("name", ["odd", "sat2", "prod"])
def test_march_against_float64(name):
    sc, inp = scene(name)
    census = {}
    for coarse, ga in VARIANTS:
        check_variant(sc, inp, coarse, ga, census=census if (coarse, ga) == (False, False) else None)
    print(f"\n[{name}] census", census, "\nflips", FLIPS, "\nworst |gpu - ref| / (2^-24 absref) (K_FAMILY in march_ref64.py)",
          {k: round(v, 3) for k, v in sorted(WORST.items())})
    need = M.NEED[name]
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
    print("\nworst |gpu - ref| / (2^-24 absref) so far", {k: round(v, 3) for k, v in sorted(WORST.items())})


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
