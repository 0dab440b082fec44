"""The ray-march check without a GPU: march_check.check_variant (the comparison tests/test_gpu_march_ref64.py runs on the
kernels) on the binary32 emulation march_emu.Emu -- inside the bound of march_ref64.K_FAMILY on the GPU test's own inputs,
every flipped decision in its band (the bound is not too tight, the inputs are admissible) --, on every mutant of
march_emu.MUTANTS -- a miss in each family the mutant lists, on at least one small scene (the bound has teeth) --, the census
the GPU test requires on the restatement's own forward, and the checker on a backend with two planted errors."""
import math

import pytest
import torch

import march_check as M
import march_emu as E
import march_ref64 as R

_HOST = {}


def host_scene(name):
    """The GPU test's `odd` (as _select picks it) and `sat2`, and host-only scenes of the same generator: `prod40` (prod's
    seed and s_val on 40^3), `cap128` (the LDS-regime test's overflow case: its 101 rays of `odd`, max_steps = 128), `tiny`
    (9 x 11 x 13, for the cheap mutants), `mbox` (tiny with a mask box inside the scene box: mask-grid corners out of
    range with non-zero weight) and `flat` (tiny with a zero gradient grid and a block of SDF nodes at exactly 0, under
    fast_thres = 1e-6 so that its samples are visited: prv == nxt bit for bit on samples with neighbours, the exact ties of
    relu' = [pc > nc])."""
    if name in ("odd", "sat2"):
        return M.scene(name)
    if name not in _HOST:
        if name == "prod40":
            sc = R.box_scene((40, 40, 40), s_val=M.SCENES["prod"]["s_val"])
            inp = M._inputs(sc, M.SCENES["prod"]["pool"], M.SCENES["prod"]["seed"])
        elif name == "cap128":
            sc0, inp0 = M.scene("odd")
            sc = R.box_scene(sc0.dims, s_val=sc0.s_val, max_steps=128)
            inp = M._subset(inp0, torch.arange(0, inp0.rays_o.shape[0], 3)[:101])
        else:
            sc = R.box_scene((9, 11, 13), vox=1.0 / 6, s_val=12.0, fast_thres=1e-6 if name == "flat" else 1e-4)
            inp = M._inputs(sc, 96, 4)
            if name == "mbox":
                sc.mlo, sc.mhi = sc.lo * 0.75, sc.hi * 0.75
            if name == "flat":
                inp.gg.zero_()
                inp.sdf.sub_(0.6)
                inp.sdf[:5] = 0.0
        _HOST[name] = (sc, inp)
    return _HOST[name]


HOST_SCENES = ["tiny", "mbox", "flat", "sat2", "cap128", "prod40", "odd"]          # cheapest first
_CLEAN = {}


def run(name, coarse, ga, mut=None, census=None):
    sc, inp = host_scene(name)
    ck = M.Check()
    fw = M.check_variant(lambda *a: E.Emu(*a, mut=mut), sc, inp, coarse, ga, ck, census=census)
    return ck, fw


def clean(name, coarse, ga):
    if (name, coarse, ga) not in _CLEAN:
        census = {}
        ck, fw = run(name, coarse, ga, census=census)
        _CLEAN[(name, coarse, ga)] = (ck, fw, census)
    return _CLEAN[(name, coarse, ga)]


# ---- the emulation inside the bound -----------------------------------------------------------------------------------
@pytest.mark.parametrize("coarse,ga", M.VARIANTS)
@pytest.mark.parametrize("name", HOST_SCENES)
def test_emulation_inside_the_bound(name, coarse, ga):
    ck, fw, _ = clean(name, coarse, ga)
    print(f"\n[{name} coarse={coarse} ga={ga}] flips", ck.flips, "\nworst |emu - ref| / (2^-24 absref)",
          {k: round(v, 3) for k, v in sorted(ck.worst.items())})
    assert not ck.fails, ck.report()
    assert fw is not None
    if name == "cap128":
        assert int(fw.overflow.sum()) > 0 and int((~fw.overflow & (fw.n1 > 0)).sum()) > 0


def test_every_family_has_a_K_of_at_most_32():
    """K_FAMILY covers exactly the families the checker bounds, each a power of two of at most 32."""
    seen = set().union(*[set(clean(n, c, g)[0].worst) for n in HOST_SCENES for c, g in M.VARIANTS])
    assert seen == set(R.K_FAMILY), set(R.K_FAMILY) ^ seen
    for f, k in R.K_FAMILY.items():
        assert 0 < k <= 32 and math.log2(k) == int(math.log2(k)), (f, k)
    worst = {f: max(clean(n, c, g)[0].worst.get(f, 0.0) for n in HOST_SCENES for c, g in M.VARIANTS) for f in R.K_FAMILY}
    print("\nworst |emu - ref| / (2^-24 absref) over the host scenes", {k: round(v, 3) for k, v in sorted(worst.items())})


# ---- the census -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["odd", "sat2"])
def test_census_without_a_gpu(name):
    """The classes test_march_against_float64 requires, on the restatement's own forward (no backend's decisions); the
    binary32 alphas of `alpha==1` are the emulation's."""
    sc, inp = M.scene(name)
    fw = R.forward(sc, inp, False, False)
    q = E.Emu(sc, inp, False, False).phase2()
    census = M._census_fwd(fw, sc, inp, cached_alpha=q.alpha[q.live])
    missing = [k for k in M.NEED[name] if census.get(k, 0) == 0]
    assert not missing, (missing, census)


@pytest.mark.parametrize("coarse,ga", M.VARIANTS)
def test_no_transmittance_on_the_value_below_the_stop(coarse, ga):
    """No transmittance of any host scene lands on the binary32 neighbour below 1e-3f, the one value at which `<=` against
    the double 1e-3 rounded down differs from `< 1e-3f`: that mutant cannot be built on these scenes."""
    below = torch.nextafter(torch.tensor(R.T_STOP, dtype=torch.float32), torch.tensor(0.0))
    for name in HOST_SCENES:
        e = E.Emu(*host_scene(name), coarse, ga)
        q = e.phase2()
        firstT = e._chain(q.alpha, q.live if coarse else q.live & (q.alpha > E._f(e.sc.fast_thres)))      # (coarse: both passes)
        for T, last in ((q.T, q.last), (firstT[0], firstT[2])):
            assert not bool(((T == below) | (last == below)[:, None]).any()), name


# ---- the mutants ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutant", list(E.MUTANTS))
def test_mutant_of_the_emulation_breaks_the_bound(mutant):
    want = set(E.MUTANTS[mutant])
    variants = {f.split()[0] for f in want}
    killed = set()
    for name in HOST_SCENES:
        for coarse, ga in M.VARIANTS:
            fam = ("coarse" if coarse else "fine") + ("_ga" if ga else "")
            if fam not in variants or not {f for f in want - killed if f.split()[0] == fam}:
                continue
            killed |= run(name, coarse, ga, mut=mutant)[0].families() & want
        if killed == want:
            break
    assert killed == want, f"mutant `{mutant}` survives in {sorted(want - killed)}"


# ---- the checker itself -----------------------------------------------------------------------------------------------
def test_checker_reports_a_moved_cell_and_a_written_untouched_cell():
    """A backend whose BWD returns the restatement's own float64 grad_sdf with one touched cell moved by 2 K U absref and one
    untouched cell set to 1e-30: both are reported, the touched one by its position."""
    sc, inp = host_scene("tiny")
    planted = {}

    class Planted(E.Emu):
        def bwd(self, off3, dweight, dlast, rec=None, acc=0, cached=None):
            grad, ggrad, dsdf = super().bwd(off3, dweight, dlast, rec=rec, acc=acc, cached=cached)
            if rec is None and "cell" not in planted:
                fw = R.forward(sc, inp, False, False, planted["force"])
                slots, r = M._slots(fw, off3)
                gwp = torch.zeros(fw.s.shape, dtype=torch.float64).index_put((r["ray"], r["j"]), dweight[slots].double())
                u, v, a = R.backward(sc, inp, fw, gwp, dlast).grad_sdf
                g64 = torch.zeros(grad.numel(), dtype=torch.float64)
                g64[u] = v
                k = int(torch.argmax(a))
                g64[u[k]] += 2 * R.K_FAMILY["fine bwd"] * R.U * a[k]
                free = torch.ones(grad.numel(), dtype=torch.bool)
                free[u] = False
                z = int(torch.nonzero(free)[0, 0])
                g64[z] = 1e-30
                planted.update(cell=k, grid=int(u[k]), zero=z)
                return g64.view(sc.dims), ggrad, dsdf
            return grad, ggrad, dsdf

    # the decisions the checker will force (the emulation's own), to plant the restatement's values under them
    e = E.Emu(sc, inp, False, False)
    cc = e.count(cached=True)
    mkeys, cache, clive = M._mask_keys(cc["cache"], cc["stats"], sc, e.n)
    cnt = e.count()
    em = torch.randint(-1, 3, (e.n,), generator=torch.Generator().manual_seed(0), dtype=torch.int64)
    off3, hdr = e.plan(cnt["cnt3"], cnt["stats"], em)
    f = e.fill(off3, hdr[3])
    lv = f["ray"] >= 0
    planted["force"] = R.Force(mask_keys=mkeys, info=cache[:, 4].contiguous().view(torch.int32)[clive],
                               rec_keys=f["ray"][lv].long() * R.KEY + f["step"][lv].long())
    ck = M.Check()
    M.check_variant(lambda *a: Planted(*a), sc, inp, False, False, ck)
    msgs = [m for fam, m in ck.fails if fam == "fine bwd"]
    assert len(ck.fails) == 2 and len(msgs) == 2, ck.report()
    assert any(f"worst at {planted['cell']} (grid cell {planted['grid']}):" in m and "1 of" in m for m in msgs), msgs
    assert any(f"untouched cells are not 0 (first [{planted['zero']}]" in m for m in msgs), msgs
